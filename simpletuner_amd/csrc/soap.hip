// soap.hip — SOAP (optimizers/soap/__init__.py: Adam in the eigenbasis of Shampoo's preconditioner) over the fp32 LoRA adapter arena, with the
// RANK side of every adapter matrix preconditioned and the long side left as identity (max_precond_dim between the two sides).
//
// Every matrix is worked on as r x L, short side first (m itself, or m^T if tall), r <= 128, R = r rounded up to 32.  Per matrix the state is
// GG (r x r, the running g g^T) and Q (r x r, its eigenbasis), both dense in two flat arenas; exp_avg lives in the original basis, exp_avg_sq
// in the rotated one.  A call is a fixed number of launches whatever the number of matrices:
//   step    one workgroup per 512-column chunk, Q in LDS: g <- s g; m <- b1 m + (1-b1) g; gp = Q^T g; v <- b2 v + (1-b2) gp^2; mp = Q^T m;
//           u = Q (mp / (sqrt(v) + eps)); p <- p - step_size u; p <- p - lr wd p; and the chunk's partial of g g^T.  The three rotations and
//           the Gram partial are v_mfma_f32_32x32x2_f32 (k-ordered fp32 fma chains) on 32-column tiles staged through LDS, so both
//           orientations load and store whole contiguous runs.  One launch per short-side class present (R = 32, 64, 96, 128).
//   fold    one workgroup per matrix: GG <- lerp(GG, sum of the chunk partials in chunk order, 1 - shampoo_beta)
//   eigh    first call only: Q = eigenvectors of GG, eigenvalues descending (parallel cyclic Jacobi in LDS, one workgroup per matrix; the
//           rotations in Rutishauser's form x - s (y + tau x): with c rounded to 1 the plain form c x - s y grows every column by t^2 / 2)
//   refresh every precondition_frequency steps: est = diag(Q^T GG Q), stable descending sort, Q <- qr(GG Q[:, idx]).Q (Gram-Schmidt applied
//           twice, a dependent column replaced by an orthonormal completion), then one chunked pass permutes exp_avg_sq by idx
// No atomics, no host sync, no allocation; every reduction has a fixed order, so results are bit-identical run to run.  The bias correction
// is the caller's (a host double folded into step_size).
#include <math.h>
#include "common.h"

enum { SP_N = 0, SP_CHUNKS = 1, SP_WS = 2, SP_QQ = 3, SP_VV = 4, SP_CLS = 5, SP_HDR = 8 };
enum { SR_POFF = 0, SR_R, SR_L, SR_RP, SR_TRANS, SR_CHUNK0, SR_NCHUNK, SR_GP, SR_QOFF, SR_IDX, SR_VOFF, SR_SPARE, SR_STRIDE };
#define SO_CH 512          // long-side columns per workgroup: four 32-column tiles per wave
#define SO_THREADS 256
#define SO_MAX_R 128
#define SO_LDX 33          // row pitch of a 32-column tile in LDS
#define SO_SWEEPS 16       // Jacobi sweeps at most (fp32 converges in 6-9)

static_assert(ST355_SOAP_PLAN_HEADER == SP_HDR && ST355_SOAP_PLAN_RECORD == SR_STRIDE, "st355.h plan constants");

struct SoapC {
  float gs, b1, omb1, b2, omb2, eps, step, lrwd;
};

__device__ __forceinline__ const int64_t* so_rec(const int64_t* plan, int mat) { return plan + SP_HDR + (int64_t)mat * SR_STRIDE; }

// the matrix whose chunk range holds `chunk` (records are in arena order, bases ascending)
__device__ __forceinline__ int so_find(const int64_t* __restrict__ plan, int n, int64_t chunk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (so_rec(plan, mid)[SR_CHUNK0] <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// element e of a wave's 32-column tile (columns kc0 .. kc0 + kn - 1 of the r x L view): its arena index and its place in the LDS tile.
// Wide matrix [r, L]: 32 consecutive lanes take 32 consecutive columns of one row.  Tall matrix [L, r]: the tile is one contiguous run.
struct SoTile {
  int64_t base;            // wide: poff + kc0;  tall: poff + kc0 * r
  int r, L, kn, trans;
};
__device__ __forceinline__ bool so_elem(const SoTile& t, int e, int& xi, int64_t& idx) {
  if (t.trans) {
    if (e >= t.kn * t.r) return false;
    const int kk = e / t.r, i = e - kk * t.r;
    xi = i * SO_LDX + kk;
    idx = t.base + e;
    return true;
  }
  const int i = e >> 5, kk = e & 31;
  if (i >= t.r || kk >= t.kn) return false;
  xi = i * SO_LDX + kk;
  idx = t.base + (int64_t)i * t.L + kk;
  return true;
}

// 32x32x2 operand maps (as in muon.hip): lane l holds A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; C/D: col = l&31,
// row = (v&3) + 8(v>>2) + 4(l>>5).
// acc[ti] = rows 32 ti .. of Q^T X (TRANSPOSED) or Q X over the R x 32 tile X
template <int NT, bool TRANSPOSED>
__device__ __forceinline__ void so_rotate(const float* __restrict__ Qs, const float* __restrict__ X, f32x16* acc) {
  constexpr int R = NT * 32, LDQ = R + 1;
  const int lane = threadIdx.x & (WAVE - 1), c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ti = 0; ti < NT; ti++) acc[ti] = (f32x16){};
  for (int s = 0; s < R / 2; s++) {
    const int k = 2 * s + h;
    const float b = X[k * SO_LDX + c];
#pragma unroll
    for (int ti = 0; ti < NT; ti++) {
      const float a = TRANSPOSED ? Qs[k * LDQ + ti * 32 + c] : Qs[(ti * 32 + c) * LDQ + k];
      acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ti], 0, 0, 0);
    }
  }
}

template <int NT>
__device__ __forceinline__ void so_store_acc(float* __restrict__ X, const f32x16* acc) {
  const int lane = threadIdx.x & (WAVE - 1), c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ti = 0; ti < NT; ti++)
#pragma unroll
    for (int v = 0; v < 16; v++) X[(ti * 32 + (v & 3) + 8 * (v >> 2) + 4 * h) * SO_LDX + c] = acc[ti][v];
}

// upper 32x32 tiles of X X^T over the tile's 32 columns, added to gacc
template <int NT>
__device__ __forceinline__ void so_gram(const float* __restrict__ X, f32x16* gacc) {
  const int lane = threadIdx.x & (WAVE - 1), c = lane & 31, h = lane >> 5;
  for (int s = 0; s < 16; s++) {
    const int col = 2 * s + h;
    float a[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) a[t] = X[(t * 32 + c) * SO_LDX + col];
    int u = 0;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = ti; tj < NT; tj++, u++) gacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti], a[tj], gacc[u], 0, 0, 0);
  }
}

template <int NT>
__device__ __forceinline__ void so_zero_tile(float* X) {
  for (int e = threadIdx.x & (WAVE - 1); e < NT * 32 * SO_LDX; e += WAVE) X[e] = 0.f;
}

// the four waves' Gram tiles summed in wave order, one tile at a time, into the chunk's R x R partial (mirrored: X X^T is symmetric bit for bit)
template <int NT>
__device__ __forceinline__ void so_gram_store(const f32x16* gacc, float* X, const float* Xall, float* __restrict__ out) {
  constexpr int R = NT * 32, NU = NT * (NT + 1) / 2;
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int u = 0; u < NU; u++) {
    int ti = 0, uu = u;
    while (uu >= NT - ti) { uu -= NT - ti; ti++; }
    const int tj = ti + uu;
#pragma unroll
    for (int vv = 0; vv < 16; vv++) X[vv * WAVE + lane] = gacc[u][vv];
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += SO_THREADS) {
      const float s = ((Xall[e] + Xall[R * SO_LDX + e]) + Xall[2 * R * SO_LDX + e]) + Xall[3 * R * SO_LDX + e];
      const int vv = e / WAVE, ln = e & (WAVE - 1);
      const int row = ti * 32 + (vv & 3) + 8 * (vv >> 2) + 4 * (ln >> 5), col = tj * 32 + (ln & 31);
      out[row * R + col] = s;
      if (ti != tj) out[col * R + row] = s;
    }
    __syncthreads();
  }
}

template <int NT>
__global__ void __launch_bounds__(SO_THREADS) k_soap_step(const int64_t* __restrict__ plan, int n, float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, const float* __restrict__ q,
                                                         float* __restrict__ ws, SoapC c, int first) {
  constexpr int R = NT * 32, LDQ = R + 1, NU = NT * (NT + 1) / 2, NIT = 16 * NT;
  constexpr bool FUSE = NT <= 2;                       // the Gram accumulators stay live through the update only where they are few
  extern __shared__ __attribute__((aligned(16))) float so_smem[];
  float* Qs = so_smem;                                 // [R][R + 1], zero beyond r
  float* Xall = so_smem + R * LDQ;                     // four tiles [R][33], one per wave
  const int64_t chunk = blockIdx.x;
  const int mat = so_find(plan, n, chunk);
  const int64_t* rc = so_rec(plan, mat);
  if (rc[SR_RP] != R) return;
  const int r = (int)rc[SR_R], L = (int)rc[SR_L], trans = (int)rc[SR_TRANS];
  const int64_t poff = rc[SR_POFF];
  const int ci = (int)(chunk - rc[SR_CHUNK0]);
  const int k0 = ci * SO_CH;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  float* X = Xall + wave * (R * SO_LDX);
  if (!first) {
    const float* qm = q + rc[SR_QOFF];
    for (int e = threadIdx.x; e < R * R; e += SO_THREADS) {
      const int i = e / R, j = e - i * R;
      Qs[i * LDQ + j] = (i < r && j < r) ? qm[i * r + j] : 0.f;
    }
  }
  float* out = ws + rc[SR_GP] + (int64_t)ci * R * R;          // this chunk's partial of g g^T
  f32x16 gacc[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) gacc[u] = (f32x16){};

  if (first || !FUSE) {                                // Gram pass on its own
    for (int b = 0; b < SO_CH / 128; b++) {
      if (k0 + b * 128 >= L) break;                    // all four waves' tiles lie past the end (the same decision in every thread)
      const int kc0 = k0 + (b * 4 + wave) * 32;
      SoTile t = {trans ? poff + (int64_t)kc0 * r : poff + kc0, r, L, max(0, min(32, L - kc0)), trans};
      so_zero_tile<NT>(X);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; it++) {
        int xi; int64_t idx;
        if (so_elem(t, it * WAVE + lane, xi, idx)) X[xi] = g[idx] * c.gs;
      }
      __syncthreads();
      if (t.kn > 0) so_gram<NT>(X, gacc);
      __syncthreads();
    }
    so_gram_store<NT>(gacc, X, Xall, out);
  }
  if (!first) {
    for (int b = 0; b < SO_CH / 128; b++) {
      if (k0 + b * 128 >= L) break;                    // all four waves' tiles lie past the end (the same decision in every thread)
      const int kc0 = k0 + (b * 4 + wave) * 32;
      SoTile t = {trans ? poff + (int64_t)kc0 * r : poff + kc0, r, L, max(0, min(32, L - kc0)), trans};
      f32x16 acc[NT];
      so_zero_tile<NT>(X);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; it++) {               // g <- s g; m <- b1 m + (1 - b1) g
        int xi; int64_t idx;
        if (so_elem(t, it * WAVE + lane, xi, idx)) {
          const float gv = g[idx] * c.gs;
          const float mn = fmaf(c.omb1, gv, c.b1 * m[idx]);
          m[idx] = mn;
          X[xi] = gv;
        }
      }
      __syncthreads();
      if (FUSE && t.kn > 0) so_gram<NT>(X, gacc);
      so_rotate<NT, true>(Qs, X, acc);                 // gp = Q^T g
      __syncthreads();
      so_store_acc<NT>(X, acc);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; it++) {               // v <- b2 v + (1 - b2) gp^2; the tile becomes m
        int xi; int64_t idx;
        if (so_elem(t, it * WAVE + lane, xi, idx)) {
          const float gp = X[xi];
          const float vn = fmaf(c.omb2, gp * gp, c.b2 * v[idx]);
          v[idx] = vn;
          X[xi] = m[idx];                              // this thread's own store of a moment ago
        }
      }
      __syncthreads();
      so_rotate<NT, true>(Qs, X, acc);                 // mp = Q^T m
      __syncthreads();
      so_store_acc<NT>(X, acc);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; it++) {               // w = mp / (sqrt(v) + eps)
        int xi; int64_t idx;
        if (so_elem(t, it * WAVE + lane, xi, idx)) X[xi] = X[xi] / (sqrtf(v[idx]) + c.eps);
      }
      __syncthreads();
      so_rotate<NT, false>(Qs, X, acc);                // u = Q w
      __syncthreads();
      so_store_acc<NT>(X, acc);
      __syncthreads();
#pragma unroll 4
      for (int it = 0; it < NIT; it++) {               // p <- p - step_size u; p <- p - lr wd p
        int xi; int64_t idx;
        if (so_elem(t, it * WAVE + lane, xi, idx)) {
          float pv = fmaf(-c.step, X[xi], p[idx]);
          if (c.lrwd > 0.f) pv = fmaf(-c.lrwd, pv, pv);
          p[idx] = pv;
        }
      }
      __syncthreads();
    }
  }
  if (!first && FUSE) so_gram_store<NT>(gacc, X, Xall, out);
}

// ---- fold: GG <- lerp(GG, sum of partials, w) with torch's lerp (w < 0.5: a + w (b - a), else b - (b - a)(1 - w)) ----------------------
__global__ void __launch_bounds__(SO_THREADS) k_soap_fold(const int64_t* __restrict__ plan, const float* __restrict__ ws, float* __restrict__ gg, float w) {
  const int64_t* rc = so_rec(plan, blockIdx.x);
  const int r = (int)rc[SR_R], R = (int)rc[SR_RP], nch = (int)rc[SR_NCHUNK];
  const float* gp = ws + rc[SR_GP];
  float* G = gg + rc[SR_QOFF];
  for (int e = threadIdx.x; e < r * r; e += SO_THREADS) {
    const int i = e / r, j = e - i * r;
    float s = 0.f;
    for (int qd = 0; qd < nch; qd++) s += gp[(int64_t)qd * R * R + i * R + j];
    const float a = G[e], d = s - a;
    G[e] = w < 0.5f ? fmaf(w, d, a) : s - d * (1.f - w);
  }
}

// rank of entry j in a stable descending sort of val[0 .. r)
__device__ __forceinline__ int so_rank_desc(const float* val, int r, int j) {
  const float x = val[j];
  int rank = 0;
  for (int k = 0; k < r; k++) rank += (val[k] > x || (val[k] == x && k < j)) ? 1 : 0;
  return rank;
}

// ---- eigh: parallel cyclic Jacobi, round-robin pairs, one workgroup per matrix ------------------------------------------------------------
__global__ void __launch_bounds__(SO_THREADS) k_soap_eigh(const int64_t* __restrict__ plan, const float* __restrict__ gg, float* __restrict__ q,
                                                         float* __restrict__ evals) {
  extern __shared__ __attribute__((aligned(16))) float so_smem[];
  const int64_t* rc = so_rec(plan, blockIdx.x);
  const int r = (int)rc[SR_R], ld = r | 1;
  float* A = so_smem;                 // [r][ld]
  float* V = A + SO_MAX_R * (SO_MAX_R + 1);
  float* cs = V + SO_MAX_R * (SO_MAX_R + 1);   // [64][4]: tau = s / (1 + c), s, a_pp', a_qq'
  float* lam = cs + 256;              // [128]
  float* red = lam + SO_MAX_R;        // [8]
  const int tid = threadIdx.x;
  const float* G = gg + rc[SR_QOFF];
  float mx = 0.f;
  for (int e = tid; e < r * r; e += SO_THREADS) {
    const int i = e / r, j = e - i * r;
    const float a = G[e];
    A[i * ld + j] = a;
    V[i * ld + j] = i == j ? 1.f : 0.f;
    mx = fmaxf(mx, fabsf(a));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = mx;
  __syncthreads();
  const float tiny = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * 9.3132257e-10f;   // 2^-30 of the largest entry
  const int mm = r + (r & 1), np = mm / 2;
  for (int sweep = 0; sweep < SO_SWEEPS; sweep++) {
    __syncthreads();
    if (tid == 0) red[4] = 0.f;
    __syncthreads();
    for (int rd = 0; rd < mm - 1; rd++) {
      if (tid < np) {
        int a = tid == 0 ? mm - 1 : (rd + tid) % (mm - 1);
        int b = tid == 0 ? rd : (rd - tid + (mm - 1)) % (mm - 1);
        const int pp = min(a, b), qq = max(a, b);
        float tau = 0.f, sv = 0.f, app = 0.f, aqq = 0.f;
        if (qq < r) {
          app = A[pp * ld + pp]; aqq = A[qq * ld + qq];
          const float apq = A[pp * ld + qq];
          const float mag = fabsf(apq);
          if (mag > tiny && mag > 1.4901161e-8f * sqrtf(fabsf(app) * fabsf(aqq))) {
            const float theta = (aqq - app) / (2.f * apq);
            const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.f)));
            // c in double: sqrtf is v_sqrt_f32 (1 ulp, not correctly rounded), and a bias in c grows every column norm rotation by rotation
            const double cd = 1.0 / sqrt(fma((double)t, (double)t, 1.0)), sd = (double)t * cd;
            sv = (float)sd;
            tau = (float)(sd / (1.0 + cd));
            app = fmaf(-t, apq, app);
            aqq = fmaf(t, apq, aqq);
            if (sv != 0.f) red[4] = 1.f;
          }
        }
        cs[4 * tid] = tau; cs[4 * tid + 1] = sv; cs[4 * tid + 2] = app; cs[4 * tid + 3] = aqq;
      }
      __syncthreads();
      for (int e = tid; e < np * r; e += SO_THREADS) {           // columns p, q of A and V
        const int k = e / r, i = e - k * r;
        const float sv = cs[4 * k + 1];
        if (sv == 0.f) continue;
        const float tau = cs[4 * k];
        int a = k == 0 ? mm - 1 : (rd + k) % (mm - 1);
        int b = k == 0 ? rd : (rd - k + (mm - 1)) % (mm - 1);
        const int pp = min(a, b), qq = max(a, b);
        const float ap = A[i * ld + pp], aq = A[i * ld + qq];
        A[i * ld + pp] = ap - sv * (aq + tau * ap);
        A[i * ld + qq] = aq + sv * (ap - tau * aq);
        const float vp = V[i * ld + pp], vq = V[i * ld + qq];
        V[i * ld + pp] = vp - sv * (vq + tau * vp);
        V[i * ld + qq] = vq + sv * (vp - tau * vq);
      }
      __syncthreads();
      for (int e = tid; e < np * r; e += SO_THREADS) {           // rows p, q of A; the 2 x 2 block gets its closed form
        const int k = e / r, j = e - k * r;
        const float sv = cs[4 * k + 1];
        if (sv == 0.f) continue;
        const float tau = cs[4 * k];
        int a = k == 0 ? mm - 1 : (rd + k) % (mm - 1);
        int b = k == 0 ? rd : (rd - k + (mm - 1)) % (mm - 1);
        const int pp = min(a, b), qq = max(a, b);
        const float ap = A[pp * ld + j], aq = A[qq * ld + j];
        float np_ = ap - sv * (aq + tau * ap), nq_ = aq + sv * (ap - tau * aq);
        if (j == pp) { np_ = cs[4 * k + 2]; nq_ = 0.f; }
        if (j == qq) { np_ = 0.f; nq_ = cs[4 * k + 3]; }
        A[pp * ld + j] = np_;
        A[qq * ld + j] = nq_;
      }
      __syncthreads();
    }
    if (red[4] == 0.f) break;
  }
  __syncthreads();
  if (tid < r) lam[tid] = A[tid * ld + tid];
  __syncthreads();
  float* Qo = q + rc[SR_QOFF];
  for (int j = tid; j < r; j += SO_THREADS) {
    const int rank = so_rank_desc(lam, r, j);
    cs[j] = (float)rank;                                         // cs is free now: r <= 128 < 256
    if (evals) evals[rc[SR_VOFF] + rank] = lam[j];
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += SO_THREADS) {
    const int i = e / r, j = e - i * r;
    Qo[i * r + (int)cs[j]] = V[i * ld + j];
  }
}

// ---- refresh: sort by the estimated eigenvalues, one power iteration, QR ------------------------------------------------------------------
// column j of B made orthogonal to columns 0 .. j-1 (Gram-Schmidt, applied twice); returns its norm afterwards (the same value in every thread)
__device__ __forceinline__ float so_cgs2(float* B, int ld, int r, int j, float* coef, float* red) {
  const int tid = threadIdx.x;
  for (int pass = 0; pass < 2; pass++) {
    __syncthreads();
    if (tid < j) {
      float s = 0.f;
      for (int i = 0; i < r; i++) s = fmaf(B[i * ld + tid], B[i * ld + j], s);
      coef[tid] = s;
    }
    __syncthreads();
    if (tid < r) {
      float s = 0.f;
      for (int k = 0; k < j; k++) s = fmaf(coef[k], B[tid * ld + k], s);
      B[tid * ld + j] -= s;
    }
  }
  __syncthreads();
  if (tid < WAVE) {
    float s = 0.f;
    for (int i = tid; i < r; i += WAVE) s = fmaf(B[i * ld + j], B[i * ld + j], s);
    s = wave_sum(s);
    if (tid == 0) red[0] = sqrtf(s);
  }
  __syncthreads();
  return red[0];
}

__global__ void __launch_bounds__(SO_THREADS) k_soap_refresh(const int64_t* __restrict__ plan, const float* __restrict__ gg, float* __restrict__ q,
                                                            float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float so_smem[];
  const int64_t* rc = so_rec(plan, blockIdx.x);
  const int r = (int)rc[SR_R], ld = r | 1;
  float* B = so_smem;                 // Q, then the permuted GG Q, then the new Q
  float* T = B + SO_MAX_R * (SO_MAX_R + 1);
  float* est = T + SO_MAX_R * (SO_MAX_R + 1);   // [128]
  float* coef = est + SO_MAX_R;       // [128]
  int* sidx = (int*)(coef + SO_MAX_R);   // [128]
  float* red = (float*)(sidx + SO_MAX_R);  // [8]
  const int tid = threadIdx.x;
  const float* G = gg + rc[SR_QOFF];
  float* Qm = q + rc[SR_QOFF];
  for (int e = tid; e < r * r; e += SO_THREADS) B[(e / r) * ld + e % r] = Qm[e];
  __syncthreads();
  for (int e = tid; e < r * r; e += SO_THREADS) {                // T = GG Q
    const int i = e / r, j = e - i * r;
    float s = 0.f;
    for (int k = 0; k < r; k++) s = fmaf(G[i * r + k], B[k * ld + j], s);
    T[i * ld + j] = s;
  }
  __syncthreads();
  if (tid < r) {                                                 // est = diag(Q^T GG Q)
    float s = 0.f;
    for (int i = 0; i < r; i++) s = fmaf(B[i * ld + tid], T[i * ld + tid], s);
    est[tid] = s;
  }
  __syncthreads();
  int* idx_out = (int*)(ws + rc[SR_IDX]);
  if (tid < r) {
    const int rank = so_rank_desc(est, r, tid);
    sidx[rank] = tid;
    idx_out[rank] = tid;
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += SO_THREADS) {                // B = (GG Q)[:, idx]
    const int i = e / r, j = e - i * r;
    B[i * ld + j] = T[i * ld + sidx[j]];
  }
  __syncthreads();
  for (int j = 0; j < r; j++) {
    if (tid < WAVE) {                                            // the column's norm before it is orthogonalised
      float s = 0.f;
      for (int i = tid; i < r; i += WAVE) s = fmaf(B[i * ld + j], B[i * ld + j], s);
      s = wave_sum(s);
      if (tid == 0) red[1] = sqrtf(s);
    }
    float nrm = so_cgs2(B, ld, r, j, coef, red);
    const float nrm0 = red[1];
    // Rank test.  Each of the j <= r coefficients of a pass is an r-term fp32 dot product with error up to r u |q| |a| (u = 2^-24), so the
    // remainder of a column that lies in the span of its predecessors comes out with a norm of the order r u nrm0: pure rounding, its
    // direction means nothing.  A remainder of at most 2 r u nrm0 cannot be told from that and gets the completion (rank deficient to working
    // precision); above it the second pass removes what the first left inside the span, and the column is kept.  r = 128: 1.5e-5 nrm0.
    if (!(nrm > 2.f * (float)r * 5.9604645e-8f * nrm0) || !(nrm0 < INFINITY)) {
      // zero or dependent column: the unit vector furthest from span(q_0 .. q_{j-1}), orthogonalised — its remainder has
      // norm^2 >= (r - j) / r, so the division below is safe
      __syncthreads();
      if (tid < r) {
        float s = 1.f;
        for (int k = 0; k < j; k++) s = fmaf(-B[tid * ld + k], B[tid * ld + k], s);
        coef[tid] = s;
      }
      __syncthreads();
      if (tid == 0) {
        int best = 0;
        for (int i = 1; i < r; i++) if (coef[i] > coef[best]) best = i;
        red[2] = (float)best;
      }
      __syncthreads();
      const int best = (int)red[2];
      if (tid < r) B[tid * ld + j] = tid == best ? 1.f : 0.f;
      nrm = so_cgs2(B, ld, r, j, coef, red);
    }
    if (tid < r) B[tid * ld + j] = B[tid * ld + j] / nrm;
    __syncthreads();
  }
  for (int e = tid; e < r * r; e += SO_THREADS) Qm[e] = B[(e / r) * ld + e % r];
}

// ---- exp_avg_sq permuted along the short side by the refresh's index: each thread owns whole columns, so the pass is in place ---------------
template <int NT>
__global__ void __launch_bounds__(SO_THREADS) k_soap_permute(const int64_t* __restrict__ plan, int n, float* __restrict__ v, const float* __restrict__ ws) {
  constexpr int R = NT * 32;
  __shared__ int sidx[R];
  const int64_t chunk = blockIdx.x;
  const int mat = so_find(plan, n, chunk);
  const int64_t* rc = so_rec(plan, mat);
  if (rc[SR_RP] != R) return;
  const int r = (int)rc[SR_R], L = (int)rc[SR_L], trans = (int)rc[SR_TRANS];
  const int64_t poff = rc[SR_POFF];
  const int* idx = (const int*)(ws + rc[SR_IDX]);
  for (int i = threadIdx.x; i < R; i += SO_THREADS) sidx[i] = i < r ? idx[i] : 0;
  __syncthreads();
  const int k0 = (int)(chunk - rc[SR_CHUNK0]) * SO_CH;
  const int ke = min(k0 + SO_CH, L);
  for (int col = k0 + threadIdx.x; col < ke; col += SO_THREADS) {
    const int64_t base = trans ? poff + (int64_t)col * r : poff + col;
    const int64_t stride = trans ? 1 : L;
    float tmp[R];
#pragma unroll
    for (int i = 0; i < R; i++) tmp[i] = i < r ? v[base + (int64_t)sidx[i] * stride] : 0.f;
#pragma unroll
    for (int i = 0; i < R; i++)
      if (i < r) v[base + (int64_t)i * stride] = tmp[i];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int st355_soap_plan(const int64_t* offsets, const int32_t* rows, const int32_t* cols, int n, int64_t* plan, int64_t* ws_floats) {
  ST_REQUIRE(offsets && rows && cols && plan && ws_floats && n > 0, "soap_plan: bad args");
  int64_t ws = 0, chunks = 0, qq = 0, vv = 0, cls = 0;
  for (int i = 0; i < n; i++) {
    ST_REQUIRE(rows[i] > 0 && cols[i] > 0 && offsets[i] >= 0, "soap_plan: matrix %d has shape [%d, %d] at offset %lld", i, rows[i], cols[i],
               (long long)offsets[i]);
    ST_REQUIRE(i == 0 || offsets[i] >= offsets[i - 1] + (int64_t)rows[i - 1] * cols[i - 1], "soap_plan: matrix %d overlaps its predecessor", i);
    const int r = rows[i] < cols[i] ? rows[i] : cols[i], L = rows[i] < cols[i] ? cols[i] : rows[i];
    ST_REQUIRE(r <= SO_MAX_R, "soap_plan: matrix %d has short side %d (the kernel takes at most %d)", i, r, SO_MAX_R);
    ST_REQUIRE((int64_t)r * L < (1ll << 31), "soap_plan: matrix %d has 2^31 elements or more", i);
    const int R = (r + 31) / 32 * 32;
    const int64_t nchunk = (L + SO_CH - 1) / SO_CH;
    int64_t* rc = plan + SP_HDR + (int64_t)i * SR_STRIDE;
    rc[SR_POFF] = offsets[i]; rc[SR_R] = r; rc[SR_L] = L; rc[SR_RP] = R; rc[SR_TRANS] = rows[i] > cols[i];
    rc[SR_CHUNK0] = chunks; rc[SR_NCHUNK] = nchunk; chunks += nchunk;
    rc[SR_GP] = ws; ws += nchunk * R * R;
    rc[SR_IDX] = ws; ws += SO_MAX_R;
    rc[SR_QOFF] = qq; qq += (int64_t)r * r;
    rc[SR_VOFF] = vv; vv += r;
    rc[SR_SPARE] = 0;
    cls |= 1 << (R / 32 - 1);
  }
  ST_REQUIRE(chunks < (1ll << 31), "soap_plan: too many chunks");
  for (int k = 0; k < SP_HDR; k++) plan[k] = 0;
  plan[SP_N] = n; plan[SP_CHUNKS] = chunks; plan[SP_WS] = ws; plan[SP_QQ] = qq; plan[SP_VV] = vv; plan[SP_CLS] = cls;
  *ws_floats = ws;
  return ST355_OK;
}

static int soap_check_plan(const int64_t* plan_host, const char* what) {
  ST_REQUIRE(plan_host[SP_N] > 0 && plan_host[SP_N] < (1ll << 31) && plan_host[SP_CHUNKS] > 0 && plan_host[SP_CHUNKS] < (1ll << 31) &&
                 plan_host[SP_CLS] > 0 && plan_host[SP_CLS] < 16, "%s: corrupt plan", what);
  return ST355_OK;
}

#define SO_EIGH_LDS ((2 * SO_MAX_R * (SO_MAX_R + 1) + 256 + SO_MAX_R + 8) * 4)
#define SO_REFRESH_LDS ((2 * SO_MAX_R * (SO_MAX_R + 1) + 3 * SO_MAX_R + 8) * 4)

template <int NT>
static void soap_launch_step(hipStream_t s, unsigned chunks, const int64_t* plan_dev, int n, float* p, const float* g, float* m, float* v,
                             const float* q, float* ws, const SoapC& c, int first) {
  constexpr int R = NT * 32, LDS = (R * (R + 1) + 4 * R * SO_LDX) * 4;
  static St355AttrOnce attr_set;
  if (attr_set.need()) { hipFuncSetAttribute((const void*)k_soap_step<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); }
  hipLaunchKernelGGL(k_soap_step<NT>, dim3(chunks), dim3(SO_THREADS), LDS, s, plan_dev, n, p, g, m, v, q, ws, c, first);
}

static void soap_launch_eigh(hipStream_t s, int n, const int64_t* plan_dev, const float* gg, float* q, float* evals) {
  static St355AttrOnce attr_set;
  if (attr_set.need()) { hipFuncSetAttribute((const void*)k_soap_eigh, hipFuncAttributeMaxDynamicSharedMemorySize, SO_EIGH_LDS); }
  hipLaunchKernelGGL(k_soap_eigh, dim3((unsigned)n), dim3(SO_THREADS), SO_EIGH_LDS, s, plan_dev, gg, q, evals);
}

extern "C" int st355_soap_step(void* stream, const int64_t* plan_host, const int64_t* plan_dev, float* p, const float* g, float* m, float* v,
                               float* gg, float* q, float* ws, int64_t ws_floats, float grad_scale, double beta1, double beta2, double eps,
                               double step_size, double lr_weight_decay, double gg_weight, int first, int refresh) {
  ST_REQUIRE(plan_host && plan_dev && p && g && m && v && gg && q && ws, "soap_step: bad args");
  if (soap_check_plan(plan_host, "soap_step") != ST355_OK) return ST355_EINVAL;
  ST_REQUIRE(ws_floats >= plan_host[SP_WS], "soap_step: workspace of %lld floats, the plan needs %lld", (long long)ws_floats,
             (long long)plan_host[SP_WS]);
  ST_REQUIRE(gg_weight >= 0.0 && gg_weight <= 1.0, "soap_step: 1 - shampoo_beta must lie in [0, 1]");
  const int n = (int)plan_host[SP_N];
  const unsigned chunks = (unsigned)plan_host[SP_CHUNKS];
  const int cls = (int)plan_host[SP_CLS];
  double flops = 0, elems = 0;
  for (int i = 0; i < n; i++) {
    const int64_t* rc = plan_host + SP_HDR + (int64_t)i * SR_STRIDE;
    flops += (first ? 2.0 : 8.0) * rc[SR_RP] * rc[SR_RP] * rc[SR_L];
    elems += (double)rc[SR_R] * rc[SR_L];
  }
  ProfScope ps(stream, ST355_K_OPTIM, flops, (first ? 4.0 : 28.0) * elems);
  hipStream_t s = (hipStream_t)stream;
  const SoapC c = {grad_scale, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)step_size,
                   (float)lr_weight_decay};
  if (cls & 1) soap_launch_step<1>(s, chunks, plan_dev, n, p, g, m, v, q, ws, c, first);
  if (cls & 2) soap_launch_step<2>(s, chunks, plan_dev, n, p, g, m, v, q, ws, c, first);
  if (cls & 4) soap_launch_step<3>(s, chunks, plan_dev, n, p, g, m, v, q, ws, c, first);
  if (cls & 8) soap_launch_step<4>(s, chunks, plan_dev, n, p, g, m, v, q, ws, c, first);
  hipLaunchKernelGGL(k_soap_fold, dim3((unsigned)n), dim3(SO_THREADS), 0, s, plan_dev, ws, gg, (float)gg_weight);
  if (first) {
    soap_launch_eigh(s, n, plan_dev, gg, q, nullptr);
  } else if (refresh) {
    static St355AttrOnce attr_set;
    if (attr_set.need()) { hipFuncSetAttribute((const void*)k_soap_refresh, hipFuncAttributeMaxDynamicSharedMemorySize, SO_REFRESH_LDS); }
    hipLaunchKernelGGL(k_soap_refresh, dim3((unsigned)n), dim3(SO_THREADS), SO_REFRESH_LDS, s, plan_dev, gg, q, ws);
    if (cls & 1) hipLaunchKernelGGL(k_soap_permute<1>, dim3(chunks), dim3(SO_THREADS), 0, s, plan_dev, n, v, ws);
    if (cls & 2) hipLaunchKernelGGL(k_soap_permute<2>, dim3(chunks), dim3(SO_THREADS), 0, s, plan_dev, n, v, ws);
    if (cls & 4) hipLaunchKernelGGL(k_soap_permute<3>, dim3(chunks), dim3(SO_THREADS), 0, s, plan_dev, n, v, ws);
    if (cls & 8) hipLaunchKernelGGL(k_soap_permute<4>, dim3(chunks), dim3(SO_THREADS), 0, s, plan_dev, n, v, ws);
  }
  return st355_check_launch("soap_step");
}

extern "C" int st355_soap_eigh(void* stream, const int64_t* plan_host, const int64_t* plan_dev, const float* gg, float* q, float* evals) {
  ST_REQUIRE(plan_host && plan_dev && gg && q, "soap_eigh: bad args");
  if (soap_check_plan(plan_host, "soap_eigh") != ST355_OK) return ST355_EINVAL;
  soap_launch_eigh((hipStream_t)stream, (int)plan_host[SP_N], plan_dev, gg, q, evals);
  return st355_check_launch("soap_eigh");
}

// muon.hip — Muon (MuonClip, optimizers/muon/__init__.py) over the fp32 LoRA adapter arena: momentum, Newton-Schulz
// orthogonalisation of every 2-D adapter matrix, scale, decoupled decay and apply, as a fixed number of launches per step
// whatever the number of matrices.
//
// Every matrix is worked on as X = m (r x L, r <= L) or X = m^T (tall m), r <= 128.  X lives in the workspace as W [L][R]
// (R = r rounded up to 32, padding rows zero): the long side is the row index, so the MFMA operand loads of both products are
// coalesced.  One Newton-Schulz iteration is three launches over ALL matrices:
//   gram   one workgroup per 512-column chunk: the upper 32x32 tiles of X X^T over the chunk (v_mfma_f32_32x32x2_f32, k-ordered fp32
//          fma chains), the four waves' tiles summed in a fixed order, one partial per chunk
//   poly   one workgroup per matrix: A = sum of the chunk partials in chunk order, B = b A + c A A (fixed k order, VALU)
//   update one workgroup per chunk: X <- a X + B X in place (each column of X only feeds its own column); on the last iteration
//          the result goes straight into the parameter: O = X (or X^T) * sqrt(max(rows, cols)) * rms_scale_factor,
//          p <- p + (-lr wd) p, p <- p + (-lr) O.
// plus one momentum / Frobenius-partial pass before and one norm launch: 2 + 3 * ns_steps launches per short-side class present (R = 32,
// 64, 96, 128; the r32 LoRA arenas have one), whatever the number of matrices.  No atomics, no host sync, no allocation: results are
// bit-identical run to run, and the step can be captured into a graph.
#include <math.h>
#include "common.h"

// plan layout (int64): header, then one record per matrix
enum { MP_N = 0, MP_TILES = 1, MP_CHUNKS = 2, MP_WS = 3, MP_HDR = 8 };
enum { MR_POFF = 0, MR_ROWS, MR_COLS, MR_R, MR_L, MR_RP, MR_TRANS, MR_W, MR_B, MR_GP, MR_TILE0, MR_NTILE, MR_CHUNK0, MR_NCHUNK, MR_SS,
       MR_NRM, MR_STRIDE };
#define MU_TC 64          // prep tile: long-side columns per workgroup
#define MU_CH 512         // gram / update chunk: long-side columns per workgroup (128 per wave)
#define MU_THREADS 256
#define MU_MAX_R 128

static_assert(ST355_MUON_PLAN_HEADER == MP_HDR && ST355_MUON_PLAN_RECORD == MR_STRIDE, "st355.h plan constants");

__device__ __forceinline__ const int64_t* mu_rec(const int64_t* plan, int mat) { return plan + MP_HDR + (int64_t)mat * MR_STRIDE; }

// the matrix whose [field] range holds `item` (records are in arena order, bases ascending)
__device__ __forceinline__ int mu_find(const int64_t* __restrict__ plan, int n, int64_t item, int field) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mu_rec(plan, mid)[field] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- pass 1: momentum (or a plain copy) into W, Frobenius partial per 64-column tile -------------------------------------------
// mode 0: m <- m + (1-mu)(s g - m), X = m;   mode 1: X = src (bare orthogonalisation)
__global__ void __launch_bounds__(MU_THREADS) k_muon_prep(const int64_t* __restrict__ plan, int n, const float* __restrict__ src,
                                                         float* __restrict__ mom, float* __restrict__ ws, float omm, float gscale, int mode) {
  __shared__ float T[MU_TC * (MU_MAX_R + 1)];
  __shared__ float red[MU_THREADS / WAVE];
  const int64_t tile = blockIdx.x;
  const int mat = mu_find(plan, n, tile, MR_TILE0);
  const int64_t* rc = mu_rec(plan, mat);
  const int64_t poff = rc[MR_POFF];
  const int r = (int)rc[MR_R], L = (int)rc[MR_L], R = (int)rc[MR_RP], trans = (int)rc[MR_TRANS];
  const int t = (int)(tile - rc[MR_TILE0]);
  const int k0 = t * MU_TC;
  const int kn = min(MU_TC, L - k0);
  const int ld = R + 1;
  float ss = 0.f;
  for (int e = threadIdx.x; e < kn * r; e += MU_THREADS) {
    int kk, i;
    int64_t idx;
    if (trans) { kk = e / r; i = e - kk * r; idx = poff + (int64_t)(k0 + kk) * r + i; }   // m is [L, r]: the tile is one contiguous run
    else { i = e / kn; kk = e - i * kn; idx = poff + (int64_t)i * L + k0 + kk; }          // m is [r, L]: kn contiguous columns per row
    float v;
    if (mode == 0) {
      const float gv = src[idx] * gscale;
      const float mv = mom[idx];
      v = mv + omm * (gv - mv);                  // lerp_(grad, 1 - momentum)
      mom[idx] = v;
    } else {
      v = src[idx];
    }
    ss = fmaf(v, v, ss);
    T[kk * ld + i] = v;
  }
  const int pad = R - r;
  for (int e = threadIdx.x; e < kn * pad; e += MU_THREADS) T[(e / pad) * ld + r + e % pad] = 0.f;
  ss = wave_sum(ss);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = ss;
  __syncthreads();
  float* W = ws + rc[MR_W] + (int64_t)k0 * R;                  // rows k0 .. k0 + kn - 1 of W: one contiguous run
  for (int e = threadIdx.x; e < kn * R; e += MU_THREADS) W[e] = T[(e / R) * ld + (e % R)];
  if (threadIdx.x == 0) ws[rc[MR_SS] + t] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- ||X||_F clamped at eps, per matrix (tile partials summed lane-strided, then a fixed lane tree) --------------------------
__global__ void __launch_bounds__(WAVE) k_muon_norm(const int64_t* __restrict__ plan, float* __restrict__ ws, float eps) {
  const int64_t* rc = mu_rec(plan, blockIdx.x);
  const float* part = ws + rc[MR_SS];
  const int nt = (int)rc[MR_NTILE];
  float s = 0.f;
  for (int i = threadIdx.x; i < nt; i += WAVE) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) ws[rc[MR_NRM]] = fmaxf(sqrtf(s), eps);
}

// ---- gram: upper tiles of X X^T over one 512-column chunk ----------------------------------------------------------------------
// 32x32x2 operand maps: lane l holds A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31].  With k = a column of X (lane half h takes
// column k0 + 2s + h), A = X[ti rows] and B = X^T[tj cols] are the same load: lane l reads W[k][32 t + (l&31)].
template <int NT>
__device__ __forceinline__ void mu_gram(const float* __restrict__ W, int L, int k0, const float* nrm, float* __restrict__ out, float* lds) {
  constexpr int R = NT * 32, NU = NT * (NT + 1) / 2;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int c = lane & 31, h = lane >> 5;
  f32x16 acc[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) acc[u] = (f32x16){};
  const float dn = nrm ? *nrm : 1.f;
  const int kb = k0 + wave * (MU_CH / 4);
  const int ke = min(kb + MU_CH / 4, L);
  for (int k = kb; k < ke; k += 8) {               // four k-steps per trip: their loads are issued before the first MFMA
    float x[4][NT];
#pragma unroll
    for (int st = 0; st < 4; st++) {
      const int kc = k + 2 * st + h;
#pragma unroll
      for (int q = 0; q < NT; q++) {
        x[st][q] = kc < ke ? W[(int64_t)kc * R + q * 32 + c] : 0.f;
        if (nrm) x[st][q] = x[st][q] / dn;
      }
    }
#pragma unroll
    for (int st = 0; st < 4; st++) {
      int u = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = ti; tj < NT; tj++, u++) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[st][ti], x[st][tj], acc[u], 0, 0, 0);
    }
  }
  // the four waves' tiles summed in wave order, one tile at a time (16 KB of LDS); C/D map: col = l&31, row = (v&3) + 8(v>>2) + 4(l>>5)
#pragma unroll
  for (int u = 0; u < NU; u++) {
#pragma unroll
    for (int v = 0; v < 16; v++) lds[wave * 1024 + v * WAVE + lane] = acc[u][v];
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += MU_THREADS) {
      const float s = ((lds[e] + lds[1024 + e]) + lds[2048 + e]) + lds[3072 + e];
      const int v = e / WAVE, ln = e & (WAVE - 1);
      out[u * 1024 + ((v & 3) + 8 * (v >> 2) + 4 * (ln >> 5)) * 32 + (ln & 31)] = s;
    }
    __syncthreads();
  }
}

// one launch per short-side class present (R = 32, 64, 96, 128): its accumulators are sized for that class, so the R = 32 launch of
// the LoRA r32 arenas keeps its occupancy; a workgroup whose chunk belongs to another class returns at once
template <int NT>
__global__ void __launch_bounds__(MU_THREADS) k_muon_gram(const int64_t* __restrict__ plan, int n, float* __restrict__ ws, int first) {
  __shared__ float lds[4 * 1024];
  const int64_t chunk = blockIdx.x;
  const int mat = mu_find(plan, n, chunk, MR_CHUNK0);
  const int64_t* rc = mu_rec(plan, mat);
  if (rc[MR_RP] != NT * 32) return;
  constexpr int NU = NT * (NT + 1) / 2;
  const int ci = (int)(chunk - rc[MR_CHUNK0]);
  mu_gram<NT>(ws + rc[MR_W], (int)rc[MR_L], ci * MU_CH, first ? ws + rc[MR_NRM] : nullptr, ws + rc[MR_GP] + (int64_t)ci * NU * 1024, lds);
}

// ---- poly: A = sum of chunk partials (chunk order), B = b A + c A A ---------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(MU_THREADS) k_muon_poly(const int64_t* __restrict__ plan, float* __restrict__ ws, float b, float c) {
  constexpr int R = NT * 32, NU = NT * (NT + 1) / 2;
  __shared__ float A[R * R];
  const int64_t* rc = mu_rec(plan, blockIdx.x);
  if (rc[MR_RP] != R) return;
  const int nch = (int)rc[MR_NCHUNK];
  const float* gp = ws + rc[MR_GP];
  for (int e = threadIdx.x; e < NU * 1024; e += MU_THREADS) {
    float s = 0.f;
    for (int q = 0; q < nch; q++) s += gp[(int64_t)q * NU * 1024 + e];
    int u = e >> 10, ti = 0;
    while (u >= NT - ti) { u -= NT - ti; ti++; }       // upper tiles in (ti, tj >= ti) order
    const int tj = ti + u, row = ti * 32 + ((e >> 5) & 31), col = tj * 32 + (e & 31);
    A[row * R + col] = s;
    A[col * R + row] = s;                              // the mirror (exact: X X^T is symmetric bit for bit)
  }
  __syncthreads();
  float* Bm = ws + rc[MR_B];
  for (int e = threadIdx.x; e < R * R; e += MU_THREADS) {
    const int i = e / R, j = e - i * R;
    float s = 0.f;
    for (int k = 0; k < R; k++) s = fmaf(A[k * R + i], A[k * R + j], s);   // A symmetric: A[i][k] = A[k][i]
    Bm[e] = fmaf(c, s, b * A[e]);
  }
}

// ---- update: X <- a X + B X over one chunk; the last iteration writes the parameter (mode 0) or the output (mode 1) ----------
// B X as 32x32x2 MFMAs with the reduction index permuted: step s of lane half h is k = h R/2 + s, so a lane's B-operand values
// (X[k][its column]) are R/2 contiguous floats of its row of W and its A-operand values (B[row][k]) R/2 contiguous floats of B.
struct MuFin {
  float* p;            // parameter arena (mode 0) or output (mode 1); NULL: not the last iteration, X goes back into W
  int mode;
  float lrwd, lr;      // -lr * weight_decay, -lr
  double rms;
};

template <int NT>
__device__ __forceinline__ void mu_update(float* W, const float* __restrict__ Bm, const int64_t* rc, int k0, const float* nrm, float a,
                                          const MuFin& f) {
  constexpr int R = NT * 32, H = R / 2;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int c = lane & 31, h = lane >> 5;
  const int L = (int)rc[MR_L], r = (int)rc[MR_R], trans = (int)rc[MR_TRANS];
  const int64_t poff = rc[MR_POFF];
  const float dn = nrm ? *nrm : 1.f;
  const float sf = f.mode == 0 ? (float)(sqrt((double)L) * f.rms) : 1.f;
  for (int blk = wave; blk < MU_CH / 32; blk += MU_THREADS / WAVE) {
    const int kc0 = k0 + blk * 32;
    if (kc0 >= L) break;
    const int kc = kc0 + c;
    const bool ok = kc < L;
    float* wcol = W + (int64_t)(ok ? kc : 0) * R;
    float x[H];
#pragma unroll
    for (int q = 0; q < H / 4; q++) {
      f32x4 v = ok ? *(const f32x4*)(wcol + h * H + 4 * q) : (f32x4){};
#pragma unroll
      for (int j = 0; j < 4; j++) x[4 * q + j] = nrm ? v[j] / dn : v[j];
    }
#pragma unroll
    for (int ti = 0; ti < NT; ti++) {
      f32x16 acc = {};
      const float* brow = Bm + (int64_t)(ti * 32 + c) * R + h * H;
#pragma unroll
      for (int q = 0; q < H / 4; q++) {
        const f32x4 bv = *(const f32x4*)(brow + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[j], x[4 * q + j], acc, 0, 0, 0);
      }
      if (!ok) continue;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int i0 = ti * 32 + 8 * g + 4 * h;          // rows i0 .. i0 + 3 of column kc are registers 4g .. 4g + 3
        f32x4 xo = *(const f32x4*)(wcol + i0);
        f32x4 xn;
#pragma unroll
        for (int j = 0; j < 4; j++) xn[j] = fmaf(a, nrm ? xo[j] / dn : xo[j], acc[4 * g + j]);
        if (f.p == nullptr) {
          *(f32x4*)(wcol + i0) = xn;
          continue;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int i = i0 + j;
          if (i >= r) continue;
          const int64_t idx = poff + (trans ? (int64_t)kc * r + i : (int64_t)i * L + kc);
          if (f.mode == 0) {
            const float o = xn[j] * sf;
            float pv = f.p[idx];
            pv = fmaf(f.lrwd, pv, pv);                   // p.add_(p, alpha=-lr*wd)
            f.p[idx] = fmaf(f.lr, o, pv);                // p.add_(O, alpha=-lr)
          } else {
            f.p[idx] = xn[j];
          }
        }
      }
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(MU_THREADS) k_muon_update(const int64_t* __restrict__ plan, int n, float* ws, int first, float a, MuFin f) {
  const int64_t chunk = blockIdx.x;
  const int mat = mu_find(plan, n, chunk, MR_CHUNK0);
  const int64_t* rc = mu_rec(plan, mat);
  if (rc[MR_RP] != NT * 32) return;
  mu_update<NT>(ws + rc[MR_W], ws + rc[MR_B], rc, (int)(chunk - rc[MR_CHUNK0]) * MU_CH, first ? ws + rc[MR_NRM] : nullptr, a, f);
}

template <int NT>
static void muon_iter(hipStream_t s, const int64_t* plan_dev, int n, int64_t chunks, float* ws, int first, const float* abc, const MuFin& f) {
  hipLaunchKernelGGL(k_muon_gram<NT>, dim3((unsigned)chunks), dim3(MU_THREADS), 0, s, plan_dev, n, ws, first);
  hipLaunchKernelGGL(k_muon_poly<NT>, dim3((unsigned)n), dim3(MU_THREADS), 0, s, plan_dev, ws, abc[1], abc[2]);
  hipLaunchKernelGGL(k_muon_update<NT>, dim3((unsigned)chunks), dim3(MU_THREADS), 0, s, plan_dev, n, ws, first, abc[0], f);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
extern "C" int st355_muon_plan(const int64_t* offsets, const int32_t* rows, const int32_t* cols, int n, int64_t* plan, int64_t* ws_floats) {
  ST_REQUIRE(offsets && rows && cols && plan && ws_floats && n > 0, "muon_plan: bad args");
  int64_t ws = 0, tiles = 0, chunks = 0;
  for (int i = 0; i < n; i++) {
    ST_REQUIRE(rows[i] > 0 && cols[i] > 0 && offsets[i] >= 0, "muon_plan: matrix %d has shape [%d, %d] at offset %lld", i, rows[i], cols[i],
               (long long)offsets[i]);
    ST_REQUIRE(i == 0 || offsets[i] >= offsets[i - 1] + (int64_t)rows[i - 1] * cols[i - 1], "muon_plan: matrix %d overlaps its predecessor", i);
    const int r = rows[i] < cols[i] ? rows[i] : cols[i], L = rows[i] < cols[i] ? cols[i] : rows[i];
    ST_REQUIRE(r <= MU_MAX_R, "muon_plan: matrix %d has short side %d (the kernel takes at most %d)", i, r, MU_MAX_R);
    const int R = (r + 31) / 32 * 32, NT = R / 32, NU = NT * (NT + 1) / 2;
    const int64_t ntile = (L + MU_TC - 1) / MU_TC, nchunk = (L + MU_CH - 1) / MU_CH;
    int64_t* rc = plan + MP_HDR + (int64_t)i * MR_STRIDE;
    rc[MR_POFF] = offsets[i]; rc[MR_ROWS] = rows[i]; rc[MR_COLS] = cols[i];
    rc[MR_R] = r; rc[MR_L] = L; rc[MR_RP] = R; rc[MR_TRANS] = rows[i] > cols[i];
    rc[MR_W] = ws; ws += (int64_t)L * R;
    rc[MR_B] = ws; ws += (int64_t)R * R;
    rc[MR_GP] = ws; ws += nchunk * NU * 1024;
    rc[MR_SS] = ws; ws += (ntile + 3) / 4 * 4;
    rc[MR_NRM] = ws; ws += 4;
    rc[MR_TILE0] = tiles; rc[MR_NTILE] = ntile; tiles += ntile;
    rc[MR_CHUNK0] = chunks; rc[MR_NCHUNK] = nchunk; chunks += nchunk;
  }
  ST_REQUIRE(tiles < (1ll << 31) && chunks < (1ll << 31), "muon_plan: too many tiles");
  for (int k = 0; k < MP_HDR; k++) plan[k] = 0;
  plan[MP_N] = n; plan[MP_TILES] = tiles; plan[MP_CHUNKS] = chunks; plan[MP_WS] = ws;
  *ws_floats = ws;
  return ST355_OK;
}

static int muon_run(void* stream, const int64_t* plan_host, const int64_t* plan_dev, const float* src, float* mom, float* ws, int64_t ws_floats,
                    int mode, float omm, float gscale, int normalize, float eps, int ns_steps, const float* coeffs, MuFin fin, const char* what) {
  ST_REQUIRE(plan_host && plan_dev && src && ws && coeffs && fin.p, "%s: bad args", what);
  ST_REQUIRE(ns_steps >= 1 && ns_steps < 100, "%s: ns_steps must be in [1, 100)", what);
  const int64_t n = plan_host[MP_N], tiles = plan_host[MP_TILES], chunks = plan_host[MP_CHUNKS];
  ST_REQUIRE(n > 0 && tiles > 0 && chunks > 0, "%s: empty plan", what);
  ST_REQUIRE(ws_floats >= plan_host[MP_WS], "%s: workspace of %lld floats, the plan needs %lld", what, (long long)ws_floats,
             (long long)plan_host[MP_WS]);
  ST_REQUIRE((uintptr_t)ws % 16 == 0, "%s: workspace must be 16-byte aligned", what);
  double flops = 0, elems = 0;
  int cls = 0;                                       // bit t: matrices with R = 32 (t + 1) are present
  for (int64_t i = 0; i < n; i++) {
    const int64_t* rc = plan_host + MP_HDR + i * MR_STRIDE;
    ST_REQUIRE(rc[MR_RP] % 32 == 0 && rc[MR_RP] >= 32 && rc[MR_RP] <= MU_MAX_R, "%s: corrupt plan", what);
    cls |= 1 << (rc[MR_RP] / 32 - 1);
    flops += 4.0 * rc[MR_RP] * rc[MR_RP] * rc[MR_L] * ns_steps;
    elems += (double)rc[MR_R] * rc[MR_L];
  }
  ProfScope ps(stream, ST355_K_OPTIM, flops, (16.0 + 12.0 * ns_steps) * elems);
  hipStream_t s = (hipStream_t)stream;
  const int ni = (int)n;
  hipLaunchKernelGGL(k_muon_prep, dim3((unsigned)tiles), dim3(MU_THREADS), 0, s, plan_dev, ni, src, mom, ws, omm, gscale, mode);
  if (normalize) hipLaunchKernelGGL(k_muon_norm, dim3((unsigned)n), dim3(WAVE), 0, s, plan_dev, ws, eps);
  const MuFin none = {nullptr, mode, 0.f, 0.f, 0.0};
  for (int it = 0; it < ns_steps; it++) {
    const int first = normalize && it == 0;
    const MuFin& f = it == ns_steps - 1 ? fin : none;
    if (cls & 1) muon_iter<1>(s, plan_dev, ni, chunks, ws, first, coeffs + 3 * it, f);
    if (cls & 2) muon_iter<2>(s, plan_dev, ni, chunks, ws, first, coeffs + 3 * it, f);
    if (cls & 4) muon_iter<3>(s, plan_dev, ni, chunks, ws, first, coeffs + 3 * it, f);
    if (cls & 8) muon_iter<4>(s, plan_dev, ni, chunks, ws, first, coeffs + 3 * it, f);
  }
  return st355_check_launch(what);
}

extern "C" int st355_muon_step(void* stream, const int64_t* plan_host, const int64_t* plan_dev, float* p, const float* g, float* m, float* ws,
                               int64_t ws_floats, float grad_scale, double momentum, double lr, double weight_decay, double eps,
                               double rms_scale_factor, int ns_steps, const float* coeffs) {
  ST_REQUIRE(p && g && m, "muon_step: bad args");
  MuFin fin = {p, 0, (float)(-lr * weight_decay), (float)(-lr), rms_scale_factor};
  return muon_run(stream, plan_host, plan_dev, g, m, ws, ws_floats, 0, (float)(1.0 - momentum), grad_scale, 1, (float)eps, ns_steps, coeffs,
                  fin, "muon_step");
}

extern "C" int st355_muon_orthogonalize(void* stream, const int64_t* plan_host, const int64_t* plan_dev, const float* x, float* out, float* ws,
                                        int64_t ws_floats, int normalize, double eps, int ns_steps, const float* coeffs) {
  ST_REQUIRE(x && out, "muon_orthogonalize: bad args");
  MuFin fin = {out, 1, 0.f, 0.f, 1.0};
  return muon_run(stream, plan_host, plan_dev, x, nullptr, ws, ws_floats, 1, 0.f, 1.f, normalize, (float)eps, ns_steps, coeffs, fin,
                  "muon_orthogonalize");
}

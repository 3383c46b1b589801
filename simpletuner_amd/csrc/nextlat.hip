// nextlat.hip — the predictor of NextLat (helpers/training/nextlat.py): LayerNorm(D, eps 1e-6) -> Linear(D -> 2D) -> GELU(erf) -> Linear(2D -> D) on rows 0 .. S-2 of one
// block's image-token output, trained to predict rows 1 .. S-1 (detached) under a smooth-L1 (beta 1) or MSE loss.  All arithmetic fp32, bf16 only in memory, no
// atomics, every reduction in a fixed order (two calls give the same bits).  The GEMMs (U = xhat W1f^T + c1, pred = A Wd^T + bd, dA = psi Wd, g = dU W1f, P1 = dU^T xhat,
// P2 = psi^T A) run on st355_gemm_bf16 / st355_gemm_tn_bf16; the row pass (xhat, rstd) is st355_ig_head_fwd on the view h[:, :S-1].  Here:
//   st355_nextlat_fold          W1f = bf16(gamma * W_up) [2D, D] and its transpose, c1 = bf16(W_up beta + b_up), bf16(W_down) [D, 2D] and its transpose, bf16(b_down).
//                               64 x 64 tiles through LDS: both the straight and the transposed store write 128 contiguous bytes per 8 lanes.
//   st355_gelu_erf_fwd / _bwd   A = gelu_erf(U);  dU = dA * gelu_erf'(U) (dU may be dA), 8 bf16 per lane.
//   st355_nextlat_loss          psi = d(per-element loss) / d pred written over pred (smooth-L1: clamp(pred - t, -1, 1); MSE: 2 (pred - t)), the mean over M * D as one
//                               fp32: per-workgroup partials in a workspace, then one workgroup adds them in index order.
//   st355_nextlat_ln_bwd_add    dx[b, r, :] = bf16(float(dx) + s * rstd * (g - mean_D g - xhat * mean_D(g xhat))), r < S-1: a wave per row, g and xhat kept in registers.
//   st355_nextlat_wgrad_up      from P1 = dU^T xhat (bf16) and db1 = colsum(dU) (fp32): dW_up = s (P1 * gamma + db1 beta^T), db_up = s db1, and the LayerNorm affine's
//                               gradients by contracting with the UNFOLDED W_up (nothing divides by gamma): d gamma[d] = s sum_n W_up[n, d] P1[n, d],
//                               d beta[d] = s sum_n W_up[n, d] db1[n].  Two stages: per 256-row chunk partial column sums, then the chunks in order.
//   st355_nextlat_wgrad_down    dW_down = s P2, db_down = s colsum(psi).
// s is ONE fp32 on the device (nextlat_weight x the upstream gradient x 1 / (M D) x the accumulation division): psi stays unscaled through the bf16 chain.
#include "common.h"

#define NL_MAX_D 4096
#define NL_PASS_COLS 512              // 64 lanes x 8 bf16
#define NL_ROWS_PER_BLOCK 4           // row kernels: one wave per row
#define NL_TILE 64                    // fold: tile edge
#define NL_LOSS_MAX_BLOCKS 1024
#define NL_WG_ROWS 256                // wgrad_up: rows of W_up per workgroup
#define NL_WG_COLS 64                 //           and columns

// 8 consecutive parameter / gradient elements (fp32: two 16-byte accesses, bf16: one)
__device__ __forceinline__ void nl_ld8(const float* p, float (&v)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void nl_ld8(const bf16* p, float (&v)[8]) {
  const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = bf2f(a[j]);
}
__device__ __forceinline__ void nl_st8(float* p, const float (&v)[8], int accumulate) {
  float o[8];
  if (accumulate) {
    nl_ld8(p, o);
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] += v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = v[j];
  }
  *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
  *(float4*)(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
}
__device__ __forceinline__ void nl_st8(bf16* p, const float (&v)[8], int accumulate) {
  float o[8];
  if (accumulate) nl_ld8(p, o);
  bf16x8 w;
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = f2bf(accumulate ? o[j] + v[j] : v[j]);
  *(bf16x8*)p = w;
}
template <typename T> __device__ __forceinline__ float nl_ld(const T* p, int64_t i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void nl_st(T* p, int64_t i, float v, int accumulate) { p[i] = (T)(accumulate ? (float)p[i] + v : v); }

// ---- fold ----
// src [R, Cc] (fp32 or bf16) -> out [R, Cc] = bf16(src * colscale[col]) and outT [Cc, R] its transpose.  A workgroup owns a 64 x 64 tile: thread (row = tid >> 3,
// chunk = tid & 7) converts 8 columns of rows row and row + 32, stores them straight (8 lanes = 128 contiguous bytes of a row) and into the LDS tile; after the barrier
// thread (col = tid >> 3, i = tid & 7) gathers rows 8 i .. 8 i + 7 of columns col and col + 32 and stores 16 bytes of outT (again 128 contiguous bytes per 8 lanes).
// LDS: [64][64] bf16, 16-byte aligned, the 16-byte chunk index XORed with (row >> 3) & 7 (a 16-byte pad per row would keep the vector stores aligned but leaves the
// gather 8-way conflicted: its lanes are 8 rows apart, any row pitch that is a multiple of 16 bytes puts them on one bank).  With the swizzle the 8 values of i hit 8
// different chunks and the 4 columns of a 32-lane group two dwords of each: 16 banks, the column pairs broadcast.
template <typename T>
__global__ void __launch_bounds__(256) k_nl_fold_mat(const T* __restrict__ src, const T* __restrict__ colscale, bf16* __restrict__ out, bf16* __restrict__ outT, int R,
                                                     int Cc) {
  __shared__ __attribute__((aligned(16))) bf16 tile[NL_TILE * NL_TILE];
  const int tid = threadIdx.x, r0 = blockIdx.y * NL_TILE, c0 = blockIdx.x * NL_TILE;
  const int ch = tid & 7;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int r = (tid >> 3) + 32 * k, gr = r0 + r, gc = c0 + ch * 8;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = f2bf(0.f);
    if (gr < R && gc < Cc) {                                      // Cc % 8 == 0: a chunk lies wholly inside or outside
      float v[8];
      nl_ld8(src + (int64_t)gr * Cc + gc, v);
      if (colscale) {
        float s[8];
        nl_ld8(colscale + gc, s);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] *= s[j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf(v[j]);
      *(bf16x8*)(out + (int64_t)gr * Cc + gc) = o;
    }
    *(bf16x8*)(&tile[r * NL_TILE + ((ch ^ ((r >> 3) & 7)) << 3)]) = o;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int cc = (tid >> 3) + 32 * k, i = tid & 7, gcc = c0 + cc, gr = r0 + 8 * i;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = tile[(8 * i + j) * NL_TILE + ((((cc >> 3) ^ i) << 3) | (cc & 7))];
    if (gcc < Cc && gr < R) *(bf16x8*)(outT + (int64_t)gcc * R + gr) = o;          // R % 8 == 0
  }
}

// c1[n] = bf16(sum_d W_up[n, d] beta[d] + b_up[n]): a wave per row n (lane-strided 8-wide partials in column order, xor butterfly); the workgroups behind the
// last row convert b_down
template <typename T>
__global__ void __launch_bounds__(NL_ROWS_PER_BLOCK* WAVE) k_nl_fold_vec(const T* __restrict__ beta, const T* __restrict__ W_up, const T* __restrict__ b_up,
                                                                         const T* __restrict__ b_down, bf16* __restrict__ c1, bf16* __restrict__ bd, int D, int N,
                                                                         int row_blocks) {
  if ((int)blockIdx.x >= row_blocks) {
    const int d = (((int)blockIdx.x - row_blocks) * (NL_ROWS_PER_BLOCK * WAVE) + threadIdx.x) * 8;
    if (d < D) {
      float v[8];
      nl_ld8(b_down + d, v);
      nl_st8(bd + d, v, 0);
    }
    return;
  }
  const int lane = threadIdx.x & (WAVE - 1), n = blockIdx.x * NL_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (n >= N) return;                                             // wave-uniform
  float a = 0.f;
  for (int d = lane * 8; d < D; d += NL_PASS_COLS) {
    float w[8], b[8];
    nl_ld8(W_up + (int64_t)n * D + d, w);
    nl_ld8(beta + d, b);
#pragma unroll
    for (int j = 0; j < 8; j++) a = fmaf(w[j], b[j], a);
  }
  a = wave_sum(a);
  if (lane == 0) c1[n] = f2bf(a + nl_ld(b_up, n));
}

template <typename T>
static void nl_fold_launch(hipStream_t st, const void* gamma, const void* beta, const void* W_up, const void* b_up, const void* W_down, const void* b_down, void* W1f,
                           void* W1fT, void* c1, void* Wd, void* WdT, void* bd, int D) {
  const int N = 2 * D;
  const dim3 block(256);
  hipLaunchKernelGGL(k_nl_fold_mat<T>, dim3((D + NL_TILE - 1) / NL_TILE, (N + NL_TILE - 1) / NL_TILE), block, 0, st, (const T*)W_up, (const T*)gamma, (bf16*)W1f,
                     (bf16*)W1fT, N, D);
  hipLaunchKernelGGL(k_nl_fold_mat<T>, dim3((N + NL_TILE - 1) / NL_TILE, (D + NL_TILE - 1) / NL_TILE), block, 0, st, (const T*)W_down, (const T*)nullptr, (bf16*)Wd,
                     (bf16*)WdT, D, N);
  const int row_blocks = (N + NL_ROWS_PER_BLOCK - 1) / NL_ROWS_PER_BLOCK, per = NL_ROWS_PER_BLOCK * WAVE * 8;
  hipLaunchKernelGGL(k_nl_fold_vec<T>, dim3(row_blocks + (D + per - 1) / per), dim3(NL_ROWS_PER_BLOCK * WAVE), 0, st, (const T*)beta, (const T*)W_up, (const T*)b_up,
                     (const T*)b_down, (bf16*)c1, (bf16*)bd, D, N, row_blocks);
}

#define NL_REQUIRE_D(name)                                                                                                                   \
  ST_REQUIRE(D > 0 && D % 8 == 0 && D <= NL_MAX_D, name ": D must be a multiple of 8, at most %d (got %d)", NL_MAX_D, D)

extern "C" int st355_nextlat_fold(void* stream, const void* gamma, const void* beta, const void* W_up, const void* b_up, const void* W_down, const void* b_down,
                                  int params_bf16, void* W1f, void* W1fT, void* c1, void* Wd, void* WdT, void* bd, int D) {
  ST_REQUIRE(gamma && beta && W_up && b_up && W_down && b_down && W1f && W1fT && c1 && Wd && WdT && bd, "nextlat_fold: bad args");
  NL_REQUIRE_D("nextlat_fold");
  ST_REQUIRE(((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W_up | (uintptr_t)b_up | (uintptr_t)W_down | (uintptr_t)b_down | (uintptr_t)W1f | (uintptr_t)W1fT |
              (uintptr_t)c1 | (uintptr_t)Wd | (uintptr_t)WdT | (uintptr_t)bd) % 16 == 0, "nextlat_fold: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * D * D, (params_bf16 ? 4.0 : 8.0) * 2.0 * D * D + 16.0 * D * D);
  if (params_bf16) nl_fold_launch<bf16>((hipStream_t)stream, gamma, beta, W_up, b_up, W_down, b_down, W1f, W1fT, c1, Wd, WdT, bd, D);
  else nl_fold_launch<float>((hipStream_t)stream, gamma, beta, W_up, b_up, W_down, b_down, W1f, W1fT, c1, Wd, WdT, bd, D);
  return st355_check_launch("nextlat_fold");
}

// ---- GELU (erf) ----
__global__ void __launch_bounds__(256) k_nl_gelu_fwd(const bf16* __restrict__ U, bf16* __restrict__ A, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const bf16x8 u = *(const bf16x8*)(U + i * 8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = f2bf(gelu_erf(bf2f(u[j])));
  *(bf16x8*)(A + i * 8) = o;
}

// (dU may be dA: a lane reads its 8 elements before it writes them)
__global__ void __launch_bounds__(256) k_nl_gelu_bwd(const bf16* __restrict__ U, const bf16* dA, bf16* dU, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const bf16x8 u = *(const bf16x8*)(U + i * 8), d = *(const bf16x8*)(dA + i * 8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = f2bf(bf2f(d[j]) * gelu_erf_grad(bf2f(u[j])));
  *(bf16x8*)(dU + i * 8) = o;
}

extern "C" int st355_gelu_erf_fwd(void* stream, const void* U, void* A, int64_t n) {
  ST_REQUIRE(U && A && n > 0 && n % 8 == 0, "gelu_erf_fwd: bad args (n must be a positive multiple of 8)");
  ST_REQUIRE(((uintptr_t)U | (uintptr_t)A) % 16 == 0, "gelu_erf_fwd: operands must be 16-byte aligned");
  ST_REQUIRE(cdiv64(n / 8, 256) <= 0x7fffffff, "gelu_erf_fwd: too many elements");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 20.0 * n, 4.0 * n);
  hipLaunchKernelGGL(k_nl_gelu_fwd, dim3((unsigned)cdiv64(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)U, (bf16*)A, n / 8);
  return st355_check_launch("gelu_erf_fwd");
}

extern "C" int st355_gelu_erf_bwd(void* stream, const void* U, const void* dA, void* dU, int64_t n) {
  ST_REQUIRE(U && dA && dU && n > 0 && n % 8 == 0, "gelu_erf_bwd: bad args (n must be a positive multiple of 8)");
  ST_REQUIRE(((uintptr_t)U | (uintptr_t)dA | (uintptr_t)dU) % 16 == 0, "gelu_erf_bwd: operands must be 16-byte aligned");
  ST_REQUIRE(cdiv64(n / 8, 256) <= 0x7fffffff, "gelu_erf_bwd: too many elements");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 24.0 * n, 6.0 * n);
  hipLaunchKernelGGL(k_nl_gelu_bwd, dim3((unsigned)cdiv64(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)U, (const bf16*)dA, (bf16*)dU, n / 8);
  return st355_check_launch("gelu_erf_bwd");
}

// ---- loss ----
// workgroup b of G walks rows 4 b + w, 4 (b + G) + w, ... (w = its wave): a lane adds its elements in that order, butterfly per wave, the 4 waves in order
template <int MSE>
__global__ void __launch_bounds__(NL_ROWS_PER_BLOCK* WAVE) k_nl_loss(bf16* pred, const bf16* __restrict__ target, float* __restrict__ partial, int rows, int D,
                                                                     int64_t n_rows, int64_t ld, int64_t bstride) {
  __shared__ float part[NL_ROWS_PER_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  float acc = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * NL_ROWS_PER_BLOCK + w; row < n_rows; row += (int64_t)gridDim.x * NL_ROWS_PER_BLOCK) {
    bf16* pp = pred + row * (int64_t)D;
    const bf16* tp = target + (row / rows) * bstride + (row % rows) * ld;
    for (int c = lane * 8; c < D; c += NL_PASS_COLS) {
      const bf16x8 p = *(const bf16x8*)(pp + c), t = *(const bf16x8*)(tp + c);
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = bf2f(p[j]) - bf2f(t[j]);
        if (MSE) {
          acc = fmaf(d, d, acc);
          o[j] = f2bf(2.f * d);
        } else {
          const float a = fabsf(d);
          acc += a < 1.f ? 0.5f * d * d : a - 0.5f;
          o[j] = f2bf(fminf(fmaxf(d, -1.f), 1.f));
        }
      }
      *(bf16x8*)(pp + c) = o;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(256) k_nl_loss_final(const float* __restrict__ partial, int n, float inv_count, float* __restrict__ loss) {
  __shared__ float part[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
  a = wave_sum(a);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) *loss = ((part[0] + part[1]) + (part[2] + part[3])) * inv_count;
}

static inline int nl_loss_blocks(int64_t n_rows) {
  const int64_t b = cdiv64(n_rows, NL_ROWS_PER_BLOCK);
  return (int)(b < NL_LOSS_MAX_BLOCKS ? b : NL_LOSS_MAX_BLOCKS);
}

extern "C" int64_t st355_nextlat_loss_workspace(int64_t n_rows) { return n_rows > 0 ? (int64_t)nl_loss_blocks(n_rows) * 4 : 0; }

extern "C" int st355_nextlat_loss(void* stream, void* pred, const void* target, int B, int rows, int D, int64_t ld, int64_t bstride, int mode, float* loss, void* ws) {
  ST_REQUIRE(pred && target && loss && ws && B > 0 && rows > 0, "nextlat_loss: bad args");
  ST_REQUIRE(mode == 0 || mode == 1, "nextlat_loss: mode must be 0 (smooth-L1) or 1 (MSE), got %d", mode);
  NL_REQUIRE_D("nextlat_loss");
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "nextlat_loss: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)pred | (uintptr_t)target) % 16 == 0 && (uintptr_t)ws % 4 == 0, "nextlat_loss: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  const int nb = nl_loss_blocks(n);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * n * D, 6.0 * n * D);
  if (mode)
    hipLaunchKernelGGL(k_nl_loss<1>, dim3(nb), dim3(NL_ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, (bf16*)pred, (const bf16*)target, (float*)ws, rows, D, n, ld,
                       bstride);
  else
    hipLaunchKernelGGL(k_nl_loss<0>, dim3(nb), dim3(NL_ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, (bf16*)pred, (const bf16*)target, (float*)ws, rows, D, n, ld,
                       bstride);
  hipLaunchKernelGGL(k_nl_loss_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, nb, (float)(1.0 / ((double)n * (double)D)), loss);
  return st355_check_launch("nextlat_loss");
}

// ---- LayerNorm backward, added into the dX view ----
// NP = passes over the row; a lane keeps its 8 * NP elements of g and of xhat (packed bf16) between the two row sums and the store
template <int NP>
__global__ void __launch_bounds__(NL_ROWS_PER_BLOCK* WAVE) k_nl_ln_bwd_add(const bf16* __restrict__ g, const bf16* __restrict__ xhat, const float* __restrict__ rstd,
                                                                           const float* __restrict__ scale, bf16* dx, int rows, int D, int64_t n_rows, int64_t ld,
                                                                           int64_t bstride, float inv_d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * NL_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                      // wave-uniform: the last block may be partly empty
  const bf16 *gp = g + row * (int64_t)D, *xp = xhat + row * (int64_t)D;
  bf16* dp = dx + (row / rows) * bstride + (row % rows) * ld;
  bf16x8 gv[NP], xv[NP];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * NL_PASS_COLS + lane * 8;
    if (c < D) {                                                  // guarded tail: D % 512 != 0 (D % 8 == 0 keeps a lane's 8 columns together)
      gv[p] = *(const bf16x8*)(gp + c);
      xv[p] = *(const bf16x8*)(xp + c);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float a = bf2f(gv[p][j]);
        s1 += a;
        s2 = fmaf(a, bf2f(xv[p][j]), s2);
      }
    }
  }
  const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;      // xor butterfly: every lane holds the same bits
  const float f = scale[0] * rstd[row];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * NL_PASS_COLS + lane * 8;
    if (c < D) {
      const bf16x8 o = *(const bf16x8*)(dp + c);
      bf16x8 w;
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = f2bf(bf2f(o[j]) + f * ((bf2f(gv[p][j]) - m1) - bf2f(xv[p][j]) * m2));
      *(bf16x8*)(dp + c) = w;
    }
  }
}

extern "C" int st355_nextlat_ln_bwd_add(void* stream, const void* g, const void* xhat, const float* rstd, const float* scale_dev, void* dx, int B, int rows, int D,
                                        int64_t ld, int64_t bstride) {
  ST_REQUIRE(g && xhat && rstd && scale_dev && dx && B > 0 && rows > 0, "nextlat_ln_bwd_add: bad args");
  NL_REQUIRE_D("nextlat_ln_bwd_add");
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "nextlat_ln_bwd_add: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)g | (uintptr_t)xhat | (uintptr_t)dx) % 16 == 0, "nextlat_ln_bwd_add: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  const dim3 grid((unsigned)cdiv64(n, NL_ROWS_PER_BLOCK)), block(NL_ROWS_PER_BLOCK * WAVE);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n * D, 8.0 * n * D);
#define NL_LAUNCH(NP_)                                                                                                                                         \
  hipLaunchKernelGGL(k_nl_ln_bwd_add<NP_>, grid, block, 0, (hipStream_t)stream, (const bf16*)g, (const bf16*)xhat, rstd, scale_dev, (bf16*)dx, rows, D, n, ld, bstride, \
                     (float)(1.0 / (double)D))
  switch ((D + NL_PASS_COLS - 1) / NL_PASS_COLS) {
    case 1: NL_LAUNCH(1); break;
    case 2: NL_LAUNCH(2); break;
    case 3: NL_LAUNCH(3); break;
    case 4: NL_LAUNCH(4); break;
    case 5: case 6: NL_LAUNCH(6); break;
    default: NL_LAUNCH(8); break;
  }
#undef NL_LAUNCH
  return st355_check_launch("nextlat_ln_bwd_add");
}

// ---- weight gradients ----
// stage 1: workgroup (column tile, row chunk) owns 64 columns x 256 rows of W_up.  Thread (cg = tid & 7, rl = tid >> 3) walks rows rl, rl + 32, ... of its 8 columns:
// dW on the way, its partial sums of W * P1 and W * db1 in row order; the 32 row lanes meet in LDS ([32][65] fp32: the column read is one bank per lane, the writes of a
// 32-lane group cover 32 banks) and are added in row-lane order into ws[chunk][0 / 1][D].  Column tile 0 also writes db_up of its rows.
template <typename T>
__global__ void __launch_bounds__(256) k_nl_wgrad_up(const bf16* __restrict__ P1, const float* __restrict__ db1, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                     const T* __restrict__ W, const float* __restrict__ scale, T* g_W, T* g_b, float* __restrict__ ws, int D, int N,
                                                     int accumulate) {
  __shared__ float sg[32][NL_WG_COLS + 1], sb[32][NL_WG_COLS + 1];
  const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
  const int c = blockIdx.x * NL_WG_COLS + cg * 8, n0 = blockIdx.y * NL_WG_ROWS;
  const float s = scale[0];
  if (blockIdx.x == 0 && n0 + tid < N) nl_st(g_b, n0 + tid, s * db1[n0 + tid], accumulate);
  float dg[8], dbe[8];
#pragma unroll
  for (int j = 0; j < 8; j++) dg[j] = dbe[j] = 0.f;
  if (c < D) {
    float ga[8], be[8];
    nl_ld8(gamma + c, ga);
    nl_ld8(beta + c, be);
#pragma unroll 2
    for (int i = 0; i < NL_WG_ROWS / 32; i++) {
      const int n = n0 + rl + 32 * i;
      if (n < N) {
        float p[8], w[8], o[8];
        nl_ld8(P1 + (int64_t)n * D + c, p);
        nl_ld8(W + (int64_t)n * D + c, w);
        const float b = db1[n];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          o[j] = s * fmaf(p[j], ga[j], b * be[j]);
          dg[j] = fmaf(w[j], p[j], dg[j]);
          dbe[j] = fmaf(w[j], b, dbe[j]);
        }
        nl_st8(g_W + (int64_t)n * D + c, o, accumulate);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    sg[rl][cg * 8 + j] = dg[j];
    sb[rl][cg * 8 + j] = dbe[j];
  }
  __syncthreads();
  if (tid < 2 * NL_WG_COLS) {
    const int col = tid & (NL_WG_COLS - 1), which = tid >> 6, d = blockIdx.x * NL_WG_COLS + col;      // wave 0: gamma sums, wave 1: beta sums
    if (d < D) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 32; k++) a += which ? sb[k][col] : sg[k][col];
      ws[((int64_t)blockIdx.y * 2 + which) * D + d] = a;
    }
  }
}

// stage 2: the row chunks in order
template <typename T>
__global__ void __launch_bounds__(256) k_nl_wgrad_up_final(const float* __restrict__ ws, const float* __restrict__ scale, T* g_gamma, T* g_beta, int D, int chunks,
                                                           int accumulate) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < chunks; k++) {
    a += ws[((int64_t)k * 2) * D + d];
    b += ws[((int64_t)k * 2 + 1) * D + d];
  }
  const float s = scale[0];
  nl_st(g_gamma, d, s * a, accumulate);
  nl_st(g_beta, d, s * b, accumulate);
}

extern "C" int64_t st355_nextlat_wgrad_workspace(int D) { return D > 0 ? (int64_t)((2 * D + NL_WG_ROWS - 1) / NL_WG_ROWS) * 2 * D * 4 : 0; }

template <typename T>
static void nl_wgrad_up_launch(hipStream_t st, const void* P1, const float* db1, const void* gamma, const void* beta, const void* W, const float* scale, void* g_gamma,
                               void* g_beta, void* g_W, void* g_b, float* ws, int D, int accumulate) {
  const int N = 2 * D, chunks = (N + NL_WG_ROWS - 1) / NL_WG_ROWS;
  hipLaunchKernelGGL(k_nl_wgrad_up<T>, dim3((D + NL_WG_COLS - 1) / NL_WG_COLS, chunks), dim3(256), 0, st, (const bf16*)P1, db1, (const T*)gamma, (const T*)beta,
                     (const T*)W, scale, (T*)g_W, (T*)g_b, ws, D, N, accumulate);
  hipLaunchKernelGGL(k_nl_wgrad_up_final<T>, dim3((D + 255) / 256), dim3(256), 0, st, (const float*)ws, scale, (T*)g_gamma, (T*)g_beta, D, chunks, accumulate);
}

extern "C" int st355_nextlat_wgrad_up(void* stream, const void* P1, const float* db1, const void* gamma, const void* beta, const void* W_up, int params_bf16,
                                      const float* scale_dev, void* g_gamma, void* g_beta, void* g_W, void* g_b, int D, int accumulate, void* ws) {
  ST_REQUIRE(P1 && db1 && gamma && beta && W_up && scale_dev && g_gamma && g_beta && g_W && g_b && ws, "nextlat_wgrad_up: bad args");
  NL_REQUIRE_D("nextlat_wgrad_up");
  ST_REQUIRE(((uintptr_t)P1 | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W_up | (uintptr_t)g_W | (uintptr_t)ws) % 16 == 0,
             "nextlat_wgrad_up: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 12.0 * D * D, (params_bf16 ? 12.0 : 20.0) * D * D);
  if (params_bf16) nl_wgrad_up_launch<bf16>((hipStream_t)stream, P1, db1, gamma, beta, W_up, scale_dev, g_gamma, g_beta, g_W, g_b, (float*)ws, D, accumulate);
  else nl_wgrad_up_launch<float>((hipStream_t)stream, P1, db1, gamma, beta, W_up, scale_dev, g_gamma, g_beta, g_W, g_b, (float*)ws, D, accumulate);
  return st355_check_launch("nextlat_wgrad_up");
}

// dW_down = s P2 (8 elements per lane); the workgroups behind the matrix write db_down = s db2
template <typename T>
__global__ void __launch_bounds__(256) k_nl_wgrad_down(const bf16* __restrict__ P2, const float* __restrict__ db2, const float* __restrict__ scale, T* g_W, T* g_b,
                                                       int64_t n8, int mat_blocks, int D, int accumulate) {
  const float s = scale[0];
  if ((int)blockIdx.x >= mat_blocks) {
    const int d = (((int)blockIdx.x - mat_blocks) * 256 + threadIdx.x) * 8;
    if (d < D) {
      float v[8];
      nl_ld8(db2 + d, v);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] *= s;
      nl_st8(g_b + d, v, accumulate);
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float v[8];
  nl_ld8(P2 + i * 8, v);
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] *= s;
  nl_st8(g_W + i * 8, v, accumulate);
}

extern "C" int st355_nextlat_wgrad_down(void* stream, const void* P2, const float* db2, int params_bf16, const float* scale_dev, void* g_W, void* g_b, int D,
                                        int accumulate) {
  ST_REQUIRE(P2 && db2 && scale_dev && g_W && g_b, "nextlat_wgrad_down: bad args");
  NL_REQUIRE_D("nextlat_wgrad_down");
  ST_REQUIRE(((uintptr_t)P2 | (uintptr_t)db2 | (uintptr_t)g_W | (uintptr_t)g_b) % 16 == 0, "nextlat_wgrad_down: operands must be 16-byte aligned");
  const int64_t n8 = (int64_t)D * 2 * D / 8;
  const int mat_blocks = (int)cdiv64(n8, 256), vec_blocks = (D / 8 + 255) / 256;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * D * D, (params_bf16 ? 8.0 : 12.0) * D * D);
  if (params_bf16)
    hipLaunchKernelGGL(k_nl_wgrad_down<bf16>, dim3(mat_blocks + vec_blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)P2, db2, scale_dev, (bf16*)g_W, (bf16*)g_b,
                       n8, mat_blocks, D, accumulate);
  else
    hipLaunchKernelGGL(k_nl_wgrad_down<float>, dim3(mat_blocks + vec_blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)P2, db2, scale_dev, (float*)g_W,
                       (float*)g_b, n8, mat_blocks, D, accumulate);
  return st355_check_launch("nextlat_wgrad_down");
}

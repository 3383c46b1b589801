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
#include "feature_common.h"

#define NL_MAX_D 4096
#define NL_LOSS_MAX_BLOCKS 1024

// ---- fold ----
// the two matrices: k_fold_mat of feature_common.h (W_up with gamma as its column scale, W_down with none).
// c1[n] = bf16(sum_d W_up[n, d] beta[d] + b_up[n]): a wave per row n (lane-strided 8-wide partials in column order, xor butterfly); the workgroups behind the
// last row convert b_down
template <typename T>
__global__ void __launch_bounds__(ROWS_PER_BLOCK* WAVE) k_nl_fold_vec(const T* __restrict__ beta, const T* __restrict__ W_up, const T* __restrict__ b_up,
                                                                      const T* __restrict__ b_down, bf16* __restrict__ c1, bf16* __restrict__ bd, int D, int N,
                                                                      int row_blocks) {
  if ((int)blockIdx.x >= row_blocks) {
    const int d = (((int)blockIdx.x - row_blocks) * (ROWS_PER_BLOCK * WAVE) + threadIdx.x) * 8;
    if (d < D) {
      float v[8];
      ld8(b_down + d, v);
      st8(bd + d, v, 0);
    }
    return;
  }
  const int lane = threadIdx.x & (WAVE - 1), n = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (n >= N) return;                                             // wave-uniform
  fold_row_dot(W_up, beta, b_up, c1, D, n, lane);
}

template <typename T>
static void nl_fold_launch(hipStream_t st, const void* gamma, const void* beta, const void* W_up, const void* b_up, const void* W_down, const void* b_down, void* W1f,
                           void* W1fT, void* c1, void* Wd, void* WdT, void* bd, int D) {
  const int N = 2 * D;
  const dim3 block(256);
  hipLaunchKernelGGL(k_fold_mat<T>, dim3((D + FOLD_TILE - 1) / FOLD_TILE, (N + FOLD_TILE - 1) / FOLD_TILE), block, 0, st, (const T*)W_up, (const T*)gamma, (bf16*)W1f,
                     (bf16*)W1fT, N, D);
  hipLaunchKernelGGL(k_fold_mat<T>, dim3((N + FOLD_TILE - 1) / FOLD_TILE, (D + FOLD_TILE - 1) / FOLD_TILE), block, 0, st, (const T*)W_down, (const T*)nullptr, (bf16*)Wd,
                     (bf16*)WdT, D, N);
  const int row_blocks = (N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, per = ROWS_PER_BLOCK * WAVE * 8;
  hipLaunchKernelGGL(k_nl_fold_vec<T>, dim3(row_blocks + (D + per - 1) / per), dim3(ROWS_PER_BLOCK * WAVE), 0, st, (const T*)beta, (const T*)W_up, (const T*)b_up,
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
__global__ void __launch_bounds__(ROWS_PER_BLOCK* WAVE) k_nl_loss(bf16* pred, const bf16* __restrict__ target, float* __restrict__ partial, int rows, int D,
                                                                  int64_t n_rows, int64_t ld, int64_t bstride) {
  __shared__ float part[ROWS_PER_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  float acc = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w; row < n_rows; row += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
    bf16* pp = pred + row * (int64_t)D;
    const bf16* tp = target + (row / rows) * bstride + (row % rows) * ld;
    for (int c = lane * 8; c < D; c += ROW_PASS_COLS) {
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
  // (pairwise, not block_reduce's wave order: this kernel's bits since its first release)
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
  const int64_t b = cdiv64(n_rows, ROWS_PER_BLOCK);
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
    hipLaunchKernelGGL(k_nl_loss<1>, dim3(nb), dim3(ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, (bf16*)pred, (const bf16*)target, (float*)ws, rows, D, n, ld,
                       bstride);
  else
    hipLaunchKernelGGL(k_nl_loss<0>, dim3(nb), dim3(ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, (bf16*)pred, (const bf16*)target, (float*)ws, rows, D, n, ld,
                       bstride);
  hipLaunchKernelGGL(k_nl_loss_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, nb, (float)(1.0 / ((double)n * (double)D)), loss);
  return st355_check_launch("nextlat_loss");
}

// ---- LayerNorm backward, added into the dX view ----
// NP = passes over the row; a lane keeps its 8 * NP elements of g and of xhat (packed bf16) between the two row sums and the store
template <int NP>
__global__ void __launch_bounds__(ROWS_PER_BLOCK* WAVE) k_nl_ln_bwd_add(const bf16* __restrict__ g, const bf16* __restrict__ xhat, const float* __restrict__ rstd,
                                                                        const float* __restrict__ scale, bf16* dx, int rows, int D, int64_t n_rows, int64_t ld,
                                                                        int64_t bstride, float inv_d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                      // wave-uniform: the last block may be partly empty
  const bf16 *gp = g + row * (int64_t)D, *xp = xhat + row * (int64_t)D;
  bf16* dp = dx + (row / rows) * bstride + (row % rows) * ld;
  bf16x8 gv[NP], xv[NP];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * ROW_PASS_COLS + lane * 8;
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
    const int c = p * ROW_PASS_COLS + lane * 8;
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
  const dim3 grid((unsigned)cdiv64(n, ROWS_PER_BLOCK)), block(ROWS_PER_BLOCK * WAVE);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n * D, 8.0 * n * D);
#define NL_LAUNCH(NP_)                                                                                                                                         \
  hipLaunchKernelGGL(k_nl_ln_bwd_add<NP_>, grid, block, 0, (hipStream_t)stream, (const bf16*)g, (const bf16*)xhat, rstd, scale_dev, (bf16*)dx, rows, D, n, ld, bstride, \
                     (float)(1.0 / (double)D))
  switch ((D + ROW_PASS_COLS - 1) / ROW_PASS_COLS) {
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
// W_up: k_wgrad_up / k_wgrad_up_final of feature_common.h over its N = 2D rows
extern "C" int64_t st355_nextlat_wgrad_workspace(int D) { return D > 0 ? wgrad_up_workspace(D, 2 * D) : 0; }

extern "C" int st355_nextlat_wgrad_up(void* stream, const void* P1, const float* db1, const void* gamma, const void* beta, const void* W_up, int params_bf16,
                                      const float* scale_dev, void* g_gamma, void* g_beta, void* g_W, void* g_b, int D, int accumulate, void* ws) {
  ST_REQUIRE(P1 && db1 && gamma && beta && W_up && scale_dev && g_gamma && g_beta && g_W && g_b && ws, "nextlat_wgrad_up: bad args");
  NL_REQUIRE_D("nextlat_wgrad_up");
  ST_REQUIRE(((uintptr_t)P1 | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W_up | (uintptr_t)g_W | (uintptr_t)ws) % 16 == 0,
             "nextlat_wgrad_up: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 12.0 * D * D, (params_bf16 ? 12.0 : 20.0) * D * D);
  if (params_bf16) wgrad_up_launch<bf16, false>((hipStream_t)stream, P1, db1, gamma, beta, W_up, scale_dev, g_gamma, g_beta, g_W, g_b, (float*)ws, D, 2 * D, accumulate);
  else wgrad_up_launch<float, false>((hipStream_t)stream, P1, db1, gamma, beta, W_up, scale_dev, g_gamma, g_beta, g_W, g_b, (float*)ws, D, 2 * D, accumulate);
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
      ld8(db2 + d, v);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] *= s;
      st8(g_b + d, v, accumulate);
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float v[8];
  ld8(P2 + i * 8, v);
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] *= s;
  st8(g_W + i * 8, v, accumulate);
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

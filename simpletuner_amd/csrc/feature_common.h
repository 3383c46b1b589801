// feature_common.h — what the training-feature kernels share (internal_guidance / nextlat / reflexflow / flow_dpo / diff2flow / self_flow / twinflow /
// eval_loss / self_transcendence / lcm): the 16-byte access helpers, the grid rule and the block reduction of the per-sample streaming losses, the 64 x 64 fold
// tile, the projector's row dot, the LayerNorm row pass and the two-stage LayerNorm-affine / Linear weight gradient.  Every "two calls give the same bits"
// guarantee of those files rests on the fixed orders written here ONCE; each feature's own arithmetic stays in its file.
#pragma once
#include "optim_common.h"

// ---- 8-wide access ------------------------------------------------------------------------------------------------------------------------------------------------
// 8 consecutive elements (fp32: two 16-byte accesses, bf16: one), widened to fp32
__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int j = 0; j < 4; j++) { v[j] = a[j]; v[j + 4] = b[j]; }
}
__device__ __forceinline__ void ld8(const bf16* p, float (&v)[8]) {
  const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = bf2f(a[j]);
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8], int accumulate) {
  float o[8];
  if (accumulate) {
    ld8(p, o);
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] += v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = v[j];
  }
  *(f32x4*)p = f32x4{o[0], o[1], o[2], o[3]};
  *(f32x4*)(p + 4) = f32x4{o[4], o[5], o[6], o[7]};
}
__device__ __forceinline__ void st8(bf16* p, const float (&v)[8], int accumulate) {
  float o[8];
  if (accumulate) ld8(p, o);
  bf16x8 w;
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = f2bf(accumulate ? o[j] + v[j] : v[j]);
  *(bf16x8*)p = w;
}
template <typename T> __device__ __forceinline__ float ld(const T* p, int64_t i) { return (float)p[i]; }
template <typename T> __device__ __forceinline__ void st(T* p, int64_t i, float v, int accumulate) { p[i] = (T)(accumulate ? (float)p[i] + v : v); }

// the tail-aware forms: 8 elements from e0 of a row — VEC: the 16-byte access(es) above; else `cnt` scalar ones (a load's rest is zero)
template <bool VEC, typename T>
__device__ __forceinline__ void load8(const T* src, int64_t e0, int cnt, float (&v)[8]) {
  if (VEC) {
    ld8(src + e0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = j < cnt ? (float)src[e0 + j] : 0.f;
  }
}
template <bool VEC, typename T>
__device__ __forceinline__ void store8(T* dst, int64_t e0, int cnt, const float (&v)[8]) {
  if (VEC) {
    st8(dst + e0, v, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (j < cnt) dst[e0 + j] = (T)v[j];
  }
}

// ---- the per-sample streaming losses --------------------------------------------------------------------------------------------------------------------------------
// partial workgroups per sample: the op_blocks grid (at most 2048 workgroups of 256 lanes, 8 elements per lane) divided among the samples
static inline int sample_parts(int64_t batch, int64_t per_sample) {
  int64_t p = cdiv64(cdiv64(per_sample, 8), OP_THREADS);
  const int64_t cap = (256 * 8) / batch;
  if (p > cap) p = cap;
  if (p < 1) p = 1;
  return (int)p;
}

// the block's NV sums -> ws[(row * gridDim.x + blockIdx.x) * STRIDE + k], the partial-workspace layout of every streaming loss (row = the sample, or the
// (slab, sample) pair): lane tree, then the wave partials in wave order (workgroups of OP_THREADS).  `row` must reach here already 64-bit — the slot index is
// computed from it, so a caller's 32-bit product (k * B + b) would overflow before the conversion
template <int NV, int STRIDE = NV>
__device__ __forceinline__ void block_reduce(float (&acc)[NV], float* __restrict__ ws, int64_t row) {
  __shared__ float red[NV][OP_THREADS / WAVE];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const float s = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    float s = 0.f;
    for (int w = 0; w < OP_THREADS / WAVE; w++) s += red[threadIdx.x][w];
    ws[(row * gridDim.x + blockIdx.x) * STRIDE + threadIdx.x] = s;
  }
}

// stage 2 of the one-accumulator losses (diff2flow, lcm), one workgroup: per sample the partials in index order -> per_sample[b] = (weight[b] *) sum / n; then the
// batch mean in sample order.  The kernel and this launcher live in diff2flow.hip (the family's one call across objects; hidden: not part of the library's ABI)
__attribute__((visibility("hidden"))) void sample_mean_finish(hipStream_t st, const float* ws, const float* weight, float* loss, float* per_sample_out, int B, int parts, float inv_per_sample);

// ---- fold -----------------------------------------------------------------------------------------------------------------------------------------------------------
// One 64 x 64 tile of src [R, Cc] (fp32 or bf16) -> out [R, Cc] = bf16(src * colscale[col]) (colscale == nullptr: bf16(src)) and outT [Cc, R] its transpose, by a
// workgroup of 256.  Thread (row = tid >> 3, chunk = tid & 7) converts 8 columns of rows row and row + 32, stores them straight (8 lanes = 128 contiguous bytes of
// a row) and into the LDS tile; after the barrier thread (col = tid >> 3, i = tid & 7) gathers rows 8 i .. 8 i + 7 of columns col and col + 32 and stores 16 bytes
// of outT (again 128 contiguous bytes per 8 lanes).  LDS: [64][64] bf16, 16-byte aligned, the 16-byte chunk index XORed with (row >> 3) & 7 (a 16-byte pad per row
// would keep the vector stores aligned but leaves the gather 8-way conflicted: its lanes are 8 rows apart, any row pitch that is a multiple of 16 bytes puts them on
// one bank).  With the swizzle the 8 values of i hit 8 different chunks and the 4 columns of a 32-lane group two dwords of each: 16 banks, the column pairs broadcast.
#define FOLD_TILE 64
template <typename T>
__device__ __forceinline__ void fold_tile(bf16* tile, const T* __restrict__ src, const T* __restrict__ colscale, bf16* __restrict__ out, bf16* __restrict__ outT, int R,
                                          int Cc, int r0, int c0) {
  const int tid = threadIdx.x, ch = tid & 7;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int r = (tid >> 3) + 32 * k, gr = r0 + r, gc = c0 + ch * 8;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = f2bf(0.f);
    if (gr < R && gc < Cc) {                                      // Cc % 8 == 0: a chunk lies wholly inside or outside
      float v[8];
      ld8(src + (int64_t)gr * Cc + gc, v);
      if (colscale) {
        float s[8];
        ld8(colscale + gc, s);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] *= s[j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf(v[j]);
      *(bf16x8*)(out + (int64_t)gr * Cc + gc) = o;
    }
    *(bf16x8*)(&tile[r * FOLD_TILE + ((ch ^ ((r >> 3) & 7)) << 3)]) = o;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int cc = (tid >> 3) + 32 * k, i = tid & 7, gcc = c0 + cc, gr = r0 + 8 * i;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = tile[(8 * i + j) * FOLD_TILE + ((((cc >> 3) ^ i) << 3) | (cc & 7))];
    if (gcc < Cc && gr < R) *(bf16x8*)(outT + (int64_t)gcc * R + gr) = o;          // R % 8 == 0
  }
}

// grid = (column tiles, row tiles), 256 threads
template <typename T>
__global__ void __launch_bounds__(256) k_fold_mat(const T* __restrict__ src, const T* __restrict__ colscale, bf16* __restrict__ out, bf16* __restrict__ outT, int R,
                                                  int Cc) {
  __shared__ __attribute__((aligned(16))) bf16 tile[FOLD_TILE * FOLD_TILE];
  fold_tile(tile, src, colscale, out, outT, R, Cc, blockIdx.y * FOLD_TILE, blockIdx.x * FOLD_TILE);
}

// ---- rows: a wave per row, 64 lanes x 8 bf16 per pass ---------------------------------------------------------------------------------------------------------------
#define ROW_PASS_COLS 512
#define ROWS_PER_BLOCK 4
#define ROW_MAX_PASSES 8              // D <= 4096

// c[n] = bf16(sum_d W[n, d] beta[d] + b[n]) by the wave of row n: lane-strided 8-wide partials in column order, then the xor butterfly
template <typename T>
__device__ __forceinline__ void fold_row_dot(const T* __restrict__ W, const T* __restrict__ beta, const T* __restrict__ b, bf16* __restrict__ c, int D, int n, int lane) {
  float a = 0.f;
  for (int d = lane * 8; d < D; d += ROW_PASS_COLS) {
    float w[8], be[8];
    ld8(W + (int64_t)n * D + d, w);
    ld8(beta + d, be);
#pragma unroll
    for (int j = 0; j < 8; j++) a = fmaf(w[j], be[j], a);
  }
  a = wave_sum(a);
  if (lane == 0) c[n] = f2bf(a + ld(b, n));
}

// the LayerNorm row pass over the [B, rows, D] view: mean, CENTRED variance (no E[x^2] - mean^2 cancellation on a row of large offset), xhat (compact bf16), rstd.
// NP = passes over the row (3 at D = 1536, 6 at D = 3072); a lane keeps its 8 * NP elements (packed bf16) between the two reductions and the store.  The eps is a
// compile-time tag: the heads of Internal Guidance and NextLat use 1e-6, Self-Flow's projector nn.LayerNorm's default 1e-5.
struct RowEps1e6 { static constexpr float value = 1e-6f; };
struct RowEps1e5 { static constexpr float value = 1e-5f; };

template <int NP, typename EPS>
__global__ void __launch_bounds__(ROWS_PER_BLOCK* WAVE) k_rows_fwd(const bf16* __restrict__ h, bf16* __restrict__ xhat, float* __restrict__ rstd, int rows, int D,
                                                                   int64_t n_rows, int64_t row_ld, int64_t bstride, float inv_d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                      // wave-uniform: the last block may be partly empty
  const bf16* hp = h + (row / rows) * bstride + (row % rows) * row_ld;
  bf16x8 v[NP];
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * ROW_PASS_COLS + lane * 8;
    if (c < D) {                                                  // guarded tail: D % 512 != 0 (D % 8 == 0 keeps a lane's 8 columns together)
      v[p] = *(const bf16x8*)(hp + c);
#pragma unroll
      for (int j = 0; j < 8; j++) s += bf2f(v[p][j]);
    }
  }
  const float mean = wave_sum(s) * inv_d;                         // xor butterfly: every lane holds the same bits
  float q = 0.f;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    if (p * ROW_PASS_COLS + lane * 8 < D) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = bf2f(v[p][j]) - mean;
        q = fmaf(d, d, q);
      }
    }
  }
  const float rs = 1.f / sqrtf(wave_sum(q) * inv_d + EPS::value);
  if (lane == 0) rstd[row] = rs;
  bf16* xp = xhat + row * (int64_t)D;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * ROW_PASS_COLS + lane * 8;
    if (c < D) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf((bf2f(v[p][j]) - mean) * rs);
      *(bf16x8*)(xp + c) = o;
    }
  }
}

// n = B * rows rows of D <= 4096 columns, dispatched on the pass count
template <typename EPS>
static void rows_fwd_launch(hipStream_t st, const bf16* h, bf16* xhat, float* rstd, int rows, int D, int64_t n, int64_t row_ld, int64_t bstride) {
  const dim3 grid((unsigned)cdiv64(n, ROWS_PER_BLOCK)), block(ROWS_PER_BLOCK * WAVE);
#define ROWS_LAUNCH(NP_) hipLaunchKernelGGL((k_rows_fwd<NP_, EPS>), grid, block, 0, st, h, xhat, rstd, rows, D, n, row_ld, bstride, (float)(1.0 / (double)D))
  switch ((D + ROW_PASS_COLS - 1) / ROW_PASS_COLS) {
    case 1: ROWS_LAUNCH(1); break;
    case 2: ROWS_LAUNCH(2); break;
    case 3: ROWS_LAUNCH(3); break;
    case 4: ROWS_LAUNCH(4); break;
    case 5: case 6: ROWS_LAUNCH(6); break;
    default: ROWS_LAUNCH(8); break;
  }
#undef ROWS_LAUNCH
}

// ---- weight gradients of LayerNorm(D) -> Linear(D -> N) -------------------------------------------------------------------------------------------------------------
// From P = dU^T xhat [N, D] (bf16) and db = colsum(dU) [N] (fp32): dW = s (P * gamma + db beta^T), d b = s db, and the LayerNorm affine's gradients by contracting with
// the UNFOLDED W (nothing divides by gamma): d gamma[d] = s sum_n W[n, d] P[n, d], d beta[d] = s sum_n W[n, d] db[n].
// stage 1: workgroup (column tile, row chunk) owns 64 columns x 256 rows of W.  Thread (cg = tid & 7, rl = tid >> 3) walks rows rl, rl + 32, ... of its 8 columns:
// dW on the way, its partial sums of W * P and W * db in row order; the 32 row lanes meet in LDS ([32][65] fp32: the column read is one bank per lane, the writes of a
// 32-lane group cover 32 banks) and are added in row-lane order into ws[chunk][0 / 1][D].  Column tile 0 also writes d b of its rows.
#define WG_ROWS 256
#define WG_COLS 64
template <typename T>
__global__ void __launch_bounds__(256) k_wgrad_up(const bf16* __restrict__ P, const float* __restrict__ db, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                  const T* __restrict__ W, const float* __restrict__ scale, T* g_W, T* g_b, float* __restrict__ ws, int D, int N,
                                                  int accumulate) {
  __shared__ float sg[32][WG_COLS + 1], sb[32][WG_COLS + 1];
  const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
  const int c = blockIdx.x * WG_COLS + cg * 8, n0 = blockIdx.y * WG_ROWS;
  const float s = scale[0];
  if (blockIdx.x == 0 && n0 + tid < N) st(g_b, n0 + tid, s * db[n0 + tid], accumulate);
  float dg[8], dbe[8];
#pragma unroll
  for (int j = 0; j < 8; j++) dg[j] = dbe[j] = 0.f;
  if (c < D) {
    float ga[8], be[8];
    ld8(gamma + c, ga);
    ld8(beta + c, be);
#pragma unroll 2
    for (int i = 0; i < WG_ROWS / 32; i++) {
      const int n = n0 + rl + 32 * i;
      if (n < N) {
        float p[8], w[8], o[8];
        ld8(P + (int64_t)n * D + c, p);
        ld8(W + (int64_t)n * D + c, w);
        const float b = db[n];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          o[j] = s * fmaf(p[j], ga[j], b * be[j]);
          dg[j] = fmaf(w[j], p[j], dg[j]);
          dbe[j] = fmaf(w[j], b, dbe[j]);
        }
        st8(g_W + (int64_t)n * D + c, o, accumulate);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    sg[rl][cg * 8 + j] = dg[j];
    sb[rl][cg * 8 + j] = dbe[j];
  }
  __syncthreads();
  if (tid < 2 * WG_COLS) {
    const int col = tid & (WG_COLS - 1), which = tid >> 6, d = blockIdx.x * WG_COLS + col;      // wave 0: gamma sums, wave 1: beta sums
    if (d < D) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 32; k++) a += which ? sb[k][col] : sg[k][col];
      ws[((int64_t)blockIdx.y * 2 + which) * D + d] = a;
    }
  }
}

// stage 2: the row chunks in order.  FUSED says how the accumulating store rounds, which the two callers have always done differently: NextLat adds the rounded
// product s * sum to the gradient (two roundings), Self-Flow forms fma(s, sum, gradient) (one)
template <typename T, bool FUSED>
__global__ void __launch_bounds__(256) k_wgrad_up_final(const float* __restrict__ ws, const float* __restrict__ scale, T* g_gamma, T* g_beta, int D, int chunks,
                                                        int accumulate) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < chunks; k++) {
    a += ws[((int64_t)k * 2) * D + d];
    b += ws[((int64_t)k * 2 + 1) * D + d];
  }
  const float s = scale[0];
  if (FUSED && accumulate) {
    g_gamma[d] = (T)fmaf(s, a, (float)g_gamma[d]);
    g_beta[d] = (T)fmaf(s, b, (float)g_beta[d]);
  } else {
    st(g_gamma, d, s * a, accumulate);
    st(g_beta, d, s * b, accumulate);
  }
}

// bytes of ws for N rows: cdiv(N, 256) chunks of two fp32 rows of D
static inline int64_t wgrad_up_workspace(int D, int N) { return (int64_t)((N + WG_ROWS - 1) / WG_ROWS) * 2 * D * 4; }

template <typename T, bool FUSED>
static void wgrad_up_launch(hipStream_t st, const void* P, const float* db, const void* gamma, const void* beta, const void* W, const float* scale, void* g_gamma,
                            void* g_beta, void* g_W, void* g_b, float* ws, int D, int N, int accumulate) {
  const int chunks = (N + WG_ROWS - 1) / WG_ROWS;
  hipLaunchKernelGGL(k_wgrad_up<T>, dim3((D + WG_COLS - 1) / WG_COLS, chunks), dim3(256), 0, st, (const bf16*)P, db, (const T*)gamma, (const T*)beta, (const T*)W, scale,
                     (T*)g_W, (T*)g_b, ws, D, N, accumulate);
  hipLaunchKernelGGL((k_wgrad_up_final<T, FUSED>), dim3((D + 255) / 256), dim3(256), 0, st, (const float*)ws, scale, (T*)g_gamma, (T*)g_beta, D, chunks, accumulate);
}

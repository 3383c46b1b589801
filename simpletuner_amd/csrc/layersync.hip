// layersync.hip — LayerSync self-alignment regulariser (helpers/training/layersync.py): per token row the cosine between a student and a (detached) teacher block
// output, its mean over all rows, and d mean / d student — one bandwidth-bound pass (reads 2, writes 1 tensor of B * rows * D bf16) plus a single-block fixed-order
// sum; and the pass that adds the scaled gradient into the dX chain at the student block.  All arithmetic fp32, F.normalize semantics (x / max(|x|, 1e-12)).
#include "common.h"

#define LS_EPS 1e-12f
#define LS_ROWS_PER_BLOCK 4           // one wave per row
#define LS_PASS_COLS 512              // 64 lanes x 8 bf16 (one 16-byte load per lane per pass)
#define LS_MAX_PASSES 8               // D <= 4096
#define LS_MEAN_THREADS 1024

// NP = passes over the row (3 at D = 1536, 6 at D = 3072).  A lane keeps its 8 * NP elements of both rows in registers (packed bf16) between the reduction and
// the store, so G may alias the student rows: every lane writes exactly the elements it has read, after it has read them.
template <int NP>
__global__ void __launch_bounds__(LS_ROWS_PER_BLOCK* WAVE) k_layersync_fwd(const bf16* student, const bf16* __restrict__ teacher, bf16* G,
                                                                           float* __restrict__ cos_rows, int rows, int D, int64_t n_rows, int64_t ld,
                                                                           int64_t s_bstride, int64_t t_bstride, float inv_n) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * LS_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                      // wave-uniform: the last block may be partly empty
  const int64_t b = row / rows, r = row % rows;
  const bf16* sp = student + b * s_bstride + r * ld;
  const bf16* tp = teacher + b * t_bstride + r * ld;
  bf16x8 sv[NP], tv[NP];
  float ss = 0.f, tt = 0.f, st = 0.f;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int c = p * LS_PASS_COLS + lane * 8;
    if (c < D) {                                                  // guarded tail: D % 512 != 0 (D % 8 == 0 keeps a lane's 8 columns together)
      sv[p] = *(const bf16x8*)(sp + c);
      tv[p] = *(const bf16x8*)(tp + c);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float s = bf2f(sv[p][j]), t = bf2f(tv[p][j]);
        ss = fmaf(s, s, ss); tt = fmaf(t, t, tt); st = fmaf(s, t, st);
      }
    }
  }
  ss = wave_sum(ss); tt = wave_sum(tt); st = wave_sum(st);       // xor butterfly: every lane holds the same bits
  const float is = 1.f / fmaxf(sqrtf(ss), LS_EPS), it = 1.f / fmaxf(sqrtf(tt), LS_EPS);
  const float c = st * is * it;
  if (lane == 0) cos_rows[row] = c;
  const float gs = is * inv_n;
  bf16* gp = G + row * (int64_t)D;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const int col = p * LS_PASS_COLS + lane * 8;
    if (col < D) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf((bf2f(tv[p][j]) * it - c * (bf2f(sv[p][j]) * is)) * gs);
      *(bf16x8*)(gp + col) = o;
    }
  }
}

// sim[0] = mean(cos_rows): ONE block, fixed order (thread-strided partial sums, butterfly per wave, the 16 wave sums in index order) — no atomics, bit-reproducible
__global__ void __launch_bounds__(LS_MEAN_THREADS) k_layersync_mean(const float* __restrict__ cos_rows, float* __restrict__ sim, int64_t n, float inv_n) {
  __shared__ float part[LS_MEAN_THREADS / WAVE];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += LS_MEAN_THREADS) a += cos_rows[i];
  a = wave_sum(a);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LS_MEAN_THREADS / WAVE; w++) s += part[w];
    sim[0] = s * inv_n;
  }
}

extern "C" int st355_layersync_fwd(void* stream, const void* student, const void* teacher, void* G, float* cos_rows, float* sim, int B, int rows, int D, int64_t ld,
                                   int64_t s_bstride, int64_t t_bstride, void* ws) {
  (void)ws;                                                       // no workspace: cos_rows is the only intermediate
  ST_REQUIRE(student && teacher && G && cos_rows && sim && B > 0 && rows > 0 && D > 0, "layersync_fwd: bad args");
  ST_REQUIRE(D % 8 == 0 && D <= LS_PASS_COLS * LS_MAX_PASSES, "layersync_fwd: D must be a multiple of 8, at most %d (got %d)", LS_PASS_COLS * LS_MAX_PASSES, D);
  ST_REQUIRE(ld >= D && ld % 8 == 0 && s_bstride % 8 == 0 && t_bstride % 8 == 0 && s_bstride >= 0 && t_bstride >= 0, "layersync_fwd: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)student | (uintptr_t)teacher | (uintptr_t)G) % 16 == 0, "layersync_fwd: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  const float inv_n = (float)(1.0 / (double)n);
  const dim3 grid((unsigned)cdiv64(n, LS_ROWS_PER_BLOCK)), block(LS_ROWS_PER_BLOCK * WAVE);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n * D, 6.0 * n * D);
#define LS_LAUNCH(NP_)                                                                                                                                  \
  hipLaunchKernelGGL(k_layersync_fwd<NP_>, grid, block, 0, (hipStream_t)stream, (const bf16*)student, (const bf16*)teacher, (bf16*)G, cos_rows, rows, D, n, ld, \
                     s_bstride, t_bstride, inv_n)
  switch ((D + LS_PASS_COLS - 1) / LS_PASS_COLS) {
    case 1: LS_LAUNCH(1); break;
    case 2: LS_LAUNCH(2); break;
    case 3: LS_LAUNCH(3); break;
    case 4: LS_LAUNCH(4); break;
    case 5: case 6: LS_LAUNCH(6); break;
    default: LS_LAUNCH(8); break;
  }
#undef LS_LAUNCH
  int rc = st355_check_launch("layersync_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(k_layersync_mean, dim3(1), dim3(LS_MEAN_THREADS), 0, (hipStream_t)stream, (const float*)cos_rows, sim, n, inv_n);
  return st355_check_launch("layersync_mean");
}

// dx[b, r, :] = bf16(float(dx) + scale_dev[0] * float(G)): product and sum are separate fp32 roundings, so the result is defined bit for bit.  (HIP's __fmul_rn /
// __fadd_rn are plain operators and contract like them; the pragma binds only under -ffp-contract=fast-honor-pragmas, which the Makefile sets for this file.)
#pragma clang fp contract(off)
__global__ void __launch_bounds__(256) k_layersync_inject(bf16* dx, const bf16* __restrict__ G, const float* __restrict__ scale_dev, int rows, int D, int64_t n_rows,
                                                          int64_t ld, int64_t bstride) {
  const float scale = scale_dev[0];
  const int nv = D >> 3;
  const int64_t total = n_rows * nv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / nv;
    const int c = (int)(i % nv) * 8;
    bf16* p = dx + (row / rows) * bstride + (row % rows) * ld + c;
    const bf16x8 d = *(const bf16x8*)p, g = *(const bf16x8*)(G + row * (int64_t)D + c);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float prod = scale * bf2f(g[j]);
      o[j] = f2bf(bf2f(d[j]) + prod);
    }
    *(bf16x8*)p = o;
  }
}
#pragma clang fp contract(fast)

extern "C" int st355_layersync_inject(void* stream, void* dx, const void* G, const float* scale_dev, int B, int rows, int D, int64_t ld, int64_t bstride) {
  ST_REQUIRE(dx && G && scale_dev && B > 0 && rows > 0 && D > 0, "layersync_inject: bad args");
  ST_REQUIRE(D % 8 == 0 && ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "layersync_inject: D, ld and the batch stride must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)dx | (uintptr_t)G) % 16 == 0, "layersync_inject: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows, total = n * (D / 8);
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 256 * 32) blocks = 256 * 32;                       // grid-stride above 32 blocks per CU
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * n * D, 6.0 * n * D);
  hipLaunchKernelGGL(k_layersync_inject, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (bf16*)dx, (const bf16*)G, scale_dev, rows, D, n, ld, bstride);
  return st355_check_launch("layersync_inject");
}

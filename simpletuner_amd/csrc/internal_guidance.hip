// internal_guidance.hip — the auxiliary head of Internal Guidance (helpers/training/internal_guidance.py): LayerNorm(D, eps 1e-6) -> Linear(D -> 64) on one block's
// image-token output.  All arithmetic fp32, bf16 only in memory, no atomics, every reduction in a fixed order (two calls give the same bits).
//   st355_ig_fold      W' = bf16(gamma * W) [64, D] and its transpose W'^T [D, 64], c = bf16(W beta + b) [64]: the operands of the projection y = xhat W'^T + c
//                      (the thin route of st355_gemm_bf16 on xhat; its bias operand is bf16, like every projection's here) and of the backward's g = dy W'.
//   st355_ig_head_fwd  one pass over the [B, rows, D] view of the block output, a row per wave kept in registers: mean, CENTRED variance, xhat (compact bf16), rstd.
//   st355_ig_head_bwd  dx += rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)), g = dy W' formed per 16-row tile on the MFMA (K = 64; W'^T staged in LDS per workgroup) and never written: the first
//                      walk over D takes the two row sums, the second forms g again (same operands, same bits) and adds into the dX view (fp32 sum, ONE bf16 rounding).
//   st355_ig_wgrad     from P = dy^T xhat [64, D] fp32 (st355_skinny_tn_seg) and db = sum_m dy: dW = P * gamma + db beta^T, and the LayerNorm affine's gradients by
//                      contracting with the UNFOLDED W instead of dividing g by gamma (gamma may be 0): sum_m dn * xhat = sum_n W[n, :] * P[n, :] and
//                      sum_m dn = sum_n W[n, :] * db[n] with dn = dy W — exact identities, so no per-block partial column sums leave the backward kernel.
#include "feature_common.h"

#define IG_N 64                       // output features of the head (16 latent channels x 2 x 2 patch)
#define IG_MAX_D (ROW_PASS_COLS * ROW_MAX_PASSES)          // the row pass keeps a row in registers: D <= 4096
#define IG_BWD_ROWS 16                // backward: token rows per wave (one MFMA tile); a workgroup's 4 waves share the staged W'^T chunk
#define IG_BWD_WAVES 4

// one block per output feature n: W'[n, :], W'^T[:, n] and c[n] = sum_d W[n, d] beta[d] + b[n] (thread-strided partials, butterfly per wave, the 4 wave sums in order)
template <typename T>
__global__ void __launch_bounds__(256) k_ig_fold(const T* __restrict__ gamma, const T* __restrict__ beta, const T* __restrict__ W, const T* __restrict__ b,
                                                 bf16* __restrict__ Wf, bf16* __restrict__ WfT, bf16* __restrict__ c, int D) {
  __shared__ float part[4];
  const int n = blockIdx.x;
  float a = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float w = ld(W, (int64_t)n * D + d);
    const bf16 f = f2bf(w * ld(gamma, d));
    Wf[(int64_t)n * D + d] = f;
    WfT[(int64_t)d * IG_N + n] = f;
    a = fmaf(w, ld(beta, d), a);
  }
  a = wave_sum(a);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) c[n] = f2bf(((part[0] + part[1]) + (part[2] + part[3])) + ld(b, n));
}

extern "C" int st355_ig_fold(void* stream, const void* gamma, const void* beta, const void* W, const void* b, int params_bf16, void* Wf, void* WfT, void* c, int N,
                             int D) {
  ST_REQUIRE(gamma && beta && W && b && Wf && WfT && c, "ig_fold: bad args");
  ST_REQUIRE(N == IG_N, "ig_fold: the head has %d output features (got %d)", IG_N, N);
  ST_REQUIRE(D > 0 && D % 8 == 0 && D <= IG_MAX_D, "ig_fold: D must be a multiple of 8, at most %d (got %d)", IG_MAX_D, D);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 3.0 * N * D, 8.0 * N * D);
  if (params_bf16)
    hipLaunchKernelGGL(k_ig_fold<bf16>, dim3(IG_N), dim3(256), 0, (hipStream_t)stream, (const bf16*)gamma, (const bf16*)beta, (const bf16*)W, (const bf16*)b, (bf16*)Wf,
                       (bf16*)WfT, (bf16*)c, D);
  else
    hipLaunchKernelGGL(k_ig_fold<float>, dim3(IG_N), dim3(256), 0, (hipStream_t)stream, (const float*)gamma, (const float*)beta, (const float*)W, (const float*)b,
                       (bf16*)Wf, (bf16*)WfT, (bf16*)c, D);
  return st355_check_launch("ig_fold");
}

// the row pass: k_rows_fwd of feature_common.h with the head's eps 1e-6
extern "C" int st355_ig_head_fwd(void* stream, const void* h, void* xhat, float* rstd, int B, int rows, int D, int64_t ld, int64_t bstride) {
  ST_REQUIRE(h && xhat && rstd && B > 0 && rows > 0 && D > 0, "ig_head_fwd: bad args");
  ST_REQUIRE(D % 8 == 0 && D <= IG_MAX_D, "ig_head_fwd: D must be a multiple of 8, at most %d (got %d)", IG_MAX_D, D);
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "ig_head_fwd: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)h | (uintptr_t)xhat) % 16 == 0, "ig_head_fwd: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * n * D, 4.0 * n * D);
  rows_fwd_launch<RowEps1e6>((hipStream_t)stream, (const bf16*)h, (bf16*)xhat, rstd, rows, D, n, ld, bstride);
  return st355_check_launch("ig_head_fwd");
}

// A workgroup is 4 waves of 16 token rows each (64 rows) and walks D in 64-column chunks.  The chunk's 64 rows of W'^T (8 KB) are staged ONCE per workgroup in LDS
// and shared by its waves (double-buffered: the next chunk's global loads fly under this chunk's MFMAs, one barrier per chunk).  Per chunk and wave: four 16x16
// tiles of g^T = W'^T dy^T on v_mfma_f32_16x16x32_bf16 (A = 16 rows of W'^T from LDS, B = dy^T of the 16 token rows, in registers; K = 64 = two steps).  The MFMA
// result has its column (the token row) on lane & 15 and rows 4 * (lane >> 4) + r in registers r = 0..3.  Tile t's A row 4 a + b is W'^T row d0 + 16 a + 4 t + b, so
// that lane (q, token) ends up with the 16 CONSECUTIVE columns d0 + 16 q .. + 15 of its token row in acc[t][r] (t-major): xhat and dx are touched as two 16-byte
// accesses per lane, 128 contiguous bytes per row and wave.  LDS image: chunk row 16 a + 4 t + b sits in slot 16 t + 4 a + b (the 16 rows one 16-lane group reads
// together are consecutive slots), slot pitch 144 B: 36 dwords, so the 16 slots' 16-byte reads fall on 16 disjoint 4-bank windows of the 64 banks.
// D % 8 == 0: a lane's 16 columns are valid in halves of 8; rows of W'^T at or past D are staged as zero.  Two walks: the first takes the two row sums, the second
// forms g again (same operands, same bits) and adds into dx.
#define IG_LDS_PITCH 72               // bf16 elements per slot (144 B)

__global__ void __launch_bounds__(IG_BWD_WAVES* WAVE) k_ig_head_bwd(const bf16* __restrict__ xhat, const float* __restrict__ rstd, const bf16* __restrict__ dy,
                                                                    const bf16* __restrict__ WfT, bf16* dx, int rows, int D, int64_t n_rows, int64_t ld,
                                                                    int64_t bstride, float inv_d) {
  __shared__ __attribute__((aligned(16))) bf16 Ws[2][64 * IG_LDS_PITCH];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), tr = lane & 15, q = lane >> 4;
  const int64_t row = ((int64_t)blockIdx.x * IG_BWD_WAVES + (tid >> 6)) * IG_BWD_ROWS + tr;
  const bool live = row < n_rows;                                 // dead token lanes (and whole dead waves of the last workgroup) still stage and meet the barriers
  bf16x8 bfr[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (live) bfr[s] = *(const bf16x8*)(dy + row * IG_N + 32 * s + 8 * q);
    else {
#pragma unroll
      for (int j = 0; j < 8; j++) bfr[s][j] = f2bf(0.f);
    }
  }
  const int nc = (D + 63) >> 6;
  bf16x8 stg[2];
  auto gload = [&](int ch) {                                      // 64 rows x 8 sixteen-byte pieces over 256 threads
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int p = tid + 256 * k, d = ch * 64 + (p >> 3);
      if (d < D) stg[k] = *(const bf16x8*)(WfT + (int64_t)d * IG_N + (p & 7) * 8);
      else {
#pragma unroll
        for (int j = 0; j < 8; j++) stg[k][j] = f2bf(0.f);
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int p = tid + 256 * k, r = p >> 3;
      const int slot = 16 * ((r >> 2) & 3) + 4 * (r >> 4) + (r & 3);
      *(bf16x8*)(&Ws[buf][slot * IG_LDS_PITCH + (p & 7) * 8]) = stg[k];
    }
  };
  const bf16* xp = xhat + (live ? row : 0) * (int64_t)D;
  bf16* dp = dx + (live ? (row / rows) * bstride + (row % rows) * ld : 0);
  const float rs = live ? rstd[row] : 0.f;
  float s1 = 0.f, s2 = 0.f, m1 = 0.f, m2 = 0.f;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int it = 0; it < 2 * nc; it++) {
    const int ch = it < nc ? it : it - nc, buf = it & 1, d0 = ch * 64;
    if (it + 1 < 2 * nc) gload(it + 1 < nc ? it + 1 : it + 1 - nc);
    if (it == nc) {                                               // between the walks: the four lanes that share a token row, xor butterfly, the same bits in all four
      s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
      m1 = s1 * inv_d; m2 = s2 * inv_d;
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const bf16* ap = &Ws[buf][(16 * t + tr) * IG_LDS_PITCH + 8 * q];
      const bf16x8 a0 = *(const bf16x8*)ap, a1 = *(const bf16x8*)(ap + 32);
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bfr[0], z, 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bfr[1], z, 0, 0, 0);
    }
    if (live) {
#pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        const int c = d0 + 16 * q + 8 * hf;
        if (c < D) {
          const bf16x8 x = *(const bf16x8*)(xp + c);
          if (it < nc) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const float g = acc[2 * hf + (j >> 2)][j & 3];
              s1 += g;
              s2 = fmaf(g, bf2f(x[j]), s2);
            }
          } else {
            const bf16x8 o = *(const bf16x8*)(dp + c);
            bf16x8 w;
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const float g = acc[2 * hf + (j >> 2)][j & 3];
              const float dh = rs * ((g - m1) - bf2f(x[j]) * m2);
              w[j] = f2bf(bf2f(o[j]) + dh);
            }
            *(bf16x8*)(dp + c) = w;
          }
        }
      }
    }
    if (it + 1 < 2 * nc) sstore(buf ^ 1);                          // (its last readers passed the barrier that ended the previous chunk)
    __syncthreads();
  }
}

extern "C" int st355_ig_head_bwd(void* stream, const void* xhat, const float* rstd, const void* dy, const void* WfT, void* dx, int B, int rows, int D, int N,
                                 int64_t ld, int64_t bstride) {
  ST_REQUIRE(xhat && rstd && dy && WfT && dx && B > 0 && rows > 0 && D > 0, "ig_head_bwd: bad args");
  ST_REQUIRE(N == IG_N, "ig_head_bwd: the head has %d output features (got %d)", IG_N, N);
  ST_REQUIRE(D % 8 == 0 && D <= IG_MAX_D, "ig_head_bwd: D must be a multiple of 8, at most %d (got %d)", IG_MAX_D, D);
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "ig_head_bwd: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)xhat | (uintptr_t)dy | (uintptr_t)WfT | (uintptr_t)dx) % 16 == 0, "ig_head_bwd: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  const dim3 grid((unsigned)cdiv64(n, IG_BWD_ROWS * IG_BWD_WAVES)), block(IG_BWD_WAVES * WAVE);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 4.0 * n * D * IG_N, 6.0 * n * D);
  hipLaunchKernelGGL(k_ig_head_bwd, grid, block, 0, (hipStream_t)stream, (const bf16*)xhat, rstd, (const bf16*)dy, (const bf16*)WfT, (bf16*)dx, rows, D, n, ld, bstride,
                     (float)(1.0 / (double)D));
  return st355_check_launch("ig_head_bwd");
}

// tiled over (n, d): a workgroup owns 32 columns, thread (ng, col) walks the 8 features 8 ng .. 8 ng + 7 of its column (dW[n, d] on the way) and the 8 groups'
// partial sums of d gamma / d beta meet in LDS, added in group order; thread n of workgroup 0 also writes d b[n] = db[n]
#define IG_WG_COLS 32
template <typename T>
__global__ void __launch_bounds__(256) k_ig_wgrad(const float* __restrict__ P, const float* __restrict__ db, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                  const T* __restrict__ W, T* g_gamma, T* g_beta, T* g_W, T* g_b, int D, int accumulate) {
  __shared__ float sg[8][IG_WG_COLS], sb[8][IG_WG_COLS];
  const int col = threadIdx.x & (IG_WG_COLS - 1), ng = threadIdx.x >> 5;
  const int d = blockIdx.x * IG_WG_COLS + col;
  if (blockIdx.x == 0 && threadIdx.x < IG_N) st(g_b, threadIdx.x, db[threadIdx.x], accumulate);
  float dg = 0.f, dbe = 0.f;
  if (d < D) {
    const float ga = ld(gamma, d), be = ld(beta, d);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int n = ng * 8 + i;
      const float p = P[(int64_t)n * D + d], w = ld(W, (int64_t)n * D + d), s = db[n];
      st(g_W, (int64_t)n * D + d, fmaf(p, ga, s * be), accumulate);
      dg = fmaf(w, p, dg);
      dbe = fmaf(w, s, dbe);
    }
  }
  sg[ng][col] = dg; sb[ng][col] = dbe;
  __syncthreads();
  if (ng == 0 && d < D) {
    float a = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++) { a += sg[k][col]; c += sb[k][col]; }
    st(g_gamma, d, a, accumulate);
    st(g_beta, d, c, accumulate);
  }
}

extern "C" int st355_ig_wgrad(void* stream, const float* P, const float* db, const void* gamma, const void* beta, const void* W, int params_bf16, void* g_gamma,
                              void* g_beta, void* g_W, void* g_b, int N, int D, int accumulate) {
  ST_REQUIRE(P && db && gamma && beta && W && g_gamma && g_beta && g_W && g_b, "ig_wgrad: bad args");
  ST_REQUIRE(N == IG_N, "ig_wgrad: the head has %d output features (got %d)", IG_N, N);
  ST_REQUIRE(D > 0 && D % 8 == 0 && D <= IG_MAX_D, "ig_wgrad: D must be a multiple of 8, at most %d (got %d)", IG_MAX_D, D);
  const dim3 grid((unsigned)((D + IG_WG_COLS - 1) / IG_WG_COLS)), block(256);
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * N * D, 12.0 * N * D);
  if (params_bf16)
    hipLaunchKernelGGL(k_ig_wgrad<bf16>, grid, block, 0, (hipStream_t)stream, P, db, (const bf16*)gamma, (const bf16*)beta, (const bf16*)W, (bf16*)g_gamma,
                       (bf16*)g_beta, (bf16*)g_W, (bf16*)g_b, D, accumulate);
  else
    hipLaunchKernelGGL(k_ig_wgrad<float>, grid, block, 0, (hipStream_t)stream, P, db, (const float*)gamma, (const float*)beta, (const float*)W, (float*)g_gamma,
                       (float*)g_beta, (float*)g_W, (float*)g_b, D, accumulate);
  return st355_check_launch("ig_wgrad");
}

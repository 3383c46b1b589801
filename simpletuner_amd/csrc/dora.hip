// dora.hip — DoRA (Liu et al. 2024, "DoRA: Weight-Decomposed Low-Rank Adaptation"; peft `use_dora`) of the Linears of one LoraGroup:
//   V = W + s B A,  norm_n = ||V[n, :]||_2 (detached),  g_n = m_n / norm_n,  y = g . (x W^T + s (x A^T) B^T) + b.
// The row scale is folded into the GEMM operands once per forward, so the GEMM routes and their epilogues run unchanged on W' = bf16(g . W) and
// B_blk' = bf16(g . B_blk) (B_blk already carries s).  All arithmetic fp32, bf16 only in memory, no atomics, every reduction in a fixed order (two calls give the
// same bits).  Here:
//   st355_dora_fold       one launch per group.  A workgroup owns 32 output rows of ONE target.  Pass 1: the B A tile of every 32-column chunk on the MFMA from the
//                         packed bf16 operands the forward multiplies with (B_blk's slab of the target, A_cat^T), W added in fp32, the squares summed per row: wave w
//                         takes chunks w, w + 4, ..., then the 32 columns of a lane group by xor butterfly, then the four waves in index order.  Pass 2 (W is read
//                         a second time: the scale is only known after the reduction): W' and B_blk' straight (16-byte stores) and transposed through LDS (the
//                         32 lanes of a half-wave write 64 contiguous bytes of a row of the transpose).  `init` writes m = norm instead of reading m.
//   st355_dora_dmag       dm[n] (+)= inv_norm[n] sum_rows dy[row, n] y0[row, n]: per 256-row chunk partial column sums into a workspace, then the chunks in order.
//   st355_dora_db_finish  gB[n, :] (+)= g[n] P[n, :] (P = s dy^T T, the unscaled product of st355_skinny_tn_seg): the row scale a scalar alpha cannot give.
#include "common.h"

#define DR_ROWS 32                 // output rows per workgroup of the fold
#define DR_CHUNK 64                // columns per pass-2 tile
#define DR_TP (DR_ROWS + 2)        // LDS pitch of the transposed tile (elements): 17 dwords, the 64 rows of a tile start on different banks
#define DR_MC 256                  // dmag: rows per chunk
#define DR_MCOLS 64                // dmag: columns per workgroup

struct DoraTargets {
  int n_off[4], n_cnt[4], tile0[5];          // tile0[g]: first workgroup of target g, tile0[G]: the grid
};

// element offset of logical row m: compact (seg_rows == 0), or segment m / seg_rows at seg_stride ROWS from the previous one
__device__ __forceinline__ int64_t dr_row_off(uint32_t m, int64_t ld, uint32_t seg_rows, int64_t seg_stride) {
  if (seg_rows == 0) return (int64_t)m * ld;
  const uint32_t s = m / seg_rows;
  return ((int64_t)s * seg_stride + (int64_t)(m - s * seg_rows)) * ld;
}

// pass 2 of the fold for one source matrix src [*, C] (C % 8 == 0): out = bf16(gs[row] * src) straight and transposed (outT [C, N_total])
__device__ __forceinline__ void dr_scale_store(const bf16* __restrict__ src, bf16* __restrict__ out, bf16* __restrict__ outT, int C, int N_total, int rowbase,
                                               int nrows, const float* gs, bf16* tT) {
  const int tid = threadIdx.x;
  for (int c0 = 0; c0 < C; c0 += DR_CHUNK) {
    {
      const int row = tid >> 3, ch = tid & 7, col = c0 + 8 * ch;
      if (row < nrows && col < C) {
        const int64_t o = (int64_t)(rowbase + row) * C + col;
        const bf16x8 v = *(const bf16x8*)(src + o);
        const float s = gs[row];
        bf16x8 w;
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = f2bf(s * bf2f(v[j]));
        *(bf16x8*)(out + o) = w;
#pragma unroll
        for (int j = 0; j < 8; j++) tT[(8 * ch + j) * DR_TP + row] = w[j];
      }
    }
    __syncthreads();
    {
      const int n = tid & 31, kq = tid >> 5;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int kk = 8 * kq + i, col = c0 + kk;
        if (n < nrows && col < C) outT[(int64_t)col * N_total + rowbase + n] = tT[kk * DR_TP + n];
      }
    }
    __syncthreads();
  }
}

template <int NK>          // 16-deep MFMA steps over the target's slab (r_pad / 16)
__global__ void __launch_bounds__(256) k_dora_fold(const bf16* __restrict__ W, const bf16* __restrict__ At, const bf16* __restrict__ Bb, float* m, int init,
                                                  float* __restrict__ inv_norm, float* __restrict__ gout, bf16* __restrict__ Wf, bf16* __restrict__ WfT,
                                                  bf16* __restrict__ Bf, bf16* __restrict__ BfT, int N_total, int K, int K2, int G, DoraTargets t) {
  __shared__ float part[4][DR_ROWS];
  __shared__ float gs[DR_ROWS];
  __shared__ bf16 tT[DR_CHUNK * DR_TP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  int g = 0;
  while (g + 1 < G && (int)blockIdx.x >= t.tile0[g + 1]) g++;
  const int rowbase = t.n_off[g] + ((int)blockIdx.x - t.tile0[g]) * DR_ROWS;
  const int nrows = min(DR_ROWS, t.n_off[g] + t.n_cnt[g] - rowbase);
  const int slab = g * (16 * NK);
  // ---- pass 1: sum_k (W + B A)^2 per row ----
  u32x4 bfrag[NK];
#pragma unroll
  for (int ks = 0; ks < NK; ks++) {
    bfrag[ks] = u32x4{0u, 0u, 0u, 0u};
    if (r < nrows) bfrag[ks] = *(const u32x4*)(Bb + (int64_t)(rowbase + r) * K2 + slab + 16 * ks + 8 * h);
  }
  float sq[16];
#pragma unroll
  for (int i = 0; i < 16; i++) sq[i] = 0.f;
  const int nchunks = (K + 31) / 32;
  for (int c = wv; c < nchunks; c += 4) {
    const int k = 32 * c + r;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < NK; ks++) {
      u32x4 av = {0u, 0u, 0u, 0u};
      if (k < K) av = *(const u32x4*)(At + (int64_t)k * K2 + slab + 16 * ks + 8 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8*)&bfrag[ks], *(bf16x8*)&av, acc, 0, 0, 0);
    }
    // D[i = row n][j = column k]: lane -> column lane & 31, register reg -> row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int n = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (n < nrows && k < K) {
        const float v = acc[reg] + bf2f(W[(int64_t)(rowbase + n) * K + k]);
        sq[reg] = fmaf(v, v, sq[reg]);
      }
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    float v = sq[reg];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // the 32 columns of this lane group
    if (r == 0) part[wv][(reg & 3) + 8 * (reg >> 2) + 4 * h] = v;
  }
  __syncthreads();
  if (tid < DR_ROWS) {
    float gv = 0.f;
    if (tid < nrows) {
      const float s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
      const float norm = sqrtf(s);
      const int n = rowbase + tid;
      float mv;
      if (init) {
        mv = norm;
        m[n] = norm;
      } else {
        mv = m[n];
      }
      gv = mv / norm;
      inv_norm[n] = 1.f / norm;
      gout[n] = gv;
    }
    gs[tid] = gv;
  }
  __syncthreads();
  // ---- pass 2: the scaled operands, straight and transposed ----
  dr_scale_store(W, Wf, WfT, K, N_total, rowbase, nrows, gs, tT);
  dr_scale_store(Bb, Bf, BfT, K2, N_total, rowbase, nrows, gs, tT);
}

extern "C" int st355_dora_fold(void* stream, const void* W, const void* A_cat_T, const void* B_blk, float* m, int init, float* inv_norm, float* g, void* Wf,
                               void* WfT, void* Bf, void* BfT, int N_total, int K, int K2, int G, const int* n_off, const int* n_cnt, int r_pad) {
  ST_REQUIRE(W && A_cat_T && B_blk && m && inv_norm && g && Wf && WfT && Bf && BfT && n_off && n_cnt, "dora_fold: bad args");
  ST_REQUIRE(N_total > 0 && K > 0 && K % 8 == 0, "dora_fold: K must be a positive multiple of 8 (got K = %d, N = %d)", K, N_total);
  ST_REQUIRE(G >= 1 && G <= 4, "dora_fold: 1 .. 4 targets per group (got %d)", G);
  ST_REQUIRE(r_pad == 32 || r_pad == 64 || r_pad == 128, "dora_fold: r_pad must be 32, 64 or 128 (got %d)", r_pad);
  ST_REQUIRE(K2 > 0 && K2 % 64 == 0 && G * r_pad <= K2, "dora_fold: K2 must be a multiple of 64 that holds the targets' slabs (got K2 = %d, %d targets, r_pad %d)", K2,
             G, r_pad);
  ST_REQUIRE(((uintptr_t)W | (uintptr_t)A_cat_T | (uintptr_t)B_blk | (uintptr_t)Wf | (uintptr_t)Bf) % 16 == 0, "dora_fold: operands must be 16-byte aligned");
  ST_REQUIRE((int64_t)N_total * (K > K2 ? K : K2) < ((int64_t)1 << 40), "dora_fold: operand too large");
  DoraTargets t;
  memset(&t, 0, sizeof(t));
  int tiles = 0, end = 0;
  for (int i = 0; i < G; i++) {
    ST_REQUIRE(n_cnt[i] > 0 && n_off[i] >= end && n_off[i] + n_cnt[i] <= N_total, "dora_fold: target %d (rows %d .. %d) must follow the one before inside N = %d", i,
               n_off[i], n_off[i] + n_cnt[i], N_total);
    end = n_off[i] + n_cnt[i];
    t.n_off[i] = n_off[i];
    t.n_cnt[i] = n_cnt[i];
    t.tile0[i] = tiles;
    tiles += (n_cnt[i] + DR_ROWS - 1) / DR_ROWS;
  }
  for (int i = G; i <= 4; i++) t.tile0[i] = tiles;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * N_total * (double)K * r_pad + 4.0 * N_total * (double)K,
               2.0 * N_total * (3.0 * K + 3.0 * K2) + 2.0 * (double)K * K2);
  const hipStream_t st = (hipStream_t)stream;
#define DR_LAUNCH(NK)                                                                                                                                           \
  hipLaunchKernelGGL(k_dora_fold<NK>, dim3(tiles), dim3(256), 0, st, (const bf16*)W, (const bf16*)A_cat_T, (const bf16*)B_blk, m, init, inv_norm, g, (bf16*)Wf, \
                     (bf16*)WfT, (bf16*)Bf, (bf16*)BfT, N_total, K, K2, G, t)
  if (r_pad == 32) DR_LAUNCH(2);
  else if (r_pad == 64) DR_LAUNCH(4);
  else DR_LAUNCH(8);
#undef DR_LAUNCH
  return st355_check_launch("dora_fold");
}

// ---- dm ----
__global__ void __launch_bounds__(256) k_dora_dmag_part(const bf16* __restrict__ dy, int64_t ldd, uint32_t seg_rows, int64_t seg_stride,
                                                       const bf16* __restrict__ y0, int64_t ldy, float* __restrict__ ws, uint32_t M, int N) {
  __shared__ float red[32][DR_MCOLS];
  const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
  const int col = blockIdx.x * DR_MCOLS + 8 * cg;
  const uint32_t m0 = blockIdx.y * (uint32_t)DR_MC, m1 = min(M, m0 + (uint32_t)DR_MC);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = 0.f;
  if (col < N)                                                    // N % 8 == 0: a chunk lies wholly inside or outside
    for (uint32_t mm = m0 + rl; mm < m1; mm += 32) {
      const bf16x8 a = *(const bf16x8*)(dy + dr_row_off(mm, ldd, seg_rows, seg_stride) + col);
      const bf16x8 b = *(const bf16x8*)(y0 + (int64_t)mm * ldy + col);
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = fmaf(bf2f(a[j]), bf2f(b[j]), acc[j]);
    }
#pragma unroll
  for (int j = 0; j < 8; j++) red[rl][8 * cg + j] = acc[j];
  __syncthreads();
  if (tid < DR_MCOLS) {
    const int c = blockIdx.x * DR_MCOLS + tid;
    if (c < N) {
      float s = 0.f;
      for (int i = 0; i < 32; i++) s += red[i][tid];
      ws[(int64_t)blockIdx.y * N + c] = s;
    }
  }
}

__global__ void __launch_bounds__(256) k_dora_dmag_final(const float* __restrict__ ws, const float* __restrict__ inv_norm, float* dm, int N, int nchunks,
                                                        int accumulate) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int c = 0; c < nchunks; c++) s += ws[(int64_t)c * N + n];
  const float v = inv_norm[n] * s;
  dm[n] = accumulate ? dm[n] + v : v;
}

extern "C" int64_t st355_dora_dmag_workspace(int64_t M, int N) { return (M > 0 && N > 0) ? cdiv64(M, DR_MC) * (int64_t)N * 4 : 0; }

extern "C" int st355_dora_dmag(void* stream, const void* dy, int64_t ldd, int64_t seg_rows, int64_t seg_stride, const void* y0, int64_t ldy, const float* inv_norm,
                               float* dm, int64_t M, int N, int accumulate, void* workspace) {
  ST_REQUIRE(dy && y0 && inv_norm && dm && workspace && M > 0 && N > 0, "dora_dmag: bad args");
  ST_REQUIRE(N % 8 == 0 && ldd % 8 == 0 && ldy % 8 == 0 && ldd >= N && ldy >= N, "dora_dmag: N and the row strides must be multiples of 8 (got N = %d)", N);
  ST_REQUIRE(((uintptr_t)dy | (uintptr_t)y0) % 16 == 0 && (uintptr_t)workspace % 4 == 0, "dora_dmag: operands must be 16-byte aligned");
  ST_REQUIRE(M < ((int64_t)1 << 31), "dora_dmag: too many rows");
  ST_REQUIRE(seg_rows >= 0 && (seg_rows == 0 || (M % seg_rows == 0 && seg_stride >= seg_rows)), "dora_dmag: seg_rows must divide M, seg_stride >= seg_rows");
  const int nchunks = (int)cdiv64(M, DR_MC);
  ST_REQUIRE(nchunks <= 65535, "dora_dmag: too many rows for one launch");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * M * (double)N, 4.0 * M * (double)N);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_dora_dmag_part, dim3((N + DR_MCOLS - 1) / DR_MCOLS, nchunks), dim3(256), 0, st, (const bf16*)dy, ldd, (uint32_t)seg_rows, seg_stride,
                     (const bf16*)y0, ldy, (float*)workspace, (uint32_t)M, N);
  hipLaunchKernelGGL(k_dora_dmag_final, dim3((N + 255) / 256), dim3(256), 0, st, (const float*)workspace, inv_norm, dm, N, nchunks, accumulate);
  return st355_check_launch("dora_dmag");
}

// ---- dB ----
__global__ void __launch_bounds__(256) k_dora_db_finish(const float* __restrict__ P, const float* __restrict__ g, float* gB, int64_t total, int rank, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float v = g[i / rank] * P[i];
  gB[i] = accumulate ? gB[i] + v : v;
}

extern "C" int st355_dora_db_finish(void* stream, const float* P, const float* g, float* gB, int N, int rank, int accumulate) {
  ST_REQUIRE(P && g && gB && N > 0 && rank > 0, "dora_db_finish: bad args");
  const int64_t total = (int64_t)N * rank;
  ST_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "dora_db_finish: too many elements");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * total, 12.0 * total);
  hipLaunchKernelGGL(k_dora_db_finish, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, P, g, gB, total, rank, accumulate);
  return st355_check_launch("dora_db_finish");
}

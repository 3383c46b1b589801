// lokr.hip — LyCORIS LoKr (Kronecker-product adapter, `algo: lokr`, both factors full) of the Linears of one LokrGroup:
//   dW = s kron(w1, w2),  dW[i ok + k, j in + l] = s w1[i, j] w2[k, l],  y = x bf16(W + dW)^T + b   (the merged-weight forward, LyCORIS' default).
// The delta is folded into the GEMM operands once per forward, so every GEMM route and epilogue runs unchanged on the folded copies.  The gradients use the
// Kronecker structure and never form a [N, K] weight gradient:
//   dP[m, j, k] = sum_i w1[i, j] dy[m, i, k]                (st355_lokr_mix)
//   dw2 = s dP.view(M im, ok)^T x.view(M im, in)            (st355_lokr_dw2)
//   P = x.view(M im, in) w2^T                               (the GEMM route, not here)
//   dw1[i, j] = s sum_{m, k} dy[m, i, k] P[m, j, k]         (st355_lokr_dw1)
// All arithmetic fp32, bf16 only in memory, no atomics, every reduction in two stages in a fixed order (two calls give the same bits).  Here:
//   st355_lokr_fold   one launch per fused projection.  A workgroup owns a 32-row x 64-column tile of W: Wf straight (16-byte stores) and WfT through LDS (the 32
//                     lanes of a half-wave write 64 contiguous bytes of a row of the transpose).  Rows outside every target are copied.  Workgroups behind the tile
//                     grid write the bf16 copy of every w2.
//   st355_lokr_mix    streaming: a lane owns 8 consecutive k of one row m, reads the ol 16-byte pieces of dy once per group of 4 output factors j and writes im
//                     16-byte pieces of dP.
//   st355_lokr_dw2    TN product with a tiny output and a long contraction on v_mfma_f32_32x32x16_bf16: a workgroup owns a 64 x 64 output tile (128 x 128 where both
//                     sides are multiples of 128) and one slice of the contraction; 64-row chunks of both operands are staged in LDS as they lie in memory and
//                     read as MFMA fragments by the transposing LDS read (the global loads of the next chunk fly under the MFMAs); fp32 partial tiles go to the
//                     workspace, a second kernel adds the slices in order (eight running sums) and applies alpha / accumulate.
//   st355_lokr_dw1    both operands k-contiguous: a lane's fragment of v_mfma_f32_16x16x32_bf16 is one 16-byte load (rows i >= ol / j >= im zero), one fp32
//                     16 x 16 tile per wave over a slice of m (four loads in flight), the four waves of a workgroup added in order, then the fixed-order reduce.
#include "common.h"

#define LK_ROWS 32                 // fold: rows per tile
#define LK_CHUNK 64                // fold: columns per tile
#define LK_TP (LK_ROWS + 2)        // fold: LDS pitch of the transposed tile (elements)
// (dw2: LDS pitches of a staged 64-row chunk = 64 B (mod 128 B), as skinny.hip's: the four tile rows a transposing read touches sit in disjoint bank windows)
#define LK_DW2_WGS 1024            // dw2: workgroups aimed at (tiles x slices)
#define LK_DW1_WAVES 4096          // dw1: waves at most (16 per CU)

struct LokrFold {
  const float* w1[4];
  const float* w2[4];
  bf16* w2b[4];
  int n_off[4], n_cnt[4], ol[4], im[4];
  int cvt0[5];                     // first conversion workgroup of target g behind the tile grid; cvt0[G]: their count
};

// element offset of logical row m: compact (seg_rows == 0), or segment m / seg_rows at seg_stride ROWS from the previous one
__device__ __forceinline__ int64_t lk_row_off(uint32_t m, int64_t ld, uint32_t seg_rows, int64_t seg_stride) {
  if (seg_rows == 0) return (int64_t)m * ld;
  const uint32_t s = m / seg_rows;
  return ((int64_t)s * seg_stride + (int64_t)(m - s * seg_rows)) * ld;
}

__global__ void __launch_bounds__(256) k_lokr_fold(const bf16* __restrict__ W, bf16* __restrict__ Wf, bf16* __restrict__ WfT, int N_total, int K, int G, int ntiles,
                                                  int nct, float s, LokrFold t) {
  __shared__ bf16 tT[LK_CHUNK * LK_TP];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= ntiles) {          // the bf16 copy of w2 (the B operand of the backward's P GEMM)
    const int c = (int)blockIdx.x - ntiles;
    int g = 0;
    while (g + 1 < G && c >= t.cvt0[g + 1]) g++;
    const int ok = t.n_cnt[g] / t.ol[g], in_ = K / t.im[g];
    const int64_t idx = (int64_t)(c - t.cvt0[g]) * 256 + tid;
    if (idx < (int64_t)ok * in_) t.w2b[g][idx] = f2bf(t.w2[g][idx]);
    return;
  }
  const int rt = (int)blockIdx.x / nct, ct = (int)blockIdx.x - rt * nct;
  const int rowbase = rt * LK_ROWS, c0 = ct * LK_CHUNK;
  {
    const int row = tid >> 3, ch = tid & 7, n = rowbase + row, col = c0 + 8 * ch;
    if (n < N_total && col < K) {           // K % 8 == 0: a chunk lies wholly inside or outside
      const int64_t o = (int64_t)n * K + col;
      bf16x8 w = *(const bf16x8*)(W + o);
      int g = -1;
      for (int q = 0; q < G; q++)
        if (n >= t.n_off[q] && n < t.n_off[q] + t.n_cnt[q]) g = q;
      if (g >= 0) {
        const int ok = t.n_cnt[g] / t.ol[g], in_ = K / t.im[g];
        const int r = n - t.n_off[g], i = r / ok, k = r - i * ok;
        const int j = col / in_, l = col - j * in_;          // in_ % 8 == 0: the 8 columns share j
        const float a = s * t.w1[g][i * t.im[g] + j];
        const float* w2p = t.w2[g] + (int64_t)k * in_ + l;
#pragma unroll
        for (int e = 0; e < 8; e++) w[e] = f2bf(fmaf(a, w2p[e], bf2f(w[e])));
      }
      *(bf16x8*)(Wf + o) = w;
#pragma unroll
      for (int e = 0; e < 8; e++) tT[(8 * ch + e) * LK_TP + row] = w[e];
    }
  }
  __syncthreads();
  {
    const int n = tid & 31, kq = tid >> 5;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int kk = 8 * kq + i, col = c0 + kk;
      if (rowbase + n < N_total && col < K) WfT[(int64_t)col * N_total + rowbase + n] = tT[kk * LK_TP + n];
    }
  }
}

extern "C" int st355_lokr_fold(void* stream, const void* W, void* Wf, void* WfT, int N_total, int K, int G, const int* n_off, const int* n_cnt, const int* ol,
                               const int* im, const float* const* w1, const float* const* w2, void* const* w2b, float s) {
  ST_REQUIRE(W && Wf && WfT && n_off && n_cnt && ol && im && w1 && w2 && w2b, "lokr_fold: bad args");
  ST_REQUIRE(N_total > 0 && K > 0 && K % 8 == 0, "lokr_fold: K must be a positive multiple of 8 (got K = %d, N = %d)", K, N_total);
  ST_REQUIRE(G >= 1 && G <= 4, "lokr_fold: 1 .. 4 targets per projection (got %d)", G);
  ST_REQUIRE(((uintptr_t)W | (uintptr_t)Wf) % 16 == 0, "lokr_fold: W and Wf must be 16-byte aligned");
  ST_REQUIRE((int64_t)N_total * K < ((int64_t)1 << 40), "lokr_fold: operand too large");
  LokrFold t;
  memset(&t, 0, sizeof(t));
  int end = 0, cvt = 0;
  for (int g = 0; g < G; g++) {
    ST_REQUIRE(n_cnt[g] > 0 && n_off[g] >= end && n_off[g] + n_cnt[g] <= N_total, "lokr_fold: target %d (rows %d .. %d) must follow the one before inside N = %d", g,
               n_off[g], n_off[g] + n_cnt[g], N_total);
    end = n_off[g] + n_cnt[g];
    ST_REQUIRE(w1[g] && w2[g] && w2b[g], "lokr_fold: target %d: null factor pointer", g);
    ST_REQUIRE(ol[g] >= 1 && ol[g] <= 16 && im[g] >= 1 && im[g] <= 16, "lokr_fold: the w1 sides must lie in 1 .. 16 (target %d: ol = %d, im = %d)", g, ol[g], im[g]);
    ST_REQUIRE(n_cnt[g] % ol[g] == 0 && K % im[g] == 0, "lokr_fold: ol must divide the target's rows and im must divide K (target %d)", g);
    ST_REQUIRE((n_cnt[g] / ol[g]) % 8 == 0 && (K / im[g]) % 8 == 0, "lokr_fold: ok and in must be multiples of 8 (target %d: ok = %d, in = %d)", g, n_cnt[g] / ol[g],
               K / im[g]);
    t.w1[g] = w1[g];
    t.w2[g] = w2[g];
    t.w2b[g] = (bf16*)w2b[g];
    t.n_off[g] = n_off[g];
    t.n_cnt[g] = n_cnt[g];
    t.ol[g] = ol[g];
    t.im[g] = im[g];
    t.cvt0[g] = cvt;
    cvt += (int)cdiv64((int64_t)(n_cnt[g] / ol[g]) * (K / im[g]), 256);
  }
  for (int g = G; g <= 4; g++) t.cvt0[g] = cvt;
  const int nct = (K + LK_CHUNK - 1) / LK_CHUNK;
  const int64_t ntiles = cdiv64(N_total, LK_ROWS) * nct;
  ST_REQUIRE(ntiles + cvt <= 0x7fffffff, "lokr_fold: grid too large");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * N_total * (double)K, 6.0 * N_total * (double)K);
  hipLaunchKernelGGL(k_lokr_fold, dim3((unsigned)(ntiles + cvt)), dim3(256), 0, (hipStream_t)stream, (const bf16*)W, (bf16*)Wf, (bf16*)WfT, N_total, K, G, (int)ntiles,
                     nct, s, t);
  return st355_check_launch("lokr_fold");
}

// ---- dP = the mix over the output factor ----
__global__ void __launch_bounds__(256) k_lokr_mix(const bf16* __restrict__ dy, int64_t ldd, uint32_t seg_rows, int64_t seg_stride, int n_off,
                                                 const float* __restrict__ w1, int ol, int im, int ok, bf16* __restrict__ dP, int64_t total) {
  __shared__ float w1s[256];
  const int tid = threadIdx.x;
  if (tid < ol * im) w1s[tid] = w1[tid];
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
  if (idx >= total) return;
  const int okc = ok >> 3;
  const uint32_t m = (uint32_t)(idx / okc);
  const int kc = (int)(idx - (int64_t)m * okc);
  const bf16* src = dy + lk_row_off(m, ldd, seg_rows, seg_stride) + n_off + 8 * kc;
  bf16* dst = dP + (int64_t)m * im * ok + 8 * kc;
  for (int j0 = 0; j0 < im; j0 += 4) {
    float acc[4][8];
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
#pragma unroll
      for (int e = 0; e < 8; e++) acc[jj][e] = 0.f;
    for (int i = 0; i < ol; i++) {
      const bf16x8 v = *(const bf16x8*)(src + (int64_t)i * ok);
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        const float w = (j0 + jj < im) ? w1s[i * im + j0 + jj] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) acc[jj][e] = fmaf(w, bf2f(v[e]), acc[jj][e]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
      if (j0 + jj < im) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = f2bf(acc[jj][e]);
        *(bf16x8*)(dst + (int64_t)(j0 + jj) * ok) = o;
      }
  }
}

extern "C" int st355_lokr_mix(void* stream, const void* dy, int64_t ldd, int64_t seg_rows, int64_t seg_stride, int n_off, const float* w1, int ol, int im, int ok,
                              void* dP, int64_t M) {
  ST_REQUIRE(dy && w1 && dP && M > 0, "lokr_mix: bad args");
  ST_REQUIRE(ol >= 1 && ol <= 16 && im >= 1 && im <= 16, "lokr_mix: the w1 sides must lie in 1 .. 16 (got ol = %d, im = %d)", ol, im);
  ST_REQUIRE(ok > 0 && ok % 8 == 0 && n_off >= 0 && n_off % 8 == 0 && ldd % 8 == 0 && ldd >= (int64_t)n_off + (int64_t)ol * ok,
             "lokr_mix: ok, n_off and the row stride must be multiples of 8 and the slab must lie inside a row (got ok = %d, n_off = %d)", ok, n_off);
  ST_REQUIRE(((uintptr_t)dy | (uintptr_t)dP) % 16 == 0, "lokr_mix: operands must be 16-byte aligned");
  ST_REQUIRE(M < ((int64_t)1 << 31), "lokr_mix: too many rows");
  ST_REQUIRE(seg_rows >= 0 && (seg_rows == 0 || (M % seg_rows == 0 && seg_stride >= seg_rows)), "lokr_mix: seg_rows must divide M, seg_stride >= seg_rows");
  const int64_t total = M * (ok / 8);
  ST_REQUIRE(cdiv64(total, 256) <= 0x7fffffff, "lokr_mix: too many elements");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * M * (double)ol * im * ok, 2.0 * M * (double)(ol + im) * ok);
  hipLaunchKernelGGL(k_lokr_mix, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)dy, ldd, (uint32_t)seg_rows, seg_stride, n_off, w1,
                     ol, im, ok, (bf16*)dP, total);
  return st355_check_launch("lokr_mix");
}

// ---- the fixed-order second stage of dw2: out[idx] (+)= alpha sum_s ws[s * slice + idx]; eight running sums (slice s goes to sum s & 7) keep eight loads in flight ----
__global__ void __launch_bounds__(256) k_lokr_reduce(const float* __restrict__ ws, float* out, int64_t total, int64_t slice, int nslices, float alpha, int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const float* p = ws + idx;
  float s[8];
#pragma unroll
  for (int u = 0; u < 8; u++) s[u] = 0.f;
  for (int q0 = 0; q0 < nslices; q0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (q0 + u < nslices) s[u] += p[(int64_t)(q0 + u) * slice];
  }
  const float v = alpha * (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])));
  out[idx] = accumulate ? out[idx] + v : v;
}

// ---- ... and of dw1: one workgroup per output element [i, j]; thread t adds partial tiles t, t + 256, ..., then a fixed halving tree over the 256 sums ----
__global__ void __launch_bounds__(256) k_lokr_dw1_reduce(const float* __restrict__ ws, float* out, int im, int ntiles, float alpha, int accumulate) {
  __shared__ float part[256];
  const int tid = threadIdx.x, i = blockIdx.x / im, j = blockIdx.x - i * im;
  float s = 0.f;
  for (int q = tid; q < ntiles; q += 256) s += ws[(int64_t)q * 256 + i * 16 + j];
  part[tid] = s;
  __syncthreads();
#pragma unroll
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    const float v = alpha * part[0];
    out[blockIdx.x] = accumulate ? out[blockIdx.x] + v : v;
  }
}

// ---- dw2 ----
static void lk_dw2_plan(int64_t rows, int ok, int in_, int* ts, int* tp, int* tq, int* nslices, int* cps) {
  *ts = (ok % 128 == 0 && in_ % 128 == 0) ? 128 : 64;          // 128 x 128 tiles where they tile the output exactly (192 x 192 would leave half of each empty)
  *tp = (ok + *ts - 1) / *ts;
  *tq = (in_ + *ts - 1) / *ts;
  const int64_t chunks = cdiv64(rows, 64);
  int64_t S = cdiv64(LK_DW2_WGS, (int64_t)*tp * *tq);
  if (S > chunks) S = chunks;
  if (S < 1) S = 1;
  const int64_t c = cdiv64(chunks, S);
  *cps = (int)c;
  *nslices = (int)cdiv64(chunks, c);
}

// WT = 1: a 64 x 64 output tile per workgroup (a 32 x 32 MFMA tile per wave);  WT = 2: 128 x 128 (2 x 2 MFMA tiles per wave) — half the operand re-reads of a large output
template <int WT>
__global__ void __launch_bounds__(256) k_lokr_dw2(const bf16* __restrict__ L, const bf16* __restrict__ x, int64_t ldx, uint32_t seg_rows, int64_t seg_stride, int im,
                                                 float* __restrict__ ws, int64_t rows, int ok, int in_, int cps) {
  constexpr int TS = 64 * WT;                 // tile side
  constexpr int NL = TS / 32;                 // 16-byte loads per thread, operand and chunk
  constexpr int LP = TS + 32;                 // LDS pitch in elements: 192 B / 320 B
  __shared__ __attribute__((aligned(16))) bf16 Ls[64 * LP];
  __shared__ __attribute__((aligned(16))) bf16 Rs[64 * LP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  // transposing-read geometry (ds_read_b64_tr_b16, common.h): group g = lane >> 4, ti = tile row within the 4-row block, tsg = 4-column segment
  const int g = lane >> 4, ti = (lane >> 2) & 3, tsg = lane & 3;
  const int row_l = 8 * (g >> 1) + ti, col_l = 16 * (g & 1) + 4 * tsg;
  const int p0 = blockIdx.y * TS, q0 = blockIdx.x * TS;
  const int64_t r_lo = (int64_t)blockIdx.z * cps * 64;
  int64_t r_hi = r_lo + (int64_t)cps * 64;
  if (r_hi > rows) r_hi = rows;
  bf16x8 lv[NL], rv[NL];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int c = tid + 256 * u, rr = c / (TS / 8), cc = c % (TS / 8);
      const int64_t row = r0 + rr;
      bf16x8 z;
#pragma unroll
      for (int e = 0; e < 8; e++) z[e] = (bf16)0.f;
      lv[u] = z;
      rv[u] = z;
      if (row < r_hi) {
        if (p0 + 8 * cc < ok) lv[u] = *(const bf16x8*)(L + row * ok + p0 + 8 * cc);
        if (q0 + 8 * cc < in_) {
          const uint32_t m = (uint32_t)(row / im);
          const int j = (int)(row - (int64_t)m * im);
          rv[u] = *(const bf16x8*)(x + lk_row_off(m, ldx, seg_rows, seg_stride) + (int64_t)j * in_ + q0 + 8 * cc);
        }
      }
    }
  };
  f32x16 acc[WT][WT];
#pragma unroll
  for (int a = 0; a < WT; a++)
#pragma unroll
    for (int b = 0; b < WT; b++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[a][b][i] = 0.f;
  const int pi = wv >> 1, qi = wv & 1;
  if (r_lo < r_hi) fetch(r_lo);
  for (int64_t r0 = r_lo; r0 < r_hi; r0 += 64) {
    __syncthreads();                       // the MFMAs of the chunk before are done with the LDS image
#pragma unroll
    for (int u = 0; u < NL; u++) {
      const int c = tid + 256 * u, rr = c / (TS / 8), cc = c % (TS / 8);
      *(bf16x8*)&Ls[rr * LP + 8 * cc] = lv[u];          // the chunk as it lies in memory: [contraction row][column]
      *(bf16x8*)&Rs[rr * LP + 8 * cc] = rv[u];
    }
    __syncthreads();
    if (r0 + 64 < r_hi) fetch(r0 + 64);    // flies under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      bf16x8 af[WT], bfr[WT];
#pragma unroll
      for (int a = 0; a < WT; a++) {          // lane (r, h) of the MFMA wants column 32 (WT pi + a) + r at contraction rows 16 ks + 8 h .. + 7: two transposing reads
        const bf16* lp = &Ls[(16 * ks + row_l) * LP + 32 * (WT * pi + a) + col_l];
        af[a] = lds_tr16x2(lp, lp + 4 * LP);
      }
#pragma unroll
      for (int b = 0; b < WT; b++) {
        const bf16* rp = &Rs[(16 * ks + row_l) * LP + 32 * (WT * qi + b) + col_l];
        bfr[b] = lds_tr16x2(rp, rp + 4 * LP);
      }
#pragma unroll
      for (int a = 0; a < WT; a++)
#pragma unroll
        for (int b = 0; b < WT; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
    }
  }
  // D[row p][col q]: lane -> column lane & 31, register reg -> row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* o = ws + (int64_t)blockIdx.z * ok * in_;
#pragma unroll
  for (int a = 0; a < WT; a++)
#pragma unroll
    for (int b = 0; b < WT; b++) {
      const int q = q0 + 32 * (WT * qi + b) + r;
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int p = p0 + 32 * (WT * pi + a) + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (p < ok && q < in_) o[(int64_t)p * in_ + q] = acc[a][b][reg];
      }
    }
}

extern "C" int64_t st355_lokr_dw2_workspace(int64_t rows, int ok, int in_) {
  if (rows <= 0 || ok <= 0 || in_ <= 0) return 0;
  int ts, tp, tq, S, cps;
  lk_dw2_plan(rows, ok, in_, &ts, &tp, &tq, &S, &cps);
  return (int64_t)S * ok * in_ * 4;
}

extern "C" int st355_lokr_dw2(void* stream, const void* dP, const void* x, int64_t ldx, int64_t seg_rows, int64_t seg_stride, int im, float* out, int64_t M, int ok,
                              int in_, float alpha, int accumulate, void* workspace) {
  ST_REQUIRE(dP && x && out && workspace && M > 0, "lokr_dw2: bad args");
  ST_REQUIRE(im >= 1 && im <= 16, "lokr_dw2: im must lie in 1 .. 16 (got %d)", im);
  ST_REQUIRE(ok > 0 && ok % 8 == 0 && in_ > 0 && in_ % 8 == 0 && ldx % 8 == 0 && ldx >= (int64_t)im * in_,
             "lokr_dw2: ok, in and the row stride of x must be multiples of 8, a row of x must hold im * in columns (got ok = %d, in = %d)", ok, in_);
  ST_REQUIRE(((uintptr_t)dP | (uintptr_t)x) % 16 == 0 && (uintptr_t)workspace % 4 == 0, "lokr_dw2: operands must be 16-byte aligned");
  ST_REQUIRE(M < ((int64_t)1 << 31) / 16, "lokr_dw2: too many rows");
  ST_REQUIRE(seg_rows >= 0 && (seg_rows == 0 || (M % seg_rows == 0 && seg_stride >= seg_rows)), "lokr_dw2: seg_rows must divide M, seg_stride >= seg_rows");
  const int64_t rows = M * im;
  int ts, tp, tq, S, cps;
  lk_dw2_plan(rows, ok, in_, &ts, &tp, &tq, &S, &cps);
  ST_REQUIRE(tp <= 65535 && S <= 65535, "lokr_dw2: output too large for one launch");
  ProfScope ps(stream, ST355_K_SKINNY, 2.0 * rows * (double)ok * in_, 2.0 * rows * ((double)ok * tq + (double)in_ * tp) + 8.0 * S * (double)ok * in_);
  const hipStream_t st = (hipStream_t)stream;
  if (ts == 128)
    hipLaunchKernelGGL(k_lokr_dw2<2>, dim3(tq, tp, S), dim3(256), 0, st, (const bf16*)dP, (const bf16*)x, ldx, (uint32_t)seg_rows, seg_stride, im, (float*)workspace,
                       rows, ok, in_, cps);
  else
    hipLaunchKernelGGL(k_lokr_dw2<1>, dim3(tq, tp, S), dim3(256), 0, st, (const bf16*)dP, (const bf16*)x, ldx, (uint32_t)seg_rows, seg_stride, im, (float*)workspace,
                       rows, ok, in_, cps);
  const int64_t total = (int64_t)ok * in_;
  hipLaunchKernelGGL(k_lokr_reduce, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, (const float*)workspace, out, total, total, S, alpha, accumulate);
  return st355_check_launch("lokr_dw2");
}

// ---- dw1 ----
static void lk_dw1_plan(int64_t M, int* nwg, int* per) {
  int64_t w = cdiv64(M, 4);                       // waves wanted: 4 rows each ...
  if (w > LK_DW1_WAVES) w = LK_DW1_WAVES;         // ... at most 16 per CU
  const int64_t g = cdiv64(w, 4);
  *per = (int)cdiv64(M, g * 4);
  *nwg = (int)g;
}

__global__ void __launch_bounds__(256) k_lokr_dw1(const bf16* __restrict__ dy, int64_t ldd, uint32_t seg_rows, int64_t seg_stride, int n_off,
                                                 const bf16* __restrict__ P, float* __restrict__ ws, int64_t M, int ol, int im, int ok, int per) {
  __shared__ float part[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, q = lane >> 4;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  const int64_t m0 = w * per;
  int64_t m1 = m0 + per;
  if (m1 > M) m1 = M;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; e++) z[e] = (bf16)0.f;
  // the wave's (row, 32-wide k step) pairs as ONE index space, four steps' loads in flight before their MFMAs (the accumulation order stays t = 0, 1, 2, ...)
  const int ksteps = (ok + 31) >> 5;
  const int64_t T = m1 > m0 ? (m1 - m0) * ksteps : 0;
  const int64_t ai = (int64_t)n_off + (int64_t)i * ok, bi = (int64_t)i * ok;
  for (int64_t t0 = 0; t0 < T; t0 += 4) {
    bf16x8 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      a[u] = z;
      b[u] = z;
      const int64_t t = t0 + u;
      if (t < T) {
        const int64_t mr = t / ksteps;
        const int64_t m = m0 + mr;
        const int k = 32 * (int)(t - mr * ksteps) + 8 * q;
        if (i < ol && k < ok) a[u] = *(const bf16x8*)(dy + lk_row_off((uint32_t)m, ldd, seg_rows, seg_stride) + ai + k);
        if (i < im && k < ok) b[u] = *(const bf16x8*)(P + m * im * ok + bi + k);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[u], acc, 0, 0, 0);
  }
  // D[row i][col j]: lane -> column lane & 15, register reg -> row 4 (lane >> 4) + reg.  The four waves' tiles are added in wave order.
#pragma unroll
  for (int reg = 0; reg < 4; reg++) part[wv][(4 * q + reg) * 16 + i] = acc[reg];
  __syncthreads();
  ws[(int64_t)blockIdx.x * 256 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

extern "C" int64_t st355_lokr_dw1_workspace(int64_t M) {
  if (M <= 0) return 0;
  int nwg, per;
  lk_dw1_plan(M, &nwg, &per);
  return (int64_t)nwg * 256 * 4;
}

extern "C" int st355_lokr_dw1(void* stream, const void* dy, int64_t ldd, int64_t seg_rows, int64_t seg_stride, int n_off, const void* P, float* out, int64_t M, int ol,
                              int im, int ok, float alpha, int accumulate, void* workspace) {
  ST_REQUIRE(dy && P && out && workspace && M > 0, "lokr_dw1: bad args");
  ST_REQUIRE(ol >= 1 && ol <= 16 && im >= 1 && im <= 16, "lokr_dw1: the w1 sides must lie in 1 .. 16 (got ol = %d, im = %d)", ol, im);
  ST_REQUIRE(ok > 0 && ok % 8 == 0 && n_off >= 0 && n_off % 8 == 0 && ldd % 8 == 0 && ldd >= (int64_t)n_off + (int64_t)ol * ok,
             "lokr_dw1: ok, n_off and the row stride must be multiples of 8 and the slab must lie inside a row (got ok = %d, n_off = %d)", ok, n_off);
  ST_REQUIRE(((uintptr_t)dy | (uintptr_t)P) % 16 == 0 && (uintptr_t)workspace % 4 == 0, "lokr_dw1: operands must be 16-byte aligned");
  ST_REQUIRE(M < ((int64_t)1 << 31), "lokr_dw1: too many rows");
  ST_REQUIRE(seg_rows >= 0 && (seg_rows == 0 || (M % seg_rows == 0 && seg_stride >= seg_rows)), "lokr_dw1: seg_rows must divide M, seg_stride >= seg_rows");
  int nwg, per;
  lk_dw1_plan(M, &nwg, &per);
  ProfScope ps(stream, ST355_K_SKINNY, 2.0 * M * (double)ol * im * ok, 2.0 * M * (double)(ol + im) * ok + 1024.0 * nwg);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_lokr_dw1, dim3(nwg), dim3(256), 0, st, (const bf16*)dy, ldd, (uint32_t)seg_rows, seg_stride, n_off, (const bf16*)P, (float*)workspace, M, ol,
                     im, ok, per);
  hipLaunchKernelGGL(k_lokr_dw1_reduce, dim3(ol * im), dim3(256), 0, st, (const float*)workspace, out, im, nwg, alpha, accumulate);
  return st355_check_launch("lokr_dw1");
}

// lora_dropout.hip — LoRA dropout (peft `lora_dropout`): y = base(x) + (alpha / r) B A dropout(x), the mask never stored.
//
// A keep bit is a pure function of (key, call, stream, row, col) — st355_lora_drop in st355.h: Philox4x32-10 with counter (c0, c1) = the 64-bit group index
// (row * K + col) / 8, c2 = the stream id (the adapted Linear), c3 = the call counter (read from the device), key = (key0, key1).  One call gives 4 x 32 bits =
// eight 16-bit lanes for the eight consecutive input columns of one row (K % 8 == 0, so a group never straddles rows): element j takes bits 16 (j % 2) of word
// j / 2, and is DROPPED iff that lane < threshold.  A bf16x8 of x is four 32-bit words whose 16-bit halves sit exactly where the element's random lane sits in
// the Philox word of the same index, so masking is four AND operations.  `row` is the LOGICAL row of the Linear's input (b * rows + s inside its stream), whatever
// the operand's lay-out (compact, or a [B, rows, C] view of a joint buffer): every kernel below turns the logical row into an address by row_off().
//
//   st355_lora_down_drop   T[m, g r_pad + r]   = scale sum_k keep_g(m,k) x[m,k] A_cat[g r_pad + r, k]        (bf16, one rounding; one pass over x for all targets)
//   st355_skinny_tn_drop   dA_g[r, k]     (+)= scale sum_m U[m, g r_pad + r] keep_g(m,k) x[m,k]               (fp32; `_multi`: the q / k / v adapters in one pass)
//   st355_lora_dx_drop     dx[m, k]        += scale sum_g keep_g(m,k) sum_r U[m, g r_pad + r] A_cat[g r_pad + r, k]   (bf16 in place, one rounding)
//   st355_lora_dropout_mask     the keep bits as uint8 [M, K] (tests and tools; never on the step)
//   st355_lora_dropout_advance  *call += 1 (one thread; belongs to the step, so a captured step advances on the device)
// The scale 1 / (1 - threshold / 65536) multiplies fp32 accumulators, never x; dropped elements are exact zeros.
#include "common.h"

#define LD_MS 32                // rows per LDS sub-tile of the dA kernel
#define LD_PT 128               // columns of x per workgroup of the dA kernel
#define LD_LP (LD_PT + 32)      // LDS pitch of an x tile (elements): 64 B mod 256 B, as skinny.hip
#define LD_MC 256               // smallest split-M chunk of the dA kernel

struct DropArgs {
  uint32_t k0, k1, thr;
  float scale;
  const uint32_t* call;
  uint32_t streams[4];
};

__device__ __forceinline__ u32x4 drop_philox(uint64_t group, uint32_t stream, uint32_t call, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {(uint32_t)group, (uint32_t)(group >> 32), stream, call};
#pragma unroll
  for (int i = 0; i < 10; i++) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  u32x4 o;
  o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
  return o;
}
// the AND mask of one group of eight bf16 (as four words): all ones over a kept element, zero over a dropped one
__device__ __forceinline__ u32x4 drop_keep_words(uint64_t group, uint32_t stream, uint32_t call, const DropArgs& d) {
  const u32x4 r = drop_philox(group, stream, call, d.k0, d.k1);
  u32x4 m;
#pragma unroll
  for (int w = 0; w < 4; w++) m[w] = ((r[w] & 0xFFFFu) >= d.thr ? 0x0000FFFFu : 0u) | ((r[w] >> 16) >= d.thr ? 0xFFFF0000u : 0u);
  return m;
}
// element offset of logical row m: compact (seg_rows == 0), or segment m / seg_rows at seg_stride ROWS from the previous one
__device__ __forceinline__ int64_t row_off(uint32_t m, int64_t ld, uint32_t seg_rows, int64_t seg_stride) {
  if (seg_rows == 0) return (int64_t)m * ld;
  const uint32_t s = m / seg_rows;
  return ((int64_t)s * seg_stride + (int64_t)(m - s * seg_rows)) * ld;
}

// ---- the keep bits, exported ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_drop_mask(uint8_t* __restrict__ out, int64_t ngroups, uint32_t stream, DropArgs d) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  const u32x4 r = drop_philox((uint64_t)g, stream, *d.call, d.k0, d.k1);
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int e = 4 * h + j;
      const uint32_t lane16 = (r[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
      v |= (lane16 >= d.thr ? 1u : 0u) << (8 * j);
    }
    o[h] = v;
  }
  *(u32x2*)(out + g * 8) = o;
}
__global__ void k_drop_advance(uint32_t* call) {
  if (threadIdx.x == 0 && blockIdx.x == 0) call[0] = call[0] + 1u;
}

// ---- forward: T = scale (keep_g . x) A_cat^T ----------------------------------------------------------------------------------------------------------------------
// One workgroup = 32 rows of x, one wave per target: the waves read the same 16-byte chunks of x at the same time (one trip to memory), each masks them with its
// own stream and multiplies by its own r_pad rows of A_cat.  Both MFMA operands are K-contiguous in memory, so a lane's fragment (8 consecutive k of one row) is
// one 16-byte load — and exactly one Philox group.
template <int NB>   // 32-column blocks per target (r_pad / 32)
__global__ void __launch_bounds__(256) k_down_drop(const bf16* __restrict__ x, int64_t ldx, uint32_t seg_rows, int64_t seg_stride, const bf16* __restrict__ A,
                                                  bf16* __restrict__ T, int64_t ldt, uint32_t M, int K, int G, int K2, DropArgs d) {
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t row0 = blockIdx.x * 32u, m = row0 + r;
  const bool valid = m < M;
  const bf16* xr = x + (valid ? row_off(m, ldx, seg_rows, seg_stride) : 0);
  const uint32_t call = *d.call, stream = d.streams[g];
  const uint64_t grp0 = (uint64_t)m * (uint64_t)(K >> 3);
  const int r_pad = 32 * NB;
  f32x16 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[b][i] = 0.f;
  for (int k = 0; k < K; k += 16) {
    const int kk = k + 8 * h;
    const bool in = kk < K;
    u32x4 xv = {0u, 0u, 0u, 0u};
    if (valid && in) {
      xv = *(const u32x4*)(xr + kk);
      const u32x4 keep = drop_keep_words(grp0 + (uint64_t)(kk >> 3), stream, call, d);
      xv &= keep;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
      u32x4 av = {0u, 0u, 0u, 0u};
      if (in) av = *(const u32x4*)(A + (int64_t)(g * r_pad + 32 * b + r) * K + kk);
      acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8*)&xv, *(bf16x8*)&av, acc[b], 0, 0, 0);
    }
  }
  // D[i = row][j = column]: lane -> column lane & 31, register reg -> row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const uint32_t mm = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (mm < M) T[(int64_t)mm * ldt + g * r_pad + 32 * b + r] = f2bf(d.scale * acc[b][reg]);
    }
  if (g == G - 1)          // the padding columns of the K-extension (G r_pad rounded up to 64): zeros, as the unmasked product leaves them
    for (int c = G * r_pad + r; c < K2; c += 32)
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const uint32_t mm = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (mm < M) T[(int64_t)mm * ldt + c] = f2bf(0.f);
      }
}

// ---- backward: dx += scale sum_g keep_g . (U_g A_g) ---------------------------------------------------------------------------------------------------------------
// One wave = a 32 (rows) x 32 (columns of dx) tile.  Per target: P^T = A_cat_T[k, :] U[m, :]^T on the MFMA (both operands r-contiguous in memory), the fp32 tile goes
// through the wave's LDS slab to the [row][8 consecutive columns] lay-out in which one lane owns whole Philox groups, is masked there and summed over the targets
// in registers; dx is read and written once, 16 bytes per lane.
__global__ void __launch_bounds__(256) k_dx_drop(bf16* __restrict__ dx, int64_t ldd, uint32_t seg_rows, int64_t seg_stride, const bf16* __restrict__ U, int64_t ldu,
                                                const bf16* __restrict__ At, uint32_t M, int K, int G, int r_pad, int K2, DropArgs d) {
  __shared__ float tile[4][32][33];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int kc0 = (blockIdx.x * 4 + wv) * 32;
  const uint32_t row0 = blockIdx.y * 32u;
  const uint32_t call = *d.call;
  const int kcol = kc0 + r;                  // this lane's row of A_cat_T (A operand)
  const uint32_t mrow = row0 + r;            // this lane's row of U (B operand)
  float sum[2][8];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int j = 0; j < 8; j++) sum[t][j] = 0.f;
  for (int g = 0; g < G; g++) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    for (int rs = 0; rs < r_pad; rs += 16) {
      const int c = g * r_pad + rs + 8 * h;
      u32x4 av = {0u, 0u, 0u, 0u}, bv = {0u, 0u, 0u, 0u};
      if (kcol < K) av = *(const u32x4*)(At + (int64_t)kcol * K2 + c);
      if (mrow < M) bv = *(const u32x4*)(U + (int64_t)mrow * ldu + c);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(bf16x8*)&av, *(bf16x8*)&bv, acc, 0, 0, 0);
    }
    // D[i = column of dx][j = row]: lane -> row lane & 31, register reg -> column (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) tile[wv][r][(reg & 3) + 8 * (reg >> 2) + 4 * h] = acc[reg];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int p = lane + 64 * t, mo = p >> 2, kg = p & 3;
      const uint32_t mm = row0 + mo;
      const int kk = kc0 + 8 * kg;
      if (mm < M && kk < K) {
        const u32x4 keep = drop_keep_words((uint64_t)mm * (uint64_t)(K >> 3) + (uint64_t)(kk >> 3), d.streams[g], call, d);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const bool kept = (keep[j >> 1] >> (16 * (j & 1))) & 1u;
          sum[t][j] += kept ? tile[wv][mo][8 * kg + j] : 0.f;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const int p = lane + 64 * t, mo = p >> 2, kg = p & 3;
    const uint32_t mm = row0 + mo;
    const int kk = kc0 + 8 * kg;
    if (mm < M && kk < K) {
      bf16* o = dx + row_off(mm, ldd, seg_rows, seg_stride) + kk;
      bf16x8 v = *(const bf16x8*)o;
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = f2bf(bf2f(v[j]) + d.scale * sum[t][j]);
      *(bf16x8*)o = v;
    }
  }
}

// ---- backward: dA_g = scale U_g^T (keep_g . x) --------------------------------------------------------------------------------------------------------------------
// skinny.hip's k_skinny_tn_mfma with the mask applied where the x sub-tile goes from registers to LDS: a thread's 16-byte chunk is one Philox group.  NS = 1: one
// stream for the whole R tile (RN = 32 / 64 columns of one target); NS = 4 (RN = 128): column block j of R belongs to target j and reads its own masked copy of
// the x tile — x still comes from memory once.
template <int RN, int NS>
__global__ void __launch_bounds__(256) k_skinny_tn_drop(const bf16* __restrict__ L, int64_t ldl, const bf16* __restrict__ R, int64_t ldr, float* __restrict__ ws,
                                                       uint32_t M, int P, uint32_t seg_rows, int64_t seg_l, int64_t seg_r, int mc, DropArgs d) {
  constexpr int RT = RN / 32;
  constexpr int RP = (RN == 32) ? 32 : (RN == 64 ? 96 : 160);
  __shared__ __attribute__((aligned(16))) bf16 Ls[NS][LD_MS * LD_LP];
  __shared__ __attribute__((aligned(16))) bf16 Rs[LD_MS * RP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = blockIdx.x * LD_PT;
  const uint32_t mbase = blockIdx.y * (uint32_t)mc;
  const uint32_t call = *d.call;
  f32x16 acc[RT];
#pragma unroll
  for (int j = 0; j < RT; j++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
  const int g = lane >> 4, ti = (lane >> 2) & 3, tsg = lane & 3;
  const int row_l = 8 * (g >> 1) + ti;
  const int a_col = 32 * wv + 16 * (g & 1) + 4 * tsg;
  const int b_col = 16 * (g & 1) + 4 * tsg;

  constexpr int RCH = (LD_MS * RN / 8 + 255) / 256;
  constexpr int LCH = LD_MS / 16;
  u32x4 lreg[LCH], rreg[RCH];
  auto load = [&](int ms) {
#pragma unroll
    for (int k = 0; k < LCH; k++) {
      const int id = k * 256 + tid;
      const int row = id >> 4, c = id & 15;
      const uint32_t m = mbase + ms + row;
      lreg[k] = u32x4{0u, 0u, 0u, 0u};
      if (m < M && p0 + c * 8 < P) lreg[k] = *(const u32x4*)(L + row_off(m, ldl, seg_rows, seg_l) + p0 + c * 8);
    }
#pragma unroll
    for (int q = 0; q < RCH; q++) {
      const int id = q * 256 + tid;
      rreg[q] = u32x4{0u, 0u, 0u, 0u};
      if (id < LD_MS * RN / 8) {
        const int row = id / (RN / 8), c = id % (RN / 8);
        const uint32_t m = mbase + ms + row;
        if (m < M) rreg[q] = *(const u32x4*)(R + row_off(m, ldr, seg_rows, seg_r) + c * 8);
      }
    }
  };
  auto store = [&](int ms) {
#pragma unroll
    for (int k = 0; k < LCH; k++) {
      const int id = k * 256 + tid;
      const int row = id >> 4, c = id & 15;
      const uint32_t m = mbase + ms + row;
      const bool live = m < M && p0 + c * 8 < P;
      const uint64_t grp = (uint64_t)m * (uint64_t)(P >> 3) + (uint64_t)((p0 + c * 8) >> 3);
#pragma unroll
      for (int s = 0; s < NS; s++) {
        u32x4 v = lreg[k];
        if (live) v &= drop_keep_words(grp, d.streams[s], call, d);
        *(u32x4*)(&Ls[s][row * LD_LP + c * 8]) = v;
      }
    }
#pragma unroll
    for (int q = 0; q < RCH; q++) {
      const int id = q * 256 + tid;
      if (id < LD_MS * RN / 8) *(u32x4*)(&Rs[(id / (RN / 8)) * RP + (id % (RN / 8)) * 8]) = rreg[q];
    }
  };
  load(0);
  for (int ms = 0; ms < mc; ms += LD_MS) {
    store(ms);
    __syncthreads();
    if (ms + LD_MS < mc) load(ms + LD_MS);
#pragma unroll
    for (int ks = 0; ks < LD_MS / 16; ks++) {
#pragma unroll
      for (int j = 0; j < RT; j++) {
        const bf16* lp = &Ls[NS == 1 ? 0 : j][(16 * ks + row_l) * LD_LP + a_col];
        const bf16x8 af = lds_tr16x2(lp, lp + 4 * LD_LP);
        const bf16* rp = &Rs[(16 * ks + row_l) * RP + b_col + 32 * j];
        const bf16x8 bfr = lds_tr16x2(rp, rp + 4 * RP);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // D[i = p][j = r]: lane -> r = lane & 31, register reg -> p = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* w = ws + ((int64_t)blockIdx.y * P) * RN;
#pragma unroll
  for (int j = 0; j < RT; j++)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int pp = p0 + 32 * wv + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      if (pp < P) w[(int64_t)pp * RN + 32 * j + (lane & 31)] = acc[j][reg];
    }
}

// fixed-order reduction of the split-M partials (the lane / chunk order of skinny.hip's k_skinny_reduce): output g takes columns [blk g, blk g + r_used) of ws
struct DropOuts { float* o[4]; };
__global__ void __launch_bounds__(256) k_drop_reduce(const float* __restrict__ ws, DropOuts outs, int64_t so_p, int64_t so_r, int P, int RN, int r_used, int nout,
                                                    int blk, int nchunks, float alpha, int accumulate) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = t / 4;
  const int q = (int)(t % 4);
  const bool live = i < (int64_t)P * r_used * nout;
  const int r = live ? (int)(i % r_used) : 0;
  const int g = live ? (int)((i / r_used) % nout) : 0;
  const int64_t p = live ? i / ((int64_t)r_used * nout) : 0;
  float s = 0.f;
  if (live)
    for (int c = q; c < nchunks; c += 4) s += ws[((int64_t)c * P + p) * RN + blk * g + r];
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (live && q == 0) {
    float* o = outs.o[g] + p * so_p + r * so_r;
    *o = (accumulate ? *o : 0.f) + alpha * s;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------------
static int drop_args(const st355_lora_drop* dr, int n_streams, DropArgs& d, const char* what) {
  ST_REQUIRE(dr && dr->call, "%s: null dropout state / call counter", what);
  ST_REQUIRE(dr->threshold >= 1 && dr->threshold <= 65535, "%s: threshold %u outside 1 .. 65535 (0 < p < 1)", what, dr->threshold);
  ST_REQUIRE(n_streams >= 1 && n_streams <= 4, "%s: 1 .. 4 targets (got %d)", what, n_streams);
  d.k0 = dr->key0; d.k1 = dr->key1; d.thr = dr->threshold; d.scale = dr->scale; d.call = dr->call;
  for (int i = 0; i < 4; i++) d.streams[i] = dr->streams[i < n_streams ? i : n_streams - 1];
  return 0;
}
static bool seg_ok(int64_t M, int64_t seg_rows, int64_t seg_stride) {
  return seg_rows == 0 || (seg_rows > 0 && M % seg_rows == 0 && seg_stride >= seg_rows);
}

extern "C" int st355_lora_dropout_mask(void* stream, uint8_t* out, int64_t M, int64_t K, const st355_lora_drop* dr) {
  DropArgs d;
  int rc = drop_args(dr, 1, d, "lora_dropout_mask");
  if (rc) return rc;
  ST_REQUIRE(out && M > 0 && K > 0 && K % 8 == 0, "lora_dropout_mask: K (%lld) must be a positive multiple of 8", (long long)K);
  const int64_t ng = M * (K / 8);
  hipLaunchKernelGGL(k_drop_mask, dim3((unsigned)cdiv64(ng, 256)), dim3(256), 0, (hipStream_t)stream, out, ng, d.streams[0], d);
  return st355_check_launch("lora_dropout_mask");
}
extern "C" int st355_lora_dropout_advance(void* stream, uint32_t* call) {
  ST_REQUIRE(call, "lora_dropout_advance: null counter");
  hipLaunchKernelGGL(k_drop_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, call);
  return st355_check_launch("lora_dropout_advance");
}

extern "C" int st355_lora_down_drop(void* stream, const void* x, int64_t ldx, int64_t seg_rows, int64_t seg_stride, const void* A_cat, void* T, int64_t ldt,
                                    int64_t M, int K, int G, int r_pad, int K2, const st355_lora_drop* dr) {
  DropArgs d;
  int rc = drop_args(dr, G, d, "lora_down_drop");
  if (rc) return rc;
  ST_REQUIRE(x && A_cat && T, "lora_down_drop: null pointer");
  ST_REQUIRE(M > 0 && M < (1ll << 31) && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K, "lora_down_drop: K (%d) must be a multiple of 8, ldx a multiple of 8 >= K", K);
  ST_REQUIRE(r_pad == 32 || r_pad == 64 || r_pad == 128, "lora_down_drop: r_pad must be 32, 64 or 128 (got %d)", r_pad);
  ST_REQUIRE(K2 % 32 == 0 && G * r_pad <= K2 && ldt >= K2, "lora_down_drop: G r_pad (%d) must fit the K2 = %d columns of T", G * r_pad, K2);
  ST_REQUIRE(seg_ok(M, seg_rows, seg_stride), "lora_down_drop: seg_rows must divide M, the segment stride be >= seg_rows");
  ProfScope ps(stream, ST355_K_SKINNY, 2.0 * M * K * G * r_pad, 2.0 * M * (K + K2) + 2.0 * K2 * K);
  dim3 grid((unsigned)cdiv64(M, 32)), blk(64 * G);
#define LAUNCH_DOWN(NB)                                                                                                                                       \
  hipLaunchKernelGGL(k_down_drop<NB>, grid, blk, 0, (hipStream_t)stream, (const bf16*)x, ldx, (uint32_t)seg_rows, seg_stride, (const bf16*)A_cat, (bf16*)T, ldt, \
                     (uint32_t)M, K, G, K2, d)
  if (r_pad == 32) LAUNCH_DOWN(1);
  else if (r_pad == 64) LAUNCH_DOWN(2);
  else LAUNCH_DOWN(4);
#undef LAUNCH_DOWN
  return st355_check_launch("lora_down_drop");
}

extern "C" int st355_lora_dx_drop(void* stream, void* dx, int64_t ldd, int64_t seg_rows, int64_t seg_stride, const void* U, int64_t ldu, const void* A_cat_T,
                                  int64_t M, int K, int G, int r_pad, int K2, const st355_lora_drop* dr) {
  DropArgs d;
  int rc = drop_args(dr, G, d, "lora_dx_drop");
  if (rc) return rc;
  ST_REQUIRE(dx && U && A_cat_T, "lora_dx_drop: null pointer");
  ST_REQUIRE(M > 0 && M < (1ll << 31) && K > 0 && K % 8 == 0 && ldd % 8 == 0 && ldd >= K, "lora_dx_drop: K (%d) must be a multiple of 8, ldd a multiple of 8 >= K", K);
  ST_REQUIRE(r_pad == 32 || r_pad == 64 || r_pad == 128, "lora_dx_drop: r_pad must be 32, 64 or 128 (got %d)", r_pad);
  ST_REQUIRE(K2 % 8 == 0 && G * r_pad <= K2 && ldu % 8 == 0 && ldu >= K2, "lora_dx_drop: G r_pad (%d) must fit the K2 = %d columns of U", G * r_pad, K2);
  ST_REQUIRE(seg_ok(M, seg_rows, seg_stride), "lora_dx_drop: seg_rows must divide M, the segment stride be >= seg_rows");
  ST_REQUIRE(cdiv64(M, 32) <= 65535, "lora_dx_drop: at most 65535 x 32 rows per call");
  ProfScope ps(stream, ST355_K_SKINNY, 2.0 * M * K * G * r_pad, 4.0 * M * K + 2.0 * M * K2 + 2.0 * K2 * K);
  dim3 grid((unsigned)cdiv64(K, 128), (unsigned)cdiv64(M, 32));
  hipLaunchKernelGGL(k_dx_drop, grid, dim3(256), 0, (hipStream_t)stream, (bf16*)dx, ldd, (uint32_t)seg_rows, seg_stride, (const bf16*)U, ldu, (const bf16*)A_cat_T,
                     (uint32_t)M, K, G, r_pad, K2, d);
  return st355_check_launch("lora_dx_drop");
}

// rows per workgroup of the dA kernel: the largest chunk that still leaves >= 512 workgroups (skinny.hip's rule; the per-row addressing needs no segment alignment)
static int drop_chunk(int64_t M, int64_t P) {
  const int64_t pt = cdiv64(P, LD_PT);
  for (int mc = 1024; mc > LD_MC; mc >>= 1)
    if (cdiv64(M, mc) * pt >= 512) return mc;
  return LD_MC;
}
static int skinny_drop_launch(void* stream, const void* L, int64_t ldl, const void* R, int64_t ldr, float* const* outs, int nout, int64_t so_p, int64_t so_r,
                              int64_t M, int64_t P, int Rn, int r_used, float alpha, int accumulate, void* workspace, int64_t seg_rows, int64_t seg_l, int64_t seg_r,
                              const st355_lora_drop* dr, bool multi, const char* what) {
  DropArgs d;
  int rc = drop_args(dr, nout, d, what);
  if (rc) return rc;
  ST_REQUIRE(L && R && outs && workspace, "%s: null pointer", what);
  for (int g = 0; g < nout; g++) ST_REQUIRE(outs[g] != nullptr, "%s: null output %d", what, g);
  ST_REQUIRE(M > 0 && M < (1ll << 31) && P > 0 && P < (1ll << 31) && P % 8 == 0 && ldl % 8 == 0 && ldr % 8 == 0 && ldl >= P && ldr >= Rn, "%s: bad shape", what);
  ST_REQUIRE(r_used > 0 && r_used <= (multi ? 32 : Rn), "%s: r_used (%d) outside the column block", what, r_used);
  ST_REQUIRE(seg_ok(M, seg_rows, seg_l ? seg_l : seg_rows) && seg_ok(M, seg_rows, seg_r ? seg_r : seg_rows), "%s: seg_rows must divide M, strides >= seg_rows", what);
  const int mc = drop_chunk(M, P);
  const int nchunks = (int)cdiv64(M, mc);
  // a compact operand beside a segmented one: its segments follow each other (stride = seg_rows)
  const int64_t sl = seg_rows ? (seg_l ? seg_l : seg_rows) : 0, sr = seg_rows ? (seg_r ? seg_r : seg_rows) : 0;
  ProfScope ps(stream, ST355_K_SKINNY, 2.0 * M * P * Rn, 2.0 * M * (P + Rn) + 8.0 * nchunks * P * Rn);
  dim3 grid((unsigned)cdiv64(P, LD_PT), nchunks);
#define LAUNCH_TN(RN_, NS_)                                                                                                                                   \
  hipLaunchKernelGGL((k_skinny_tn_drop<RN_, NS_>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)L, ldl, (const bf16*)R, ldr, (float*)workspace, (uint32_t)M, \
                     (int)P, (uint32_t)seg_rows, sl, sr, mc, d)
  if (multi) LAUNCH_TN(128, 4);
  else if (Rn == 32) LAUNCH_TN(32, 1);
  else LAUNCH_TN(64, 1);
#undef LAUNCH_TN
  rc = st355_check_launch(what);
  if (rc) return rc;
  DropOuts so{};
  for (int g = 0; g < nout; g++) so.o[g] = outs[g];
  const int64_t n = P * r_used * nout * 4;
  hipLaunchKernelGGL(k_drop_reduce, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, so, so_p, so_r, (int)P, Rn, r_used, nout,
                     32, nchunks, alpha * d.scale, accumulate);
  return st355_check_launch("lora_drop_reduce");
}
extern "C" int st355_skinny_tn_drop(void* stream, const void* L, int64_t ldl, const void* R, int64_t ldr, float* out, int64_t so_p, int64_t so_r, int64_t M, int64_t P,
                                    int Rn, int r_used, float alpha, int accumulate, void* workspace, int64_t seg_rows, int64_t seg_l, int64_t seg_r,
                                    const st355_lora_drop* dr) {
  ST_REQUIRE(Rn == 32 || Rn == 64, "skinny_tn_drop: Rn must be 32 or 64 (got %d)", Rn);
  float* outs[1] = {out};
  return skinny_drop_launch(stream, L, ldl, R, ldr, outs, 1, so_p, so_r, M, P, Rn, r_used, alpha, accumulate, workspace, seg_rows, seg_l, seg_r, dr, false,
                            "skinny_tn_drop");
}
extern "C" int st355_skinny_tn_drop_multi(void* stream, const void* L, int64_t ldl, const void* R, int64_t ldr, float* const* outs, int nout, int64_t so_p, int64_t so_r,
                                          int64_t M, int64_t P, int r_used, float alpha, int accumulate, void* workspace, int64_t seg_rows, int64_t seg_l,
                                          int64_t seg_r, const st355_lora_drop* dr) {
  ST_REQUIRE(outs && nout >= 1 && nout <= 4 && ldr >= 128, "skinny_tn_drop_multi: 1 .. 4 outputs, R needs 128 columns");
  return skinny_drop_launch(stream, L, ldl, R, ldr, outs, nout, so_p, so_r, M, P, 128, r_used, alpha, accumulate, workspace, seg_rows, seg_l, seg_r, dr, true,
                            "skinny_tn_drop_multi");
}

// attention_sage.hip — SageAttention-style quantised attention FORWARD for validation sampling (no backward, no lse2, no key bias):
//   O = softmax(scale * Q K^T) V   with Q K^T on the int8 MFMA and P V on the fp8 MFMA, both at twice the bf16 issue rate on gfx950.
//
// Numerics (c = scale * log2 e; include/st355.h restates them, tests/attn_sage_ref.py is the torch restatement):
//   kbar[b,h,:] = mean_{s<S} K[b,h,s,:] in fp32, two fixed-order stages (64-row partial sums in row order, then the partials in block order, then / S);
//   K' = K - kbar (exact for softmax: every score of a row moves by q.kbar);
//   Qh / Kh = rne(x / s) as int8 with s = amax|x| / 127 per block of 64 rows (1 for an all-zero block), rows >= S written as zero;
//   Vh = e4m3(V / sv) with sv = amax_{s<S}|V| / 448 per (b, h, channel) (1 for an all-zero row), columns >= S written as zero;
//   per 128-key step: s2 = int32(Qh.Kh) * (sq * sk * c), keys >= S masked, online max m, e = exp2(s2 - m + 8) (the 2^8 of the e4m3 grid rides in the exponent),
//   l += sum e (unquantised), acc = acc * alpha + e4m3(e) . Vh;   O = acc * sv / l -> bf16.
//
// Quantise pass, four launches, no atomics: k_sage_kpart (64-row column sums of K, one lane per block and 8-channel chunk, rows in order), k_sage_kmean (the partials in
// block order, / S), k_sage_quant_qk (one wave per 64-row block of Q or K: amax, scale, int8 rows) and k_sage_quant_v (one wave per V^T row: amax along the
// contiguous key axis, scale, v_cvt_pk_fp8_f32).
//
// Main kernel k_sage_fwd, gfx950 design:
//   * workgroup = 4 waves x 32 queries (two 16-query MFMA column tiles per wave, every Kh / Vh fragment read feeding two MFMAs), 128-key steps, LDS ring of
//     2 x 32 KiB at d 128 and 2 x 16 KiB at d 64.  Occupancy: d 64 runs two workgroups per CU (206 VGPRs, no spills); d 128 is bounded to ONE workgroup per
//     CU (one wave per SIMD, 388 of the 512 registers): under the 256-register budget of two waves per SIMD hipcc spilled 80 registers in the main loop
//     (64 score + 64 O^T + 16 Qh + 16 P + 16 staging registers are live together), also with the two query tiles' scores taken in turn.
//   * scores are computed TRANSPOSED on v_mfma_i32_16x16x64_i8 (S^T = Kh Qh^T: the Kh tile is the A operand from LDS, Qh the B operand held in registers;
//     one MFMA per 16 x 16 score tile at d 64, two at d 128), so lane (n, g) = (lane & 15, lane >> 4) owns query column n and key rows 4 g + r of every tile.
//   * the Kh tile is staged in PERMUTED row order: LDS row 16 t + 4 a + b holds key 32 a + 4 t + b.  Score tile t then leaves key 32 g + 4 t + r in register r
//     of lane (n, g), so the lane's 32 exponentials of a step, packed to e4m3 in register order, are keys 32 g .. 32 g + 31 in byte order: exactly the B
//     operand of O^T += Vh^T P^T on v_mfma_scale_f32_16x16x128_f8f6f4 against a PLAIN 32-byte row read of the Vh tile.  P never crosses lanes or touches LDS.
//     (Both operands of either MFMA use the same lane -> contraction-index map, and contraction order is free, so no knowledge of the instructions' internal
//     K order is needed.)  Block scales are the unit E8M0 byte 127; the real scales sq, sk, sv stay in fp32 around the MFMAs.
//   * a lane's 32 keys of a step lie in ONE 64-key block: its raw int32 maximum is taken first and scaled once; the scale rides in the exponent's fma.
//   * row maximum across the four lane groups by v_permlane16_swap + v_permlane32_swap (VALU, no LDS round trip); the row sum is reduced once, at the end.
//   * both LDS images use XOR-swizzled 16-byte chunks (16 consecutive rows of one chunk column are conflict-free for ds_read_b128); register-staged double
//     buffering as in k_attn_fwd4 (next step's global loads issued before the MFMA work, written to the other buffer after it).
//   * the ragged last step is peeled (MASKED): keys >= S are excluded from the maximum and contribute exact zeros; Kh rows / Vh columns >= Sp are staged as
//     zeros, never read.  Query rows >= S are clamped on load and not stored.  No atomics, no scratch: launches are bit-identical.
#include <type_traits>
#include "attn_common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---- workspace layout (bytes; every section starts on a 256-byte boundary; ops.py mirrors it) ----
struct SageWs { size_t qh, kh, vh, sq, sk, sv, kmean, kpart, total; };
static inline size_t sage_up(size_t x) { return (x + 255) & ~(size_t)255; }
static SageWs sage_ws(int B, int H, int Sp, int d) {
  const size_t BH = (size_t)B * H, nb = (size_t)Sp / 64;
  SageWs w;
  size_t o = 0;
  w.qh = o; o += sage_up(BH * Sp * d);
  w.kh = o; o += sage_up(BH * Sp * d);
  w.vh = o; o += sage_up(BH * Sp * d);
  w.sq = o; o += sage_up(BH * nb * 4);
  w.sk = o; o += sage_up(BH * nb * 4);
  w.sv = o; o += sage_up(BH * d * 4);
  w.kmean = o; o += sage_up(BH * d * 4);
  w.kpart = o; o += sage_up(BH * nb * d * 4);
  w.total = o;
  return w;
}

// ------------------------------------------------------------------------------------------------
// quantise pass
// ------------------------------------------------------------------------------------------------
// stage 1 of the K column mean: lane = (block, 8-channel chunk), 64 / (D / 8) blocks per wave; a lane adds the 64 rows of its block in row order (rows >= S
// add +0) from 16-byte loads, so every channel's sum is formed in one fixed order by one lane
template <int D>
__global__ void __launch_bounds__(64) k_sage_kpart(const bf16* __restrict__ K, float* __restrict__ kpart, int S, int nb) {
  constexpr int CH = D / 8;
  const int blk = blockIdx.x * (64 / CH) + threadIdx.x / CH, c = threadIdx.x % CH;
  if (blk >= nb) return;
  const int64_t bh = blockIdx.y;
  const bf16* src = K + bh * (int64_t)S * D + 8 * c;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int r = 0; r < 64; r++) {
    const int row = blk * 64 + r;
    bf16x8 v;
    if (row < S) v = *(const bf16x8*)(src + (int64_t)row * D);
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] += row < S ? bf2f(v[j]) : 0.f;
  }
  float* dst = kpart + (bh * nb + blk) * D + 8 * c;
  f32x4 lo = {acc[0], acc[1], acc[2], acc[3]}, hi = {acc[4], acc[5], acc[6], acc[7]};
  *(f32x4*)dst = lo;
  *(f32x4*)(dst + 4) = hi;
}
// stage 2: the partials in block order, then the true division by S
__global__ void k_sage_kmean(const float* __restrict__ kpart, float* __restrict__ kmean, int S, int nb, int d) {
  const int c = threadIdx.x;
  const int64_t bh = blockIdx.x;
  float acc = 0.f;
  for (int blk = 0; blk < nb; blk++) acc += kpart[(bh * nb + blk) * d + c];
  kmean[bh * d + c] = acc / (float)S;
}

// one wave per 64-row block of Q (blockIdx.z = 0, no mean) or K (1, minus kbar): amax -> scale -> int8 rows; rows >= S of the Sp-row image are zero.
// A lane's 16-byte chunks all sit in one chunk column (64 % (D / 8) == 0), so its 8 kbar values are loaded once.
template <int D>
__global__ void __launch_bounds__(256) k_sage_quant_qk(const bf16* __restrict__ Q, const bf16* __restrict__ K, const float* __restrict__ kmean,
                                                       int8_t* __restrict__ Qh, int8_t* __restrict__ Kh, float* __restrict__ sq, float* __restrict__ sk,
                                                       int S, int Sp, int nb) {
  constexpr int CH = D / 8;
  const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= nb) return;
  const bool isk = blockIdx.z != 0;
  const int64_t bh = blockIdx.y;
  const bf16* src = (isk ? K : Q) + bh * (int64_t)S * D;
  int8_t* dst = (isk ? Kh : Qh) + bh * (int64_t)Sp * D;
  const int c = lane % CH, r0 = lane / CH;
  float mu[8];
#pragma unroll
  for (int j = 0; j < 8; j++) mu[j] = isk ? kmean[bh * D + 8 * c + j] : 0.f;
  float amax = 0.f;
  for (int it = 0; it < CH; it++) {
    const int row = blk * 64 + it * (64 / CH) + r0;
    if (row < S) {
      const bf16x8 v = *(const bf16x8*)(src + (int64_t)row * D + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf(bf2f(v[j]) - mu[j]));
    }
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax / 127.0f : 1.0f;
  if (lane == 0) (isk ? sk : sq)[bh * nb + blk] = sc;
  for (int it = 0; it < CH; it++) {
    const int row = blk * 64 + it * (64 / CH) + r0;
    u32x2 o;
    o[0] = 0u; o[1] = 0u;
    if (row < S) {
      const bf16x8 v = *(const bf16x8*)(src + (int64_t)row * D + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int q = (int)rintf((bf2f(v[j]) - mu[j]) / sc);
        o[j >> 2] |= (uint32_t)(q & 0xFF) << (8 * (j & 3));
      }
    }
    *(u32x2*)(dst + (int64_t)row * D + 8 * c) = o;
  }
}

// one wave per row of Vt (one (b, h, channel)): amax over the keys < S, sv = amax / 448, e4m3 bytes; columns >= S of the Sp-wide row are zero
__global__ void __launch_bounds__(256) k_sage_quant_v(const bf16* __restrict__ Vt, uint8_t* __restrict__ Vh, float* __restrict__ sv, int S, int Sp, int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16* src = Vt + row * Sp;
  uint8_t* dst = Vh + row * Sp;
  float amax = 0.f;
  for (int k = lane * 8; k < S; k += 512) {
    const bf16x8 v = *(const bf16x8*)(src + k);
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (k + j < S) amax = fmaxf(amax, fabsf(bf2f(v[j])));
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
  if (lane == 0) sv[row] = sc;
  for (int k = lane * 8; k < Sp; k += 512) {
    const bf16x8 v = *(const bf16x8*)(src + k);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = k + j < S ? fminf(fmaxf(bf2f(v[j]) / sc, -448.f), 448.f) : 0.f;
    u32x2 o;
    o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0u, false), true);
    o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0u, false), true);
    *(u32x2*)(dst + k) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// main kernel
// ------------------------------------------------------------------------------------------------
#define SAGE_KB 128      // keys per step (one fp8 MFMA contraction)
#define SAGE_QB 128      // queries per workgroup

__device__ __forceinline__ float xrow16_max(float x) {      // max over lanes l and l ^ 16 (v_permlane16_swap: rows of 16 lanes exchanged pairwise)
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xrow16_sum(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// swizzled byte offset of 16-byte chunk `chunk` of row `row` in an LDS image with ROWB-byte rows (128: 8 chunks, 64: 4 chunks)
template <int ROWB>
__device__ __forceinline__ int sage_off(int row, int chunk) {
  if (ROWB == 128) return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
  return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4);
}

template <int HD>
__global__ void __launch_bounds__(256, HD == 128 ? 1 : 2) k_sage_fwd(const int8_t* __restrict__ Qh, const int8_t* __restrict__ Kh, const uint8_t* __restrict__ Vh,
                                                     const float* __restrict__ sq, const float* __restrict__ sk, const float* __restrict__ sv,
                                                     bf16* __restrict__ O, int64_t ld_o, int H, int S, int Sp, float c2) {
  constexpr int NKK = HD / 64;                 // int8 MFMAs per 16 x 16 score tile
  constexpr int NCT = HD / 16;                 // 16-channel tiles of O^T
  constexpr int KT_BYTES = SAGE_KB * HD;       // Kh tile: 128 key rows of HD bytes
  constexpr int VT_BYTES = HD * SAGE_KB;       // Vh tile: HD channel rows of 128 bytes
  constexpr int BUF = KT_BYTES + VT_BYTES;
  constexpr int KCH = KT_BYTES / 16 / 256;     // 16-byte chunks per thread and tile
  constexpr int VCH = VT_BYTES / 16 / 256;
  constexpr int KCPR = HD / 16;                // chunks per Kh row
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int nb = Sp / 64;
  const int q0 = wg.tile * SAGE_QB + wv * 32;

  const int8_t* Kg = Kh + bh * (int64_t)Sp * HD;
  const uint8_t* Vg = Vh + bh * (int64_t)HD * Sp;

  i32x4 qf[2][NKK];
#pragma unroll
  for (int qt = 0; qt < 2; qt++) {
    const int row = min(q0 + 16 * qt + n, S - 1);
#pragma unroll
    for (int kk = 0; kk < NKK; kk++) qf[qt][kk] = *(const i32x4*)(Qh + (bh * Sp + row) * (int64_t)HD + 64 * kk + 16 * g);
  }
  const float sqc = sq[bh * nb + min(q0 >> 6, nb - 1)];             // the wave's 32 queries lie in one 64-row block

  f32x4 acc[2][NCT];
#pragma unroll
  for (int qt = 0; qt < 2; qt++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[qt][ct][r] = 0.f;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};

  // register staging in two halves that share one register set (KCH == VCH): the next Kh tile travels under the score MFMAs, the next Vh tile under the
  // softmax and the PV MFMAs; the other LDS buffer is free for the whole step
  static_assert(KCH == VCH, "the Kh and Vh halves share the staging registers");
  u32x4 stg[KCH];
  auto load_k = [&](int kt) {
    const int key0 = kt * SAGE_KB;
#pragma unroll
    for (int p = 0; p < KCH; p++) {                        // the Kh tile is contiguous memory: chunk id at byte id * 16; rows >= Sp do not exist -> zeros
      const int id = p * 256 + tid;
      u32x4 z = {0u, 0u, 0u, 0u};
      stg[p] = key0 + id / KCPR < Sp ? *(const u32x4*)(Kg + (int64_t)key0 * HD + (int64_t)id * 16) : z;
    }
  };
  auto load_v = [&](int kt) {
    const int key0 = kt * SAGE_KB;
#pragma unroll
    for (int p = 0; p < VCH; p++) {                        // Vh tile: channel row id / 8, keys key0 + 16 (id % 8) ..; columns >= Sp do not exist -> zeros
      const int id = p * 256 + tid;
      const int kcol = key0 + 16 * (id & 7);
      u32x4 z = {0u, 0u, 0u, 0u};
      stg[p] = kcol < Sp ? *(const u32x4*)(Vg + (int64_t)(id >> 3) * Sp + kcol) : z;
    }
  };
  auto store_k = [&](int buf) {
    char* ks = smem + buf * BUF;
#pragma unroll
    for (int p = 0; p < KCH; p++) {
      const int id = p * 256 + tid;
      const int k = id / KCPR, cc = id % KCPR;
      const int rho = 16 * ((k >> 2) & 7) + 4 * (k >> 5) + (k & 3);      // key 32 a + 4 t + b -> LDS row 16 t + 4 a + b
      *(u32x4*)(ks + sage_off<HD>(rho, cc)) = stg[p];
    }
  };
  auto store_v = [&](int buf) {
    char* vs = smem + buf * BUF + KT_BYTES;
#pragma unroll
    for (int p = 0; p < VCH; p++) {
      const int id = p * 256 + tid;
      *(u32x4*)(vs + sage_off<128>(id >> 3, id & 7)) = stg[p];
    }
  };

  const int nkt = (S + SAGE_KB - 1) / SAGE_KB;
  load_k(0);
  store_k(0);
  load_v(0);
  store_v(0);
  __syncthreads();

  auto tile = [&](int kt, auto masked_c) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const int buf = kt & 1;
    if (kt + 1 < nkt) load_k(kt + 1);
    const char* ks = smem + buf * BUF;
    const char* vs = ks + KT_BYTES;
    const int key0 = kt * SAGE_KB;

    i32x4 s[2][8];
#pragma unroll
    for (int t = 0; t < 8; t++)
#pragma unroll
      for (int kk = 0; kk < NKK; kk++) {                   // one Kh fragment read feeds both query tiles
        const i32x4 kf = *(const i32x4*)(ks + sage_off<HD>(16 * t + n, 4 * kk + g));
#pragma unroll
        for (int qt = 0; qt < 2; qt++) {
          i32x4 z = {0, 0, 0, 0};
          s[qt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[qt][kk], kk == 0 ? z : s[qt][t], 0, 0, 0);
        }
      }
    if (kt + 1 < nkt) { store_k(buf ^ 1); load_v(kt + 1); }
    // the lane's keys of this step are key0 + 32 g + 4 t + r: one 64-key block, one sk
    const float f = sqc * sk[bh * nb + min((key0 + 32 * g) >> 6, nb - 1)] * c2;
    const int kbase = key0 + 32 * g;
    i32x8 pf[2];
#pragma unroll
    for (int qt = 0; qt < 2; qt++) {
      int imax = INT32_MIN;
      bool any = !MASKED;
#pragma unroll
      for (int t = 0; t < 8; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (MASKED) {
            if (kbase + 4 * t + r < S) { imax = max(imax, s[qt][t][r]); any = true; }
          } else {
            imax = max(imax, s[qt][t][r]);
          }
        }
      float mt = any ? (float)imax * f : -INFINITY;        // f > 0: max(f * s) = f * max(s)
      mt = xhalf_max(xrow16_max(mt));
      const float m_new = fmaxf(m_run[qt], mt);
      const float alpha = fast_exp2(m_run[qt] - m_new);
      m_run[qt] = m_new;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc[qt][ct][r] *= alpha;
      }
      const float m8 = m_new - 8.f;                         // e = exp2(s2 - m + 8) = p * 2^8 <= 256 < 448: cannot saturate e4m3
      float ls = 0.f;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          e[r] = fast_exp2(fmaf((float)s[qt][t][r], f, -m8));
          if (MASKED && kbase + 4 * t + r >= S) e[r] = 0.f;
        }
        ls += (e[0] + e[1]) + (e[2] + e[3]);
        pf[qt][t] = (int)__builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], 0u, false), true);
      }
      l_run[qt] = l_run[qt] * alpha + ls;
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      i32x8 vf;
      *(i32x4*)&vf = *(const i32x4*)(vs + sage_off<128>(16 * ct + n, 2 * g));
      *((i32x4*)&vf + 1) = *(const i32x4*)(vs + sage_off<128>(16 * ct + n, 2 * g + 1));
#pragma unroll
      for (int qt = 0; qt < 2; qt++)
        acc[qt][ct] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[qt], acc[qt][ct], 0 /* A = e4m3 */, 0 /* B = e4m3 */, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }
    if (kt + 1 < nkt) store_v(buf ^ 1);
    __syncthreads();
  };
  const int nfull = S / SAGE_KB;
  for (int kt = 0; kt < nfull; kt++) tile(kt, std::false_type{});
  for (int kt = nfull; kt < nkt; kt++) tile(kt, std::true_type{});

  // O^T tile ct of query tile qt: lane (n, g) holds channels 16 ct + 4 g + r of query q0 + 16 qt + n
#pragma unroll
  for (int qt = 0; qt < 2; qt++) {
    const float l_tot = xhalf_sum(xrow16_sum(l_run[qt]));   // = 2^8 * l
    const int q = q0 + 16 * qt + n;
    if (q < S) {
      bf16* orow = O + ((int64_t)b * S + q) * ld_o + (int64_t)head * HD + 4 * g;
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        const f32x4 svv = *(const f32x4*)(sv + bh * HD + 16 * ct + 4 * g);
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = f2bf(acc[qt][ct][r] * svv[r] / l_tot);
        *(bf16x4*)(orow + 16 * ct) = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int sage_shape_ok(const char* fn, int B, int H, int S, int Sp, int d) {
  if (d != 64 && d != 128) { st355_set_error("%s: head_dim %d not built (64 or 128)", fn, d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && H > 0 && S > 0 && Sp % 64 == 0 && Sp >= S && Sp - S < 64 && (int64_t)B * H < 65536, "%s: bad shape B=%d H=%d S=%d Sp=%d (Sp = ceil64(S))",
             fn, B, H, S, Sp);
  return ST355_OK;
}

extern "C" size_t st355_attn_sage_workspace(int B, int H, int S, int d) {
  if (B <= 0 || H <= 0 || S <= 0 || (d != 64 && d != 128)) return 0;
  return sage_ws(B, H, (S + 63) / 64 * 64, d).total;
}

extern "C" int st355_attn_sage_quantize(void* stream, const void* Q, const void* K, const void* Vt, void* workspace, int B, int H, int S, int Sp, int d) {
  ST_REQUIRE(Q && K && Vt && workspace && (uintptr_t)workspace % 16 == 0, "attn_sage_quantize: null pointer or a workspace off the 16-byte grid");
  if (const int rc = sage_shape_ok("attn_sage_quantize", B, H, S, Sp, d)) return rc;
  const SageWs w = sage_ws(B, H, Sp, d);
  char* ws = (char*)workspace;
  const int nb = Sp / 64, BH = B * H;
  const double elems = 3.0 * BH * (double)Sp * d;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 4.0 * elems, 6.0 * elems);
  hipStream_t st = (hipStream_t)stream;
  float* kpart = (float*)(ws + w.kpart);
  float* kmean = (float*)(ws + w.kmean);
  if (d == 128) hipLaunchKernelGGL(k_sage_kpart<128>, dim3((nb + 3) / 4, BH), dim3(64), 0, st, (const bf16*)K, kpart, S, nb);
  else hipLaunchKernelGGL(k_sage_kpart<64>, dim3((nb + 7) / 8, BH), dim3(64), 0, st, (const bf16*)K, kpart, S, nb);
  hipLaunchKernelGGL(k_sage_kmean, dim3(BH), dim3(d), 0, st, (const float*)kpart, kmean, S, nb, d);
  const dim3 gq((nb + 3) / 4, BH, 2);
  if (d == 128)
    hipLaunchKernelGGL(k_sage_quant_qk<128>, gq, dim3(256), 0, st, (const bf16*)Q, (const bf16*)K, (const float*)kmean, (int8_t*)(ws + w.qh), (int8_t*)(ws + w.kh),
                       (float*)(ws + w.sq), (float*)(ws + w.sk), S, Sp, nb);
  else
    hipLaunchKernelGGL(k_sage_quant_qk<64>, gq, dim3(256), 0, st, (const bf16*)Q, (const bf16*)K, (const float*)kmean, (int8_t*)(ws + w.qh), (int8_t*)(ws + w.kh),
                       (float*)(ws + w.sq), (float*)(ws + w.sk), S, Sp, nb);
  const int64_t rows = (int64_t)BH * d;
  hipLaunchKernelGGL(k_sage_quant_v, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const bf16*)Vt, (uint8_t*)(ws + w.vh), (float*)(ws + w.sv), S, Sp, rows);
  return st355_check_launch("attn_sage_quantize");
}

extern "C" int st355_attn_sage_fwd(void* stream, const void* workspace, void* O, int64_t ld_o, int B, int H, int S, int Sp, int d, float scale) {
  ST_REQUIRE(workspace && O && (uintptr_t)workspace % 16 == 0 && (uintptr_t)O % 8 == 0, "attn_sage_fwd: null pointer, a workspace off the 16-byte grid or O off the 8-byte grid");
  if (const int rc = sage_shape_ok("attn_sage_fwd", B, H, S, Sp, d)) return rc;
  ST_REQUIRE(ld_o % 4 == 0 && ld_o >= (int64_t)H * d && scale > 0.f, "attn_sage_fwd: bad ld_o=%lld or scale", (long long)ld_o);
  const SageWs w = sage_ws(B, H, Sp, d);
  const char* ws = (const char*)workspace;
  const double flops = 4.0 * (double)B * H * (double)S * S * d;
  ProfScope ps(stream, ST355_K_ATTN_FWD, flops, 3.0 * B * H * (double)Sp * d + 2.0 * B * H * (double)S * d);
  const dim3 grid((S + SAGE_QB - 1) / SAGE_QB, H, B);
  const int lds = 2 * 2 * SAGE_KB * d;
  const float c2 = scale * LOG2E;
#define ST355_SAGE_LAUNCH(HD_)                                                                                                              \
  do {                                                                                                                                     \
    static St355AttrOnce set;                                                                                                               \
    if (set.need()) { hipFuncSetAttribute((const void*)k_sage_fwd<HD_>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); }                 \
    hipLaunchKernelGGL(k_sage_fwd<HD_>, grid, dim3(256), lds, (hipStream_t)stream, (const int8_t*)(ws + w.qh), (const int8_t*)(ws + w.kh), \
                       (const uint8_t*)(ws + w.vh), (const float*)(ws + w.sq), (const float*)(ws + w.sk), (const float*)(ws + w.sv), (bf16*)O, ld_o, H, S, Sp, c2); \
  } while (0)
  if (d == 128) ST355_SAGE_LAUNCH(128);
  else ST355_SAGE_LAUNCH(64);
#undef ST355_SAGE_LAUNCH
  return st355_check_launch("attn_sage_fwd");
}

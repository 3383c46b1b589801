// attention_wide.hip — fused attention for heads wider than 128 channels (SD 1.x: 8 heads over 1280 channels, head_dim 160), forward and backward, on
// TOKEN-MAJOR operands: every q / k / v / dO / O / dq / dk / dv pointer is the first column of a column block of a [B*S, ld] projection buffer (row b*S + i
// holds head h at columns h*HD .. h*HD + HD - 1), i.e. the fused qkv / q / kv Linears' outputs and to_out's input as they are.  No head-split, padded,
// transposed or head-major copy exists on either side.
//   O  = softmax(scale Q K^T) V,   lse2 = log2 sum_j exp(scale q.k_j)                                  (log2 convention of attn_common.h)
//   dV = P^T dO,  dS = P o (dP - delta),  dP = dO V^T,  delta_i = sum_j P_ij dP_ij,  dQ = scale dS K,  dK = scale dS^T Q
//
// gfx950 design (v_mfma_f32_32x32x16_bf16, fp32 accumulation, fragment maps of attn_common.h), kernels templated on HD (HD % 32 == 0; 160 instantiated):
//   * one 64-row tile image serves all three kernels: 64 token rows x HD channels copied straight from the token-major rows, row pitch 2 HD bytes (320 at
//     HD 160: 80 banks = 16 mod 64, so rows r, r+4, r+8, r+12 start on the same bank).  Swizzle: the 16-byte chunk index is XORed with (row >> 2) & 3 — it
//     stays inside an aligned group of 4 chunks (a bijection on the HD/8 chunks of a row), and the 16 rows of a 16-lane ds_read_b128 group then land on 16
//     distinct 4-bank slots: conflict-free at HD 160 (and at every HD = 32 mod 64; HD 192 / 256 stay correct but want their own XOR term to be conflict-free).
//     The same image is read two ways: row fragments (ds_read_b128: rows are the MFMA A rows, fetched in perm23 order) and TRANSPOSED fragments
//     (ds_read_b64_tr_b16 pairs: channels are the A rows, 8 consecutive token rows the contraction slots).  For the transposed reads (row >> 2) & 3 is the same
//     for the four rows of a 4 x 16 block, so the XOR term is lane-uniform per read; the 32 lanes of a half wave cover all 64 banks once.
//   * forward  k_attn_wide_fwd: workgroup = 4 waves x 32 queries, 64-key tiles.  S^T = K Q^T (K row fragments x Q fragments held in registers): a lane owns a
//     query column, online softmax in registers, exp(S^T) registers are the B operand of O^T += V^T P^T (V^T fragments by transposing reads of the row-major V
//     tile) — P never leaves the register file.  Next tile's global loads are issued before the MFMA work and written to the other LDS buffer after it.
//     LDS 2 x (K 20 KiB + V 20 KiB) = 80 KiB at HD 160.  Registers: Q 40, O^T 80, scores 32, staging 40 + the fragment reads in flight = 374 (254 VGPR +
//     120 AGPR), so ONE workgroup per CU (1 wave per SIMD); held to 256 the compiler spills 20 registers into the tile loop, which costs more than the second
//     resident workgroup gives at these levels (<= 1024 tokens: at most a few workgroups per CU in the whole grid).
//   * backward k_attn_wide_dq: the forward's shape, two passes over the key tiles.  Pass A recomputes P = exp2(s2 - lse2) and dP^T = V dO^T and sums
//     delta = sum_j P dP in fp32 (P un-rounded); pass B recomputes both with the same instructions, dS = P (dP - delta), dQ^T += K^T dS^T (K^T fragments by
//     transposing reads of the K tile already staged for the scores).  delta never comes from the bf16 O (the backward does not read O at all), so the common
//     component of the keys cancels in dQ / dK as in exact arithmetic.  Writes dQ x scale token-major and delta [B, H, Sq] fp32 to the workspace.
//     Registers Q 40 + dO 40 + dQ^T 80 + S / dP 64 + staging 40: one workgroup per CU (launch bound 256 threads, 1 wave per SIMD), LDS 80 KiB.
//   * backward k_attn_wide_dkv: the mirror image — workgroup = 4 waves x 32 KEYS (K and V fragments in registers), 64-QUERY tiles of Q and dO staged in LDS with
//     their lse2 / delta (512 bytes per buffer).  S = Q K^T, dP = dO V^T: a lane owns a key column; dV^T += dO^T P, dK^T += Q^T dS (transposing reads of the
//     staged dO / Q tiles).  LDS 2 x (20 + 20 + 0.5) KiB = 81 KiB, one workgroup per CU (dK^T + dV^T alone are 160 accumulator registers; 392 in all, the
//     two 32-query halves of a tile run as a rolled loop: unrolled, the hoisted fragment reads spill 68 registers).
//   No atomics: every output element has one owner and a fixed summation order, so launches are bit-identical.  Ragged query / key tails: loads clamp the row,
//   masked scores give P = 0 exactly, stores are guarded.
#include <type_traits>
#include "attn_common.h"

#define WIDE_THREADS 256
#define WIDE_ROWS 64      // token rows per staged tile

template <int HD>
struct WideTile {
  static_assert(HD % 32 == 0, "attention_wide: head_dim must be a multiple of 32");
  static constexpr int ROWB = HD * 2;                              // row pitch, bytes
  static constexpr int NCH = HD / 8;                               // 16-byte chunks per row
  static constexpr int BYTES = WIDE_ROWS * ROWB;
  static constexpr int PER = WIDE_ROWS * NCH / WIDE_THREADS;       // chunks per thread (= HD / 32)
  static constexpr int NKS = HD / 16, NDT = HD / 32;

  static __device__ __forceinline__ int off(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 2) & 3)) << 4); }

  // rows row0 .. row0 + 63 of one head's column block (base = block start + head * HD of batch row 0); rows past nrows - 1 re-read the last valid row
  static __device__ __forceinline__ void load(bf16x8 (&reg)[PER], const bf16* base, int64_t ld, int row0, int nrows, int tid) {
#pragma unroll
    for (int p = 0; p < PER; p++) {
      const int id = p * WIDE_THREADS + tid;
      const int row = id / NCH, c = id - row * NCH;
      reg[p] = *(const bf16x8*)(base + (int64_t)min(row0 + row, nrows - 1) * ld + c * 8);
    }
  }
  static __device__ __forceinline__ void store(const bf16x8 (&reg)[PER], char* lds, int tid) {
#pragma unroll
    for (int p = 0; p < PER; p++) {
      const int id = p * WIDE_THREADS + tid;
      const int row = id / NCH, c = id - row * NCH;
      *(bf16x8*)(lds + off(row, c)) = reg[p];
    }
  }
  // MFMA A fragment, rows = token rows: A[i = row][k = 16 ks + 8 h + 0..7]
  static __device__ __forceinline__ bf16x8 rows(const char* lds, int row, int ks, int h) { return *(const bf16x8*)(lds + off(row, 2 * ks + h)); }
  // per-lane base of the transposed fragments.  lane = 32 h + 16 ih + 4 r + s supplies 4 contiguous channels 16 ih + 4 s .. + 3 of token row 8 h + r (+ 4 for
  // the second read) and receives channel 16 ih + (lane & 15) of 4 token rows: A[i = channel 32 dt + (lane & 31)][k = token r0 + 8 h + 0..7].
  static __device__ __forceinline__ int tr_base(int lane, int second) {
    const int h = lane >> 5, ih = (lane >> 4) & 1, r = (lane >> 2) & 3, s = lane & 3;
    return off(8 * h + r + 4 * second, 2 * ih + (s >> 1)) + (s & 1) * 8;
  }
  // r0: a multiple of 16 (the XOR term of row r0 + x equals that of x); d tile dt adds 4 chunks, above the two swizzled bits
  static __device__ __forceinline__ bf16x8 cols(const char* lds, int tr0, int tr1, int r0, int dt) {
    const char* p = lds + r0 * ROWB + dt * 64;
    return lds_tr16x2(p + tr0, p + tr1);
  }
};

// a head's fragments of one token row held in registers as the MFMA B operand: B[k = 16 ks + 8 h + 0..7][n = lane & 31]
template <int HD>
__device__ __forceinline__ void wide_row_frags(bf16x8 (&f)[HD / 16], const bf16* row, int h) {
#pragma unroll
  for (int ks = 0; ks < HD / 16; ks++) f[ks] = *(const bf16x8*)(row + 16 * ks + 8 * h);
}

// accumulators acc[dt][4 a + b] = X^T[channel 32 dt + 8 a + 4 h + b][token lane & 31] -> one token-major row, scaled
template <int HD>
__device__ __forceinline__ void wide_store_row(bf16* row, const f32x16 (&acc)[HD / 32], float mul, int h) {
#pragma unroll
  for (int dt = 0; dt < HD / 32; dt++)
#pragma unroll
    for (int a = 0; a < 4; a++) {
      bf16x4 o;
#pragma unroll
      for (int bb = 0; bb < 4; bb++) o[bb] = f2bf(acc[dt][4 * a + bb] * mul);
      *(bf16x4*)(row + 32 * dt + 8 * a + 4 * h) = o;
    }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(WIDE_THREADS, 1) k_attn_wide_fwd(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                   const bf16* __restrict__ V, int64_t ld_v, bf16* __restrict__ O, int64_t ld_o,
                                                                   float* __restrict__ lse2, int H, int Sq, int Sk, float scale2) {
  using TL = WideTile<HD>;
  constexpr int NKS = TL::NKS, NDT = TL::NDT, BUF = 2 * TL::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int q0 = wg.tile * 128 + wv * 32;
  const int qi = min(q0 + l31, Sq - 1);
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + (int64_t)head * HD;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + (int64_t)head * HD;

  bf16x8 qf[NKS];
  wide_row_frags<HD>(qf, Q + ((int64_t)b * Sq + qi) * ld_q + (int64_t)head * HD, h);
  f32x16 acc_o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc_o[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  bf16x8 kreg[TL::PER], vreg[TL::PER];
  const int nkt = (Sk + WIDE_ROWS - 1) / WIDE_ROWS;
  const int krow_p = perm23(l31);
  const int tr0 = TL::tr_base(lane, 0), tr1 = TL::tr_base(lane, 1);

  TL::load(kreg, Kg, ld_k, 0, Sk, tid);
  TL::load(vreg, Vg, ld_v, 0, Sk, tid);
  TL::store(kreg, smem, tid);
  TL::store(vreg, smem + TL::BYTES, tid);
  __syncthreads();

  auto tile = [&](int kt, auto masked_c) {
    constexpr bool MASKED = decltype(masked_c)::value;      // ragged last tile: scores are rewritten in place, already scaled
    const int buf = kt & 1;
    if (kt + 1 < nkt) {
      TL::load(kreg, Kg, ld_k, (kt + 1) * WIDE_ROWS, Sk, tid);
      TL::load(vreg, Vg, ld_v, (kt + 1) * WIDE_ROWS, Sk, tid);
    }
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TL::BYTES;
    const int key0 = kt * WIDE_ROWS;

    f32x16 sacc[2];
    float mt = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < 2; sb++) {
#pragma unroll
      for (int r = 0; r < 16; r++) sacc[sb][r] = 0.f;
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++)
        sacc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::rows(ks, 32 * sb + krow_p, ks_, h), qf[ks_], sacc[sb], 0, 0, 0);
    }
#pragma unroll
    for (int sb = 0; sb < 2; sb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        if (MASKED) {
          float s = sacc[sb][r] * scale2;
          if (key0 + 32 * sb + acc_row(r, h) >= Sk) s = -INFINITY;
          sacc[sb][r] = s;
        }
        mt = fmaxf(mt, sacc[sb][r]);
      }
    const float psc = MASKED ? 1.f : scale2;               // plain tiles keep the RAW score: the scale rides in the exponent's fma
    if (!MASKED) mt *= scale2;                             // scale2 > 0
    mt = xhalf_max(mt);
    const float m_new = fmaxf(m_run, mt);
    const float alpha = fast_exp2(m_run - m_new);
    m_run = m_new;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
      for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc_o[dt][r] *= alpha;
    }
    float ls[2] = {0.f, 0.f};
#pragma unroll
    for (int sb = 0; sb < 2; sb++)
#pragma unroll
      for (int m = 0; m < 2; m++) {
        float e[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
          e[r] = fast_exp2(fmaf(sacc[sb][8 * m + r], psc, -m_new));
          ls[r & 1] += e[r];
        }
        const bf16x8 pf = pack8(e);
#pragma unroll
        for (int dt = 0; dt < NDT; dt++)      // V^T[d = 32 dt + l31][keys 32 sb + 16 m + 8 h + 0..7]
          acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::cols(vs, tr0, tr1, 32 * sb + 16 * m, dt), pf, acc_o[dt], 0, 0, 0);
      }
    l_run = l_run * alpha + (ls[0] + ls[1]);
    if (kt + 1 < nkt) {
      TL::store(kreg, smem + (buf ^ 1) * BUF, tid);
      TL::store(vreg, smem + (buf ^ 1) * BUF + TL::BYTES, tid);
    }
    __syncthreads();
  };
  const int nfull = Sk / WIDE_ROWS;
  for (int kt = 0; kt < nfull; kt++) tile(kt, std::false_type{});
  for (int kt = nfull; kt < nkt; kt++) tile(kt, std::true_type{});

  const float l_tot = xhalf_sum(l_run);
  const int q = q0 + l31;
  if (q < Sq) {
    wide_store_row<HD>(O + ((int64_t)b * Sq + q) * ld_o + (int64_t)head * HD, acc_o, 1.f / l_tot, h);
    if (h == 0) lse2[bh * Sq + q] = m_run + __log2f(l_tot);
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dQ and delta
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(WIDE_THREADS) k_attn_wide_dq(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                               const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ dO, int64_t ld_do,
                                                               const float* __restrict__ lse2, bf16* __restrict__ dQ, int64_t ld_dq,
                                                               float* __restrict__ delta_out, int H, int Sq, int Sk, float scale, float scale2) {
  using TL = WideTile<HD>;
  constexpr int NKS = TL::NKS, NDT = TL::NDT, BUF = 2 * TL::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int q0 = wg.tile * 128 + wv * 32;
  const int qi = min(q0 + l31, Sq - 1);
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + (int64_t)head * HD;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + (int64_t)head * HD;

  bf16x8 qf[NKS], gf[NKS];
  wide_row_frags<HD>(qf, Q + ((int64_t)b * Sq + qi) * ld_q + (int64_t)head * HD, h);
  wide_row_frags<HD>(gf, dO + ((int64_t)b * Sq + qi) * ld_do + (int64_t)head * HD, h);
  const float L = lse2[bh * Sq + qi];
  f32x16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[dt][r] = 0.f;
  float dsum = 0.f, delta = 0.f;

  bf16x8 kreg[TL::PER], vreg[TL::PER];
  const int nkt = (Sk + WIDE_ROWS - 1) / WIDE_ROWS;
  const int krow_p = perm23(l31);
  const int tr0 = TL::tr_base(lane, 0), tr1 = TL::tr_base(lane, 1);

  TL::load(kreg, Kg, ld_k, 0, Sk, tid);
  TL::load(vreg, Vg, ld_v, 0, Sk, tid);
  TL::store(kreg, smem, tid);
  TL::store(vreg, smem + TL::BYTES, tid);
  __syncthreads();

  for (int it = 0; it < 2 * nkt; it++) {          // pass A (delta): it < nkt; pass B (dQ): the same tiles again
    const bool pass_b = it >= nkt;
    const int kt = pass_b ? it - nkt : it;
    const int buf = it & 1;
    if (it + 1 < 2 * nkt) {
      const int kn = it + 1 >= nkt ? it + 1 - nkt : it + 1;
      TL::load(kreg, Kg, ld_k, kn * WIDE_ROWS, Sk, tid);
      TL::load(vreg, Vg, ld_v, kn * WIDE_ROWS, Sk, tid);
    }
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TL::BYTES;
    const int key0 = kt * WIDE_ROWS;
#pragma unroll
    for (int sb = 0; sb < 2; sb++) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++) {          // S^T = K Q^T, dP^T = V dO^T: lane = query column, registers = keys
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::rows(ks, 32 * sb + krow_p, ks_, h), qf[ks_], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::rows(vs, 32 * sb + krow_p, ks_, h), gf[ks_], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float p = fast_exp2(fmaf(s[r], scale2, -L));
        s[r] = key0 + 32 * sb + acc_row(r, h) < Sk ? p : 0.f;
      }
      if (!pass_b) {
#pragma unroll
        for (int r = 0; r < 16; r++) dsum = fmaf(s[r], dp[r], dsum);
      } else {
#pragma unroll
        for (int m = 0; m < 2; m++) {
          float ds[8];
#pragma unroll
          for (int r = 0; r < 8; r++) ds[r] = s[8 * m + r] * (dp[8 * m + r] - delta);
          const bf16x8 dsf = pack8(ds);
#pragma unroll
          for (int dt = 0; dt < NDT; dt++)      // dQ^T[d][q] += K^T[d][keys 32 sb + 16 m + 8 h + 0..7] dS^T[keys][q]
            acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::cols(ks, tr0, tr1, 32 * sb + 16 * m, dt), dsf, acc[dt], 0, 0, 0);
        }
      }
    }
    if (it == nkt - 1) delta = xhalf_sum(dsum);
    if (it + 1 < 2 * nkt) {
      TL::store(kreg, smem + (buf ^ 1) * BUF, tid);
      TL::store(vreg, smem + (buf ^ 1) * BUF + TL::BYTES, tid);
    }
    __syncthreads();
  }
  const int q = q0 + l31;
  if (q < Sq) {
    wide_store_row<HD>(dQ + ((int64_t)b * Sq + q) * ld_dq + (int64_t)head * HD, acc, scale, h);
    if (h == 0) delta_out[bh * Sq + q] = delta;
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dK and dV
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(WIDE_THREADS) k_attn_wide_dkv(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ dO, int64_t ld_do,
                                                                const float* __restrict__ lse2, const float* __restrict__ delta, bf16* __restrict__ dK,
                                                                int64_t ld_dk, bf16* __restrict__ dV, int64_t ld_dv, int H, int Sq, int Sk, float scale,
                                                                float scale2) {
  using TL = WideTile<HD>;
  constexpr int NKS = TL::NKS, NDT = TL::NDT, AUX = 2 * WIDE_ROWS * 4, BUF = 2 * TL::BYTES + AUX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int key0 = wg.tile * 128 + wv * 32;
  const int kj = min(key0 + l31, Sk - 1);
  const bool active = key0 < Sk;                   // wave-uniform: a wave whose 32 keys all lie past Sk only helps staging
  const bf16* Qg = Q + (int64_t)b * Sq * ld_q + (int64_t)head * HD;
  const bf16* Gg = dO + (int64_t)b * Sq * ld_do + (int64_t)head * HD;

  bf16x8 kf[NKS], vf[NKS];
  wide_row_frags<HD>(kf, K + ((int64_t)b * Sk + kj) * ld_k + (int64_t)head * HD, h);
  wide_row_frags<HD>(vf, V + ((int64_t)b * Sk + kj) * ld_v + (int64_t)head * HD, h);
  f32x16 acc_k[NDT], acc_v[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++)
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_k[dt][r] = 0.f; acc_v[dt][r] = 0.f; }

  bf16x8 qreg[TL::PER], greg[TL::PER];
  float areg = 0.f;
  const int nqt = (Sq + WIDE_ROWS - 1) / WIDE_ROWS;
  const int qrow_p = perm23(l31);
  const int tr0 = TL::tr_base(lane, 0), tr1 = TL::tr_base(lane, 1);
  // per query of the tile: threads 0..63 carry lse2 (+inf past Sq: P = exp2(-inf) = 0 exactly), threads 64..127 carry delta (0 past Sq)
  auto load_tile = [&](int qt) {
    TL::load(qreg, Qg, ld_q, qt * WIDE_ROWS, Sq, tid);
    TL::load(greg, Gg, ld_do, qt * WIDE_ROWS, Sq, tid);
    if (tid < 2 * WIDE_ROWS) {
      const int qq = qt * WIDE_ROWS + (tid & (WIDE_ROWS - 1));
      const float* src = tid < WIDE_ROWS ? lse2 : delta;
      const float pad = tid < WIDE_ROWS ? INFINITY : 0.f;
      areg = qq < Sq ? src[bh * Sq + qq] : pad;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * BUF;
    TL::store(qreg, base, tid);
    TL::store(greg, base + TL::BYTES, tid);
    if (tid < 2 * WIDE_ROWS) ((float*)(base + 2 * TL::BYTES))[tid] = areg;
  };
  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int qt = 0; qt < nqt; qt++) {
    const int buf = qt & 1;
    if (qt + 1 < nqt) load_tile(qt + 1);
    const char* qs = smem + buf * BUF;
    const char* gs = qs + TL::BYTES;
    const float* aux = (const float*)(qs + 2 * TL::BYTES);
    if (active) {
#pragma unroll 1
      for (int sb = 0; sb < 2; sb++) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks_ = 0; ks_ < NKS; ks_++) {        // S = Q K^T, dP = dO V^T: lane = key column, registers = queries
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::rows(qs, 32 * sb + qrow_p, ks_, h), kf[ks_], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::rows(gs, 32 * sb + qrow_p, ks_, h), vf[ks_], dp, 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < 2; m++) {
          const int qb = 32 * sb + 16 * m + 8 * h;         // registers 8 m .. 8 m + 7 hold queries qb .. qb + 7 of the tile
          const f32x4 l0 = *(const f32x4*)(aux + qb), l1 = *(const f32x4*)(aux + qb + 4);
          const f32x4 d0 = *(const f32x4*)(aux + WIDE_ROWS + qb), d1 = *(const f32x4*)(aux + WIDE_ROWS + qb + 4);
          float p[8], ds[8];
#pragma unroll
          for (int r = 0; r < 8; r++) {
            const float Lr = r < 4 ? l0[r & 3] : l1[r & 3], Dr = r < 4 ? d0[r & 3] : d1[r & 3];
            p[r] = fast_exp2(fmaf(s[8 * m + r], scale2, -Lr));
            ds[r] = p[r] * (dp[8 * m + r] - Dr);
          }
          const bf16x8 pf = pack8(p), dsf = pack8(ds);
#pragma unroll
          for (int dt = 0; dt < NDT; dt++) {      // dV^T[d][key] += dO^T[d][queries] P[queries][key];  dK^T[d][key] += Q^T[d][queries] dS[queries][key]
            acc_v[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::cols(gs, tr0, tr1, 32 * sb + 16 * m, dt), pf, acc_v[dt], 0, 0, 0);
            acc_k[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TL::cols(qs, tr0, tr1, 32 * sb + 16 * m, dt), dsf, acc_k[dt], 0, 0, 0);
          }
        }
      }
    }
    if (qt + 1 < nqt) store_tile(buf ^ 1);
    __syncthreads();
  }
  const int key = key0 + l31;
  if (key < Sk) {
    wide_store_row<HD>(dK + ((int64_t)b * Sk + key) * ld_dk + (int64_t)head * HD, acc_k, scale, h);
    wide_store_row<HD>(dV + ((int64_t)b * Sk + key) * ld_dv + (int64_t)head * HD, acc_v, 1.f, h);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool wide_block_ok(const void* p, int64_t ld, int H, int d) { return p && ((uintptr_t)p & 15) == 0 && ld % 8 == 0 && ld >= (int64_t)H * d; }

#define WIDE_SET_LDS(KERN, BYTES)                                                                                  \
  do {                                                                                                             \
    static St355AttrOnce set;                                                                                      \
    if (set.need()) hipFuncSetAttribute((const void*)(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES); \
  } while (0)

extern "C" int st355_attn_wide_fwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, void* o, int64_t ld_o,
                                   float* lse2, int B, int H, int Sq, int Sk, int d, float scale) {
  if (d != 160) { st355_set_error("attn_wide_fwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_wide_fwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(lse2 && wide_block_ok(q, ld_q, H, d) && wide_block_ok(k, ld_k, H, d) && wide_block_ok(v, ld_v, H, d) && wide_block_ok(o, ld_o, H, d),
             "attn_wide_fwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * d");
  ProfScope ps(stream, ST355_K_ATTN_FWD, 4.0 * (double)B * H * (double)Sq * Sk * d, 2.0 * (double)B * H * 2.0 * (Sq + Sk) * d);
  constexpr int lds = 2 * 2 * WideTile<160>::BYTES;
  WIDE_SET_LDS(k_attn_wide_fwd<160>, lds);
  hipLaunchKernelGGL(k_attn_wide_fwd<160>, dim3((Sq + 127) / 128, H, B), dim3(WIDE_THREADS), lds, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)k,
                     ld_k, (const bf16*)v, ld_v, (bf16*)o, ld_o, lse2, H, Sq, Sk, scale * LOG2E);
  return st355_check_launch("attn_wide_fwd");
}

extern "C" size_t st355_attn_wide_bwd_workspace(int B, int H, int Sq, int d) {      // delta [B, H, Sq] fp32
  (void)d;
  return B > 0 && H > 0 && Sq > 0 ? (size_t)B * H * Sq * sizeof(float) : 0;
}

extern "C" int st355_attn_wide_bwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* dO,
                                   int64_t ld_do, const float* lse2, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk, void* dv, int64_t ld_dv, void* workspace,
                                   int B, int H, int Sq, int Sk, int d, float scale) {
  if (d != 160) { st355_set_error("attn_wide_bwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_wide_bwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(lse2 && workspace && ((uintptr_t)workspace & 3) == 0, "attn_wide_bwd: null lse2 / workspace");
  ST_REQUIRE(wide_block_ok(q, ld_q, H, d) && wide_block_ok(k, ld_k, H, d) && wide_block_ok(v, ld_v, H, d) && wide_block_ok(dO, ld_do, H, d) &&
                 wide_block_ok(dq, ld_dq, H, d) && wide_block_ok(dk, ld_dk, H, d) && wide_block_ok(dv, ld_dv, H, d),
             "attn_wide_bwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * d");
  float* delta = (float*)workspace;
  const float scale2 = scale * LOG2E;
  const double fl_unit = 2.0 * (double)B * H * (double)Sq * Sk * d;
  {
    ProfScope ps(stream, ST355_K_ATTN_BWD_DQ, 5.0 * fl_unit, 2.0 * (double)B * H * (3.0 * Sq + 2.0 * Sk) * d);
    constexpr int lds = 2 * 2 * WideTile<160>::BYTES;
    WIDE_SET_LDS(k_attn_wide_dq<160>, lds);
    hipLaunchKernelGGL(k_attn_wide_dq<160>, dim3((Sq + 127) / 128, H, B), dim3(WIDE_THREADS), lds, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)k,
                       ld_k, (const bf16*)v, ld_v, (const bf16*)dO, ld_do, lse2, (bf16*)dq, ld_dq, delta, H, Sq, Sk, scale, scale2);
    const int rc = st355_check_launch("attn_wide_dq");
    if (rc) return rc;
  }
  ProfScope ps(stream, ST355_K_ATTN_BWD_DKV, 4.0 * fl_unit, 2.0 * (double)B * H * (2.0 * Sq + 4.0 * Sk) * d);
  constexpr int lds = 2 * (2 * WideTile<160>::BYTES + 2 * WIDE_ROWS * 4);
  WIDE_SET_LDS(k_attn_wide_dkv<160>, lds);
  hipLaunchKernelGGL(k_attn_wide_dkv<160>, dim3((Sk + 127) / 128, H, B), dim3(WIDE_THREADS), lds, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)k,
                     ld_k, (const bf16*)v, ld_v, (const bf16*)dO, ld_do, lse2, delta, (bf16*)dk, ld_dk, (bf16*)dv, ld_dv, H, Sq, Sk, scale, scale2);
  return st355_check_launch("attn_wide_dkv");
}

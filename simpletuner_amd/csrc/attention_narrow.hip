// attention_narrow.hip — fused attention for heads of 40 and 80 channels (SD 1.x: 8 heads over 320 / 640 channels), forward and backward, on TOKEN-MAJOR
// operands in the layout of attention_wide.hip: every q / k / v / o / o_res / dO / dq / dk / dv pointer is the first column of a column block of a [B*S, ld]
// projection buffer (row b*S + i holds head h at columns h*HD .. h*HD + HD - 1).  No head-split, zero-padded, transposed or head-major copy on either side.
//   O  = softmax(scale Q K^T) V,   lse2 = log2 sum_j exp(scale q.k_j),   o_res = bf16(O_fp32 - bf16(O))         (log2 convention of attn_common.h)
//   dV = P^T dO,  dS = P o (dP - delta),  dP = dO V^T,  delta_i = sum_c dO_ic (O_ic + o_res_ic),  dQ = scale dS K,  dK = scale dS^T Q
//
// gfx950 design (v_mfma_f32_16x16x32_bf16, fp32 accumulation), kernels templated on HD (HD % 8 == 0, HD <= 96; 40 and 80 instantiated).
// Fragment maps of the 16x16x32 MFMA (lane l, g = l >> 4, n = l & 15):  A[i = n][k = 8 g + 0..7],  B[k = 8 g + 0..7][n],  C[i = 4 g + r][n] in register r.
//   * channel tiling: the output channels are ceil(HD / 16) tiles of 16 (3 at HD 40, 48 rows of which 40 are stored; exactly 5 at HD 80); the score contraction
//     is ceil(HD / 32) steps of 32 (32 + an 8-channel tail at HD 40; 32 + 32 + a 16-channel tail at HD 80).  In the tail step the lane groups whose 8 channels
//     lie past HD hold ZEROS MADE IN REGISTERS on both operands: the columns right of a head belong to the next head or lie past the row, and are never loaded.
//   * one 64-row tile image serves all three kernels: 64 token rows x HD channels copied in 16-byte chunks straight from the token-major rows (5 or 10 chunks
//     per row: 320 / 640 chunks over 256 threads, the chunk index is guarded).  Row pitch = an ODD number of chunks: 5 (80 bytes) at HD 40 as it is, 11 (176
//     bytes, one pad chunk never written or read) at HD 80 — 160 bytes would put rows r and r + 8 on the same banks.  Bank model of attention_wide.hip:
//       - row fragments (ds_read_b128; lane (n, g) reads chunk 4 ks + g of row pi(n)): a 16-lane group reads the 16 rows of a 16-row tile, whose 4-bank
//         slots are (pitch * row + chunk) mod 16 — a bijection of the rows for an odd pitch: conflict-free, no swizzle.
//       - transposed fragments (ds_read_b64_tr_b16 pairs; channels are the A rows, token rows the contraction slots): a half wave reads 8 rows x 32 bytes;
//         a row covers the two 8-byte-pair slots (pitch * row) mod 16 and the next one, so 8 CONSECUTIVE rows would collide two-way (rows 0 and 3 at pitch 5).
//         Hence the row order pi(m) = 2 (m & 7) + (m >> 3) of a 16-row tile: lane groups 0 / 1 (one half wave) own the even rows, groups 2 / 3 the odd rows,
//         the slots pitch * 2 m' mod 16 of a half wave are all even and distinct: conflict-free for every odd pitch.  pi is applied where a tile's rows
//         are the A rows of a score MFMA (free: the 16 lanes of a group still read 16 distinct rows), and the transposed reads fetch the rows in that order.
//   * fragment chaining: scores are computed transposed (S^T = K Q^T: a lane owns a query column n, its 4 registers of the 16-key tile t hold the keys
//     16 t + pi(4 g + r)).  The exp2 registers of the two tiles 2 p and 2 p + 1 are the 8 contraction slots 8 g + 0..7 of the B operand of
//     O^T += V^T P^T as they are; the same key order is what the transposed V reads deliver (first read: rows pi(4 g + 0..3) of tile 2 p, second: of tile
//     2 p + 1).  P (and dS in the backward) never leaves the register file, and no lane exchange is needed.
//   * work split: a workgroup is 4 waves x 32 queries (forward, dQ; two 16-query column tiles per wave, each A fragment read from LDS feeds two MFMAs) or
//     4 waves x 32 keys (dK / dV) over 64-row staged tiles, double-buffered: the next tile's global loads are issued before the MFMA work and written to the
//     other LDS buffer after it.  Grid (tiles, H, B) through attn_wg_map().  LDS: forward / dQ 2 x (K + V) = 20 KiB at HD 40, 44 KiB at HD 80; dK / dV
//     2 x (Q + dO + 512 bytes of lse2 / delta) = 21 / 45 KiB.  Launch bound 256 threads x 2 workgroups per CU (2 waves per SIMD); registers, scratch (0) and
//     occupancy as compiled are recorded in profiles/attn_narrow_kernel_stats.md.
//   * delta comes from sum_c dO (O + o_res) in fp32, formed in the dQ kernel's prologue from the rows the lane already owns and written to the workspace for
//     dK / dV: at 4096 keys a second pass over the keys (attention_wide.hip's dQ) would be 4 of 10 matmul units.  o_res == nullptr: delta from the bf16 O alone.
//   No atomics: every output element has one owner and a fixed summation order, so launches are bit-identical.  Ragged query / key tails, any Sq, Sk >= 1:
//   loads clamp the row, masked scores give P = 0 exactly, stores are guarded.
#include <type_traits>
#include "attn_common.h"

#define NARROW_THREADS 256
#define NARROW_ROWS 64      // token rows per staged tile

#define NARROW_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

// row order of a 16-row tile as MFMA A rows / transposed-read rows (see the header): even rows first
__device__ __forceinline__ int narrow_pi(int m) { return 2 * (m & 7) + (m >> 3); }

// all-reduce over the four lanes n, n + 16, n + 32, n + 48 that share a column (v_permlane16_swap + v_permlane32_swap: VALU, no LDS round trip)
__device__ __forceinline__ float quad_max(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_max(fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1])));
}
__device__ __forceinline__ float quad_sum(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_sum(__uint_as_float(r[0]) + __uint_as_float(r[1]));
}

template <int HD>
struct NarrowTile {
  static_assert(HD % 8 == 0 && HD >= 8 && HD <= 96, "attention_narrow: head_dim must be a multiple of 8, at most 96");
  static constexpr int NCH = HD / 8;                               // 16-byte chunks per row
  static constexpr int ROWB = (NCH | 1) * 16;                      // row pitch, bytes: an odd number of chunks
  static constexpr int BYTES = NARROW_ROWS * ROWB;
  static constexpr int TOTAL = NARROW_ROWS * NCH;                  // chunks per tile
  static constexpr int PER = (TOTAL + NARROW_THREADS - 1) / NARROW_THREADS;
  static constexpr int NKS = (HD + 31) / 32;                       // contraction steps of the score products
  static constexpr int NCT = (HD + 15) / 16;                       // 16-channel output tiles

  // rows row0 .. row0 + 63 of one head's column block (base = block start + head * HD of batch row 0); rows past nrows - 1 re-read the last valid row
  static __device__ __forceinline__ void load(bf16x8 (&reg)[PER], const bf16* base, int64_t ld, int row0, int nrows, int tid) {
#pragma unroll
    for (int p = 0; p < PER; p++) {
      const int id = p * NARROW_THREADS + tid;
      if ((p + 1) * NARROW_THREADS <= TOTAL || id < TOTAL) {
        const int row = id / NCH, c = id - row * NCH;
        reg[p] = *(const bf16x8*)(base + (int64_t)min(row0 + row, nrows - 1) * ld + c * 8);
      }
    }
  }
  static __device__ __forceinline__ void store(const bf16x8 (&reg)[PER], char* lds, int tid) {
#pragma unroll
    for (int p = 0; p < PER; p++) {
      const int id = p * NARROW_THREADS + tid;
      if ((p + 1) * NARROW_THREADS <= TOTAL || id < TOTAL) {
        const int row = id / NCH, c = id - row * NCH;
        *(bf16x8*)(lds + row * ROWB + c * 16) = reg[p];
      }
    }
  }
};

// per-lane LDS offsets of the two fragment kinds
template <int HD>
struct NarrowLane {
  using TL = NarrowTile<HD>;
  int row_off;         // row fragments: byte offset of row pi(n) + this lane's chunk g of contraction step 0
  int tail_off;        // ... of the last contraction step (chunk clamped into the row)
  bool tail_live;      // the lane's 8 channels of the last contraction step lie inside the head
  int tr_off;          // transposed fragments: row pi(4 g + i'), channels 4 s .. 4 s + 3 (lane = 16 g + 4 i' + s)
  int tr_last;         // ... of the last channel tile (channels clamped into the row: the lanes that receive channels >= HD are never stored)
  __device__ __forceinline__ NarrowLane(int lane) {
    const int g = lane >> 4, n = lane & 15, ip = (lane >> 2) & 3, s = lane & 3;
    const int c_tail = 4 * (TL::NKS - 1) + g;
    row_off = narrow_pi(n) * TL::ROWB + g * 16;
    tail_live = c_tail < TL::NCH;
    tail_off = narrow_pi(n) * TL::ROWB + min(c_tail, TL::NCH - 1) * 16;
    tr_off = narrow_pi(4 * g + ip) * TL::ROWB + s * 8;
    tr_last = narrow_pi(4 * g + ip) * TL::ROWB + min(16 * (TL::NCT - 1) + 4 * s, HD - 4) * 2;
  }
  // MFMA A fragment, rows = token rows of the 16-row tile t: A[i = n -> row 16 t + pi(n)][k = channels 32 ks + 8 g + 0..7], zeros past the head
  __device__ __forceinline__ bf16x8 rows(const char* lds, int t, int ks) const {
    const char* p = lds + t * 16 * TL::ROWB;
    if (32 * ks + 32 <= HD) return *(const bf16x8*)(p + row_off + ks * 64);
    const bf16x8 x = *(const bf16x8*)(p + tail_off);
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return tail_live ? x : z;
  }
  // MFMA A fragment, rows = channels of tile ct: A[i = n -> channel 16 ct + n][k = 8 g + j -> token row 32 p + 16 (j >> 2) + pi(4 g + (j & 3))]
  __device__ __forceinline__ bf16x8 cols(const char* lds, int p, int ct) const {
    const char* q = lds + p * 32 * TL::ROWB + (16 * ct + 16 <= HD ? tr_off + ct * 32 : tr_last);
    return lds_tr16x2(q, q + 16 * TL::ROWB);
  }
};

// a head's fragments of one token row held in registers as the MFMA B operand: B[k = channels 32 ks + 8 g + 0..7][n], zeros past the head (never loaded)
template <int HD>
__device__ __forceinline__ void narrow_row_frags(bf16x8 (&f)[NarrowTile<HD>::NKS], const bf16* row, int g) {
#pragma unroll
  for (int ks = 0; ks < NarrowTile<HD>::NKS; ks++) {
    bf16x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (32 * ks + 32 <= HD || 32 * ks + 8 * g < HD) x = *(const bf16x8*)(row + 32 * ks + 8 * g);
    f[ks] = x;
  }
}

// accumulators acc[ct][r] = X^T[channel 16 ct + 4 g + r][token n] -> one token-major row, scaled; res: the rounding residual of the same values (or null)
template <int HD>
__device__ __forceinline__ void narrow_store_row(bf16* row, bf16* res, const f32x4 (&acc)[NarrowTile<HD>::NCT], float mul, int g) {
#pragma unroll
  for (int ct = 0; ct < NarrowTile<HD>::NCT; ct++) {
    const int c = 16 * ct + 4 * g;
    if (16 * ct + 16 <= HD || c < HD) {
      bf16x4 o, e;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float x = acc[ct][r] * mul;
        o[r] = f2bf(x);
        e[r] = f2bf(x - bf2f(o[r]));
      }
      *(bf16x4*)(row + c) = o;
      if (res) *(bf16x4*)(res + c) = e;
    }
  }
}

// key (or query) of a 16-row tile held by accumulator register r of lane group g
__device__ __forceinline__ int narrow_acc_row(int r, int g) { return narrow_pi(4 * g + r); }

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(NARROW_THREADS, 2) k_attn_narrow_fwd(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                       const bf16* __restrict__ V, int64_t ld_v, bf16* __restrict__ O, int64_t ld_o,
                                                                       bf16* __restrict__ Ores, int64_t ld_r, float* __restrict__ lse2, int H, int Sq, int Sk,
                                                                       float scale2) {
  using TL = NarrowTile<HD>;
  constexpr int NKS = TL::NKS, NCT = TL::NCT, BUF = 2 * TL::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int q0 = wg.tile * 128 + wv * 32;
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + (int64_t)head * HD;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + (int64_t)head * HD;
  const NarrowLane<HD> ln(lane);

  bf16x8 qf[2][NKS];
  f32x4 acc[2][NCT];
  float m_run[2], l_run[2];
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int qi = min(q0 + 16 * nt + n, Sq - 1);
    narrow_row_frags<HD>(qf[nt], Q + ((int64_t)b * Sq + qi) * ld_q + (int64_t)head * HD, g);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[nt] = -INFINITY;
    l_run[nt] = 0.f;
  }

  bf16x8 kreg[TL::PER], vreg[TL::PER];
  const int nkt = (Sk + NARROW_ROWS - 1) / NARROW_ROWS;
  TL::load(kreg, Kg, ld_k, 0, Sk, tid);
  TL::load(vreg, Vg, ld_v, 0, Sk, tid);
  TL::store(kreg, smem, tid);
  TL::store(vreg, smem + TL::BYTES, tid);
  __syncthreads();

  auto tile = [&](int kt, auto masked_c) {
    constexpr bool MASKED = decltype(masked_c)::value;      // ragged last tile: scores are rewritten in place, already scaled
    const int buf = kt & 1;
    if (kt + 1 < nkt) {
      TL::load(kreg, Kg, ld_k, (kt + 1) * NARROW_ROWS, Sk, tid);
      TL::load(vreg, Vg, ld_v, (kt + 1) * NARROW_ROWS, Sk, tid);
    }
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TL::BYTES;
    const int key0 = kt * NARROW_ROWS;

    f32x4 s[4][2];                                           // S^T[key 16 t + pi(4 g + r)][query 16 nt + n]
#pragma unroll
    for (int t = 0; t < 4; t++) {
      s[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      s[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++) {
        const bf16x8 a = ln.rows(ks, t, ks_);
        s[t][0] = NARROW_MFMA(a, qf[0][ks_], s[t][0]);
        s[t][1] = NARROW_MFMA(a, qf[1][ks_], s[t][1]);
      }
    }
    const float psc = MASKED ? 1.f : scale2;                 // plain tiles keep the RAW score: the scale rides in the exponent's fma
    float m_new[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
      float mt = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (MASKED) {
            float x = s[t][nt][r] * scale2;
            if (key0 + 16 * t + narrow_acc_row(r, g) >= Sk) x = -INFINITY;
            s[t][nt][r] = x;
          }
          mt = fmaxf(mt, s[t][nt][r]);
        }
      if (!MASKED) mt *= scale2;                             // scale2 > 0
      mt = quad_max(mt);
      m_new[nt] = fmaxf(m_run[nt], mt);
      const float alpha = fast_exp2(m_run[nt] - m_new[nt]);
      m_run[nt] = m_new[nt];
      l_run[nt] *= alpha;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc[nt][ct][r] *= alpha;
      }
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
      bf16x8 pf[2];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        float e[8];
        float ls0 = 0.f, ls1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          e[j] = fast_exp2(fmaf(s[2 * p + (j >> 2)][nt][j & 3], psc, -m_new[nt]));
          if (j & 1) ls1 += e[j]; else ls0 += e[j];
        }
        l_run[nt] += ls0 + ls1;
        pf[nt] = pack8(e);
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {                     // V^T[channel 16 ct + n][keys of the tile pair p, in the order of pf]
        const bf16x8 a = ln.cols(vs, p, ct);
        acc[0][ct] = NARROW_MFMA(a, pf[0], acc[0][ct]);
        acc[1][ct] = NARROW_MFMA(a, pf[1], acc[1][ct]);
      }
    }
    if (kt + 1 < nkt) {
      TL::store(kreg, smem + (buf ^ 1) * BUF, tid);
      TL::store(vreg, smem + (buf ^ 1) * BUF + TL::BYTES, tid);
    }
    __syncthreads();
  };
  const int nfull = Sk / NARROW_ROWS;
  for (int kt = 0; kt < nfull; kt++) tile(kt, std::false_type{});
  for (int kt = nfull; kt < nkt; kt++) tile(kt, std::true_type{});

#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const float l_tot = quad_sum(l_run[nt]);
    const int q = q0 + 16 * nt + n;
    if (q < Sq) {
      const int64_t row = (int64_t)b * Sq + q;
      narrow_store_row<HD>(O + row * ld_o + (int64_t)head * HD, Ores ? Ores + row * ld_r + (int64_t)head * HD : nullptr, acc[nt], 1.f / l_tot, g);
      if (g == 0) lse2[bh * Sq + q] = m_run[nt] + __log2f(l_tot);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward: delta and dQ
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(NARROW_THREADS, 2) k_attn_narrow_dq(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                      const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ O, int64_t ld_o,
                                                                      const bf16* __restrict__ Ores, int64_t ld_r, const bf16* __restrict__ dO, int64_t ld_do,
                                                                      const float* __restrict__ lse2, bf16* __restrict__ dQ, int64_t ld_dq,
                                                                      float* __restrict__ delta_out, int H, int Sq, int Sk, float scale, float scale2) {
  using TL = NarrowTile<HD>;
  constexpr int NKS = TL::NKS, NCT = TL::NCT, BUF = 2 * TL::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int q0 = wg.tile * 128 + wv * 32;
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + (int64_t)head * HD;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + (int64_t)head * HD;
  const NarrowLane<HD> ln(lane);

  bf16x8 kreg[TL::PER], vreg[TL::PER];
  const int nkt = (Sk + NARROW_ROWS - 1) / NARROW_ROWS;
  TL::load(kreg, Kg, ld_k, 0, Sk, tid);
  TL::load(vreg, Vg, ld_v, 0, Sk, tid);

  bf16x8 qf[2][NKS], gf[2][NKS];
  f32x4 acc[2][NCT];
  float L[2], delta[2];
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int q = q0 + 16 * nt + n, qi = min(q, Sq - 1);
    const int64_t row = (int64_t)b * Sq + qi;
    narrow_row_frags<HD>(qf[nt], Q + row * ld_q + (int64_t)head * HD, g);
    narrow_row_frags<HD>(gf[nt], dO + row * ld_do + (int64_t)head * HD, g);
    L[nt] = lse2[bh * Sq + qi];
    // delta = sum_c dO (O + o_res): this lane's channels (zeros past the head), then the four lanes of the query
    bf16x8 of[NKS];
    narrow_row_frags<HD>(of, O + row * ld_o + (int64_t)head * HD, g);
    float dsum = 0.f;
    if (Ores) {
      bf16x8 rf[NKS];
      narrow_row_frags<HD>(rf, Ores + row * ld_r + (int64_t)head * HD, g);
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++)
#pragma unroll
        for (int j = 0; j < 8; j++) dsum = fmaf(bf2f(gf[nt][ks_][j]), bf2f(of[ks_][j]) + bf2f(rf[ks_][j]), dsum);
    } else {
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++)
#pragma unroll
        for (int j = 0; j < 8; j++) dsum = fmaf(bf2f(gf[nt][ks_][j]), bf2f(of[ks_][j]), dsum);
    }
    delta[nt] = quad_sum(dsum);
    if (g == 0 && q < Sq) delta_out[bh * Sq + q] = delta[nt];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  TL::store(kreg, smem, tid);
  TL::store(vreg, smem + TL::BYTES, tid);
  __syncthreads();

  for (int kt = 0; kt < nkt; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nkt) {
      TL::load(kreg, Kg, ld_k, (kt + 1) * NARROW_ROWS, Sk, tid);
      TL::load(vreg, Vg, ld_v, (kt + 1) * NARROW_ROWS, Sk, tid);
    }
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TL::BYTES;
    const int key0 = kt * NARROW_ROWS;
#pragma unroll
    for (int p = 0; p < 2; p++) {
      f32x4 s[2][2], dp[2][2];                               // [tile 2 p + tt][nt]: S^T = K Q^T, dP^T = V dO^T: lane = query column, registers = keys
#pragma unroll
      for (int tt = 0; tt < 2; tt++) {
        s[tt][0] = s[tt][1] = dp[tt][0] = dp[tt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks_ = 0; ks_ < NKS; ks_++) {
          const bf16x8 ak = ln.rows(ks, 2 * p + tt, ks_), av = ln.rows(vs, 2 * p + tt, ks_);
          s[tt][0] = NARROW_MFMA(ak, qf[0][ks_], s[tt][0]);
          s[tt][1] = NARROW_MFMA(ak, qf[1][ks_], s[tt][1]);
          dp[tt][0] = NARROW_MFMA(av, gf[0][ks_], dp[tt][0]);
          dp[tt][1] = NARROW_MFMA(av, gf[1][ks_], dp[tt][1]);
        }
      }
      bf16x8 dsf[2];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        float ds[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int tt = j >> 2, r = j & 3;
          float pr = fast_exp2(fmaf(s[tt][nt][r], scale2, -L[nt]));
          if (key0 + 32 * p + 16 * tt + narrow_acc_row(r, g) >= Sk) pr = 0.f;
          ds[j] = pr * (dp[tt][nt][r] - delta[nt]);
        }
        dsf[nt] = pack8(ds);
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {                     // dQ^T[channel][query] += K^T[channel][keys of the pair] dS^T[keys][query]
        const bf16x8 a = ln.cols(ks, p, ct);
        acc[0][ct] = NARROW_MFMA(a, dsf[0], acc[0][ct]);
        acc[1][ct] = NARROW_MFMA(a, dsf[1], acc[1][ct]);
      }
    }
    if (kt + 1 < nkt) {
      TL::store(kreg, smem + (buf ^ 1) * BUF, tid);
      TL::store(vreg, smem + (buf ^ 1) * BUF + TL::BYTES, tid);
    }
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int q = q0 + 16 * nt + n;
    if (q < Sq) narrow_store_row<HD>(dQ + ((int64_t)b * Sq + q) * ld_dq + (int64_t)head * HD, nullptr, acc[nt], scale, g);
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dK and dV
// ------------------------------------------------------------------------------------------------
template <int HD>
__global__ void __launch_bounds__(NARROW_THREADS, 2) k_attn_narrow_dkv(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                       const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ dO, int64_t ld_do,
                                                                       const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                       bf16* __restrict__ dK, int64_t ld_dk, bf16* __restrict__ dV, int64_t ld_dv, int H, int Sq,
                                                                       int Sk, float scale, float scale2) {
  using TL = NarrowTile<HD>;
  constexpr int NKS = TL::NKS, NCT = TL::NCT, AUX = 2 * NARROW_ROWS * 4, BUF = 2 * TL::BYTES + AUX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int key0 = wg.tile * 128 + wv * 32;
  const bool active = key0 < Sk;                   // wave-uniform: a wave whose 32 keys all lie past Sk only helps staging
  const bf16* Qg = Q + (int64_t)b * Sq * ld_q + (int64_t)head * HD;
  const bf16* Gg = dO + (int64_t)b * Sq * ld_do + (int64_t)head * HD;
  const NarrowLane<HD> ln(lane);

  bf16x8 kf[2][NKS], vf[2][NKS];
  f32x4 acc_k[2][NCT], acc_v[2][NCT];
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int kj = min(key0 + 16 * nt + n, Sk - 1);
    narrow_row_frags<HD>(kf[nt], K + ((int64_t)b * Sk + kj) * ld_k + (int64_t)head * HD, g);
    narrow_row_frags<HD>(vf[nt], V + ((int64_t)b * Sk + kj) * ld_v + (int64_t)head * HD, g);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc_k[nt][ct] = acc_v[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  bf16x8 qreg[TL::PER], greg[TL::PER];
  float areg = 0.f;
  const int nqt = (Sq + NARROW_ROWS - 1) / NARROW_ROWS;
  // per query of the tile, in the accumulator order (slot 16 t + m holds query 16 t + pi(m)): threads 0..63 carry lse2 (+inf past Sq: P = exp2(-inf) = 0
  // exactly), threads 64..127 carry delta (0 past Sq)
  const int aux_q = (tid & 48) + narrow_pi(tid & 15);
  auto load_tile = [&](int qt) {
    TL::load(qreg, Qg, ld_q, qt * NARROW_ROWS, Sq, tid);
    TL::load(greg, Gg, ld_do, qt * NARROW_ROWS, Sq, tid);
    if (tid < 2 * NARROW_ROWS) {
      const int qq = qt * NARROW_ROWS + aux_q;
      const float* src = tid < NARROW_ROWS ? lse2 : delta;
      const float pad = tid < NARROW_ROWS ? INFINITY : 0.f;
      areg = qq < Sq ? src[bh * Sq + qq] : pad;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * BUF;
    TL::store(qreg, base, tid);
    TL::store(greg, base + TL::BYTES, tid);
    if (tid < 2 * NARROW_ROWS) ((float*)(base + 2 * TL::BYTES))[tid] = areg;
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
#pragma unroll
      for (int p = 0; p < 2; p++) {
        f32x4 s[2][2], dp[2][2];                             // [tile 2 p + tt][nt]: S = Q K^T, dP = dO V^T: lane = key column, registers = queries
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
          s[tt][0] = s[tt][1] = dp[tt][0] = dp[tt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks_ = 0; ks_ < NKS; ks_++) {
            const bf16x8 aq = ln.rows(qs, 2 * p + tt, ks_), ag = ln.rows(gs, 2 * p + tt, ks_);
            s[tt][0] = NARROW_MFMA(aq, kf[0][ks_], s[tt][0]);
            s[tt][1] = NARROW_MFMA(aq, kf[1][ks_], s[tt][1]);
            dp[tt][0] = NARROW_MFMA(ag, vf[0][ks_], dp[tt][0]);
            dp[tt][1] = NARROW_MFMA(ag, vf[1][ks_], dp[tt][1]);
          }
        }
        f32x4 l4[2], d4[2];                                  // lse2 / delta of the queries of registers 0..3 of the two tiles
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
          l4[tt] = *(const f32x4*)(aux + 32 * p + 16 * tt + 4 * g);
          d4[tt] = *(const f32x4*)(aux + NARROW_ROWS + 32 * p + 16 * tt + 4 * g);
        }
        bf16x8 pf[2], dsf[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
          float pr[8], ds[8];
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const int tt = j >> 2, r = j & 3;
            pr[j] = fast_exp2(fmaf(s[tt][nt][r], scale2, -l4[tt][r]));
            ds[j] = pr[j] * (dp[tt][nt][r] - d4[tt][r]);
          }
          pf[nt] = pack8(pr);
          dsf[nt] = pack8(ds);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {      // dV^T[channel][key] += dO^T[channel][queries] P[queries][key];  dK^T[channel][key] += Q^T[channel][queries] dS[queries][key]
          const bf16x8 ag = ln.cols(gs, p, ct), aq = ln.cols(qs, p, ct);
          acc_v[0][ct] = NARROW_MFMA(ag, pf[0], acc_v[0][ct]);
          acc_v[1][ct] = NARROW_MFMA(ag, pf[1], acc_v[1][ct]);
          acc_k[0][ct] = NARROW_MFMA(aq, dsf[0], acc_k[0][ct]);
          acc_k[1][ct] = NARROW_MFMA(aq, dsf[1], acc_k[1][ct]);
        }
      }
    }
    if (qt + 1 < nqt) store_tile(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int key = key0 + 16 * nt + n;
    if (key < Sk) {
      narrow_store_row<HD>(dK + ((int64_t)b * Sk + key) * ld_dk + (int64_t)head * HD, nullptr, acc_k[nt], scale, g);
      narrow_store_row<HD>(dV + ((int64_t)b * Sk + key) * ld_dv + (int64_t)head * HD, nullptr, acc_v[nt], 1.f, g);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool narrow_block_ok(const void* p, int64_t ld, int H, int d) { return p && ((uintptr_t)p & 15) == 0 && ld % 8 == 0 && ld >= (int64_t)H * d; }

template <int HD>
static void narrow_launch_fwd(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, void* o, int64_t ld_o,
                              void* o_res, int64_t ld_r, float* lse2, int B, int H, int Sq, int Sk, float scale) {
  constexpr int lds = 2 * 2 * NarrowTile<HD>::BYTES;
  hipLaunchKernelGGL(k_attn_narrow_fwd<HD>, dim3((Sq + 127) / 128, H, B), dim3(NARROW_THREADS), lds, st, (const bf16*)q, ld_q, (const bf16*)k, ld_k,
                     (const bf16*)v, ld_v, (bf16*)o, ld_o, (bf16*)o_res, ld_r, lse2, H, Sq, Sk, scale * LOG2E);
}

template <int HD>
static void narrow_launch_dq(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o, int64_t ld_o,
                             const void* o_res, int64_t ld_r, const void* dO, int64_t ld_do, const float* lse2, void* dq, int64_t ld_dq, float* delta, int B, int H,
                             int Sq, int Sk, float scale) {
  constexpr int lds = 2 * 2 * NarrowTile<HD>::BYTES;
  hipLaunchKernelGGL(k_attn_narrow_dq<HD>, dim3((Sq + 127) / 128, H, B), dim3(NARROW_THREADS), lds, st, (const bf16*)q, ld_q, (const bf16*)k, ld_k,
                     (const bf16*)v, ld_v, (const bf16*)o, ld_o, (const bf16*)o_res, ld_r, (const bf16*)dO, ld_do, lse2, (bf16*)dq, ld_dq, delta, H, Sq, Sk, scale,
                     scale * LOG2E);
}

template <int HD>
static void narrow_launch_dkv(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* dO,
                              int64_t ld_do, const float* lse2, const float* delta, void* dk, int64_t ld_dk, void* dv, int64_t ld_dv, int B, int H, int Sq, int Sk,
                              float scale) {
  constexpr int lds = 2 * (2 * NarrowTile<HD>::BYTES + 2 * NARROW_ROWS * 4);
  hipLaunchKernelGGL(k_attn_narrow_dkv<HD>, dim3((Sk + 127) / 128, H, B), dim3(NARROW_THREADS), lds, st, (const bf16*)q, ld_q, (const bf16*)k, ld_k,
                     (const bf16*)v, ld_v, (const bf16*)dO, ld_do, lse2, delta, (bf16*)dk, ld_dk, (bf16*)dv, ld_dv, H, Sq, Sk, scale, scale * LOG2E);
}

extern "C" int st355_attn_narrow_fwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, void* o, int64_t ld_o,
                                     void* o_res, int64_t ld_ores, float* lse2, int B, int H, int Sq, int Sk, int d, float scale) {
  if (d != 40 && d != 80) { st355_set_error("attn_narrow_fwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_narrow_fwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(lse2 && narrow_block_ok(q, ld_q, H, d) && narrow_block_ok(k, ld_k, H, d) && narrow_block_ok(v, ld_v, H, d) && narrow_block_ok(o, ld_o, H, d) &&
                 (!o_res || narrow_block_ok(o_res, ld_ores, H, d)),
             "attn_narrow_fwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * d");
  ProfScope ps(stream, ST355_K_ATTN_FWD, 4.0 * (double)B * H * (double)Sq * Sk * d, 2.0 * (double)B * H * ((o_res ? 3.0 : 2.0) * Sq + 2.0 * Sk) * d);
  if (d == 40) narrow_launch_fwd<40>((hipStream_t)stream, q, ld_q, k, ld_k, v, ld_v, o, ld_o, o_res, ld_ores, lse2, B, H, Sq, Sk, scale);
  else narrow_launch_fwd<80>((hipStream_t)stream, q, ld_q, k, ld_k, v, ld_v, o, ld_o, o_res, ld_ores, lse2, B, H, Sq, Sk, scale);
  return st355_check_launch("attn_narrow_fwd");
}

extern "C" size_t st355_attn_narrow_bwd_workspace(int B, int H, int Sq, int d) {      // delta [B, H, Sq] fp32
  (void)d;
  return B > 0 && H > 0 && Sq > 0 ? (size_t)B * H * Sq * sizeof(float) : 0;
}

extern "C" int st355_attn_narrow_bwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o,
                                     int64_t ld_o, const void* o_res, int64_t ld_ores, const void* dO, int64_t ld_do, const float* lse2, void* dq, int64_t ld_dq,
                                     void* dk, int64_t ld_dk, void* dv, int64_t ld_dv, void* workspace, int B, int H, int Sq, int Sk, int d, float scale) {
  if (d != 40 && d != 80) { st355_set_error("attn_narrow_bwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_narrow_bwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(lse2 && workspace && ((uintptr_t)workspace & 3) == 0, "attn_narrow_bwd: null lse2 / workspace");
  ST_REQUIRE(narrow_block_ok(q, ld_q, H, d) && narrow_block_ok(k, ld_k, H, d) && narrow_block_ok(v, ld_v, H, d) && narrow_block_ok(o, ld_o, H, d) &&
                 (!o_res || narrow_block_ok(o_res, ld_ores, H, d)) && narrow_block_ok(dO, ld_do, H, d) && narrow_block_ok(dq, ld_dq, H, d) &&
                 narrow_block_ok(dk, ld_dk, H, d) && narrow_block_ok(dv, ld_dv, H, d),
             "attn_narrow_bwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * d");
  float* delta = (float*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  const double fl_unit = 2.0 * (double)B * H * (double)Sq * Sk * d;
  {
    ProfScope ps(stream, ST355_K_ATTN_BWD_DQ, 3.0 * fl_unit, 2.0 * (double)B * H * ((o_res ? 5.0 : 4.0) * Sq + 2.0 * Sk) * d);
    if (d == 40) narrow_launch_dq<40>(st, q, ld_q, k, ld_k, v, ld_v, o, ld_o, o_res, ld_ores, dO, ld_do, lse2, dq, ld_dq, delta, B, H, Sq, Sk, scale);
    else narrow_launch_dq<80>(st, q, ld_q, k, ld_k, v, ld_v, o, ld_o, o_res, ld_ores, dO, ld_do, lse2, dq, ld_dq, delta, B, H, Sq, Sk, scale);
    const int rc = st355_check_launch("attn_narrow_dq");
    if (rc) return rc;
  }
  ProfScope ps(stream, ST355_K_ATTN_BWD_DKV, 4.0 * fl_unit, 2.0 * (double)B * H * (2.0 * Sq + 4.0 * Sk) * d);
  if (d == 40) narrow_launch_dkv<40>(st, q, ld_q, k, ld_k, v, ld_v, dO, ld_do, lse2, delta, dk, ld_dk, dv, ld_dv, B, H, Sq, Sk, scale);
  else narrow_launch_dkv<80>(st, q, ld_q, k, ld_k, v, ld_v, dO, ld_do, lse2, delta, dk, ld_dk, dv, ld_dv, B, H, Sq, Sk, scale);
  return st355_check_launch("attn_narrow_dkv");
}

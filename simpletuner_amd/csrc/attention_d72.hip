// attention_d72.hip — fused attention for heads of 72 channels (PixArt-Sigma: 16 heads over 1152 channels), forward and backward, self and cross, on TOKEN-MAJOR
// operands with a HEAD PITCH and an additive KEY BIAS.  Every q / k / v / o / dO / dq / dk / dv pointer is the first column of a column block of a [B*S, ld]
// buffer; row b*S + i holds head h at columns h*pitch .. h*pitch + 71 (pitch >= 72, pitch % 8 == 0: 96 on PixArt's head-padded projections, 72 on an unpadded
// layout).  Columns 72 .. pitch-1 of a head are never read; the kernels write ZEROS there in o / dq / dk / dv, so every element of every head's pitch-wide block of
// the outputs is written.  No head-split, transposed or head-major copy on either side.
//   x_ij = scale q_i.k_j + bias_j     O = softmax(x) V     lse2_i = log2 sum_j exp(x_ij)                       (log2 convention of attn_common.h, bias included)
//   dV = P^T dO,  dS = P o (dP - delta),  dP = dO V^T,  delta_i = sum_c dO_ic O_ic (fp32, from the bf16 O),  dQ = scale dS K,  dK = scale dS^T Q
//
// gfx950 design (v_mfma_f32_16x16x32_bf16, fp32 accumulation).  Fragment maps (lane l, g = l >> 4, n = l & 15):  A[i = n][k = 8 g + 0..7],  B[k = 8 g + 0..7][n],
// C[i = 4 g + r][n] in register r.
//   * channel tiling: output channels are 5 tiles of 16 (80 rows: 72 are stored, the lanes that own channels 72..79 store zeros when pitch leaves room for them,
//     columns 80 .. pitch-1 are zero-filled by 16-byte vector stores of the same lanes).  The score contraction is 32 + 32 + an 8-channel tail: in the tail step
//     lane groups 1..3 hold ZEROS MADE IN REGISTERS on both operands — the columns right of channel 71 are pad lanes or the next head and are never loaded.
//   * tile image: 64 token rows x 72 channels = 9 chunks of 16 bytes per row, copied straight from the token-major rows (576 chunks over 256 threads).  Row pitch
//     = 9 chunks = 144 bytes, no pad chunk.  Bank model (64 banks x 4 bytes; a 16-byte chunk is one of 16 four-bank slots), derived for pitch 9:
//       - row fragments (ds_read_b128; lane (n, g) reads chunk 4 ks + g of row pi(n)): the 16 lanes of a group read one chunk column of 16 rows; slot =
//         (9 row + chunk) mod 16, and 9 is odd, so row -> slot is a bijection of the 16 rows: conflict-free, no swizzle.  (The tail step reads chunk 8 of every
//         row in all four groups: the same addresses, a broadcast.)
//       - transposed fragments (ds_read_b64_tr_b16 pairs; a half wave reads 8 rows x 32 bytes = two slots per row, starting at slot 9 row + 2 ct mod 16): in the
//         row order pi(m) = 2 (m & 7) + (m >> 3) a half wave owns the even (or the odd) rows of a 16-row tile; 9 * 2 m' mod 16 = 2 m' mod 16, eight distinct even
//         slots, each row covering its slot and the next odd one: disjoint, conflict-free.  Consecutive rows would collide (rows 0 and 7: slots 0,1 and 15,0).
//   * fragment chaining: scores are computed transposed (S^T = K Q^T; a lane owns a query column, its 4 registers of key tile t hold keys 16 t + pi(4 g + r)), so
//     the exp2 registers of tiles 2 p, 2 p + 1 are the B operand of O^T += V^T P^T as they are, and the transposed V reads deliver the same key order.  P and dS
//     never leave the register file.
//   * key bias and ragged keys share one mechanism: with every staged 64-key tile go 64 floats b2 = bias log2e (0 without a bias), -inf for keys past Sk, in
//     accumulator order, so a lane reads its four keys' values as one ds_read_b128.  x = fma(s, scale2, b2): a masked key gives P = exp2(-inf) = 0 exactly.
//     Forward tiles that are full and unbiased keep the raw score and carry the scale in the exponent's fma.  dK/dV (lane = key) holds its keys' b2 in registers.
//   * work split, chosen for PixArt (4096 / 16384 queries and keys in self-attention, 300 keys in cross-attention).  Forward and dQ: a wave owns NT 16-query
//     column tiles, a workgroup 4 waves = 64 NT queries; every K / V fragment read from LDS feeds NT MFMAs.  NT = 2 (32 queries per wave, two waves per SIMD) is
//     what is launched.  NT = 4 (64 queries per wave) halves the LDS fragment traffic per MFMA and compiles without scratch, but needs 380 / 407 registers
//     (forward / dQ): one wave per SIMD, and measured SLOWER at S 4096 and 16384 (forward 316 / 2364 us against 256 / 1841 us, backward 725 / 5576 against
//     663 / 4951): with one wave nothing covers the softmax VALU section between the two MFMA runs of a tile.  The template stays general in NT; only NT = 2 is
//     instantiated.  dK/dV: a wave owns NT 16-key tiles; NT = 2 (128 keys per workgroup) from D72_LONG keys, NT = 1 (64 keys) below, so that 300 keys are five
//     workgroups with 19 of 20 waves live instead of three with 10 of 12 (the query loop is the whole of Sq either way).  Staged tiles are double-buffered: the
//     next tile's global loads are issued before the MFMA work and written to the other LDS buffer after it.  Grid (tiles, H, B) through attn_wg_map().
//   * LDS: forward / dQ 2 x (K + V + 256 bytes of b2) = 37 376 bytes; dK/dV 2 x (Q + dO + 512 bytes of lse2 / delta) = 37 888 bytes.  Registers, scratch (0) and
//     occupancy as compiled: profiles/attn_d72_kernel_stats.md.
//   No atomics and no scratch: every output element has one owner and a fixed summation order, so launches are bit-identical.  Any Sq, Sk >= 1: loads clamp the
//   row, masked scores give P = 0 exactly, stores are guarded.
#include <type_traits>
#include "attn_common.h"

#define D72_THREADS 256
#define D72_ROWS 64         // token rows per staged tile
#define D72_HD 72
#define D72_LONG 512        // dK/dV: key count from which a wave owns 32 keys instead of 16

#define D72_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

namespace {

constexpr int NCH = D72_HD / 8;                  // 16-byte chunks per row
constexpr int ROWB = NCH * 16;                   // row pitch, bytes: 9 chunks, odd
constexpr int TILE_BYTES = D72_ROWS * ROWB;
constexpr int TOTAL = D72_ROWS * NCH;            // chunks per tile
constexpr int PER = (TOTAL + D72_THREADS - 1) / D72_THREADS;
constexpr int NKS = 3;                           // contraction steps: 32 + 32 + 8
constexpr int NCT = 5;                           // 16-channel output tiles

// row order of a 16-row tile as MFMA A rows / transposed-read rows: even rows first
__device__ __forceinline__ int d72_pi(int m) { return 2 * (m & 7) + (m >> 3); }

// all-reduce over the four lanes n, n + 16, n + 32, n + 48 that share a column (VALU lane swaps, no LDS round trip)
__device__ __forceinline__ float d72_quad_max(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_max(fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1])));
}
__device__ __forceinline__ float d72_quad_sum(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_sum(__uint_as_float(r[0]) + __uint_as_float(r[1]));
}

// rows row0 .. row0 + 63 of one head (base = block start + batch offset + head * pitch); rows past nrows - 1 re-read the last valid row; channels 0..71 only
__device__ __forceinline__ void tile_load(bf16x8 (&reg)[PER], const bf16* base, int64_t ld, int row0, int nrows, int tid) {
#pragma unroll
  for (int p = 0; p < PER; p++) {
    const int id = p * D72_THREADS + tid;
    if ((p + 1) * D72_THREADS <= TOTAL || id < TOTAL) {
      const int row = id / NCH, c = id - row * NCH;
      reg[p] = *(const bf16x8*)(base + (int64_t)min(row0 + row, nrows - 1) * ld + c * 8);
    }
  }
}
__device__ __forceinline__ void tile_store(const bf16x8 (&reg)[PER], char* lds, int tid) {
#pragma unroll
  for (int p = 0; p < PER; p++) {
    const int id = p * D72_THREADS + tid;
    if ((p + 1) * D72_THREADS <= TOTAL || id < TOTAL) {
      const int row = id / NCH, c = id - row * NCH;
      *(bf16x8*)(lds + row * ROWB + c * 16) = reg[p];
    }
  }
}

// per-lane LDS offsets of the two fragment kinds
struct Lane {
  int row_off;         // row fragments: row pi(n), chunk g of contraction step 0
  int tail_off;        // ... chunk 8 of the same row: the tail step
  bool tail_live;      // lane group 0 holds channels 64..71 in the tail step, groups 1..3 hold zeros
  int tr_off;          // transposed fragments: row pi(4 g + i'), channels 4 s .. 4 s + 3 (lane = 16 g + 4 i' + s)
  int tr_last;         // ... of channel tile 4 (channels clamped to 68..71: the lanes that receive channels >= 72 store zeros)
  __device__ __forceinline__ Lane(int lane) {
    const int g = lane >> 4, n = lane & 15, ip = (lane >> 2) & 3, s = lane & 3;
    row_off = d72_pi(n) * ROWB + g * 16;
    tail_off = d72_pi(n) * ROWB + (NCH - 1) * 16;
    tail_live = g == 0;
    tr_off = d72_pi(4 * g + ip) * ROWB + s * 8;
    tr_last = d72_pi(4 * g + ip) * ROWB + min(64 + 4 * s, D72_HD - 4) * 2;
  }
  // MFMA A fragment, rows = token rows of the 16-row tile t: A[i = n -> row 16 t + pi(n)][k = channels 32 ks + 8 g + 0..7], zeros past channel 71
  __device__ __forceinline__ bf16x8 rows(const char* lds, int t, int ks) const {
    const char* p = lds + t * 16 * ROWB;
    if (ks < NKS - 1) return *(const bf16x8*)(p + row_off + ks * 64);
    const bf16x8 x = *(const bf16x8*)(p + tail_off);
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return tail_live ? x : z;
  }
  // MFMA A fragment, rows = channels of tile ct: A[i = n -> channel 16 ct + n][k = 8 g + j -> token row 32 p + 16 (j >> 2) + pi(4 g + (j & 3))]
  __device__ __forceinline__ bf16x8 cols(const char* lds, int p, int ct) const {
    const char* q = lds + p * 32 * ROWB + (ct < NCT - 1 ? tr_off + ct * 32 : tr_last);
    return lds_tr16x2(q, q + 16 * ROWB);
  }
};

// one token row of a head as MFMA B fragments: B[k = channels 32 ks + 8 g + 0..7][n]; the tail step loads channels 64..71 in lane group 0 only
__device__ __forceinline__ void row_frags(bf16x8 (&f)[NKS], const bf16* row, int g) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  f[0] = *(const bf16x8*)(row + 8 * g);
  f[1] = *(const bf16x8*)(row + 32 + 8 * g);
  f[2] = z;
  if (g == 0) f[2] = *(const bf16x8*)(row + 64);
}

// accumulators acc[ct][r] = X^T[channel 16 ct + 4 g + r][token n] -> one head of a token-major row: channels 0..71 scaled, zeros on 72 .. pitch-1
__device__ __forceinline__ void store_row(bf16* row, const f32x4 (&acc)[NCT], float mul, int g, int pitch) {
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    const int c = 16 * ct + 4 * g;
    if (ct < NCT - 1 || c < pitch) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; r++) o[r] = (ct < NCT - 1 || c < D72_HD) ? f2bf(acc[ct][r] * mul) : f2bf(0.f);
      *(bf16x4*)(row + c) = o;
    }
  }
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 16 * NCT + 8 * g; c < pitch; c += 32) *(bf16x8*)(row + c) = z;
}

// b2 of a staged key tile in accumulator order: slot 16 t + m holds key 16 t + pi(m)
__device__ __forceinline__ int aux_slot_row(int tid) { return (tid & 48) + d72_pi(tid & 15); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(D72_THREADS, NT > 2 ? 1 : 2) k_attn_d72_fwd(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                              const bf16* __restrict__ V, int64_t ld_v, const float* __restrict__ key_bias,
                                                                              bf16* __restrict__ O, int64_t ld_o, float* __restrict__ lse2, int H, int Sq, int Sk,
                                                                              int pitch, float scale2) {
  constexpr int AUX = D72_ROWS * 4, BUF = 2 * TILE_BYTES + AUX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head, hoff = (int64_t)head * pitch;
  const int q0 = wg.tile * (64 * NT) + wv * (16 * NT);
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + hoff;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + hoff;
  const float* bias = key_bias ? key_bias + (int64_t)b * Sk : nullptr;
  const Lane ln(lane);

  bf16x8 qf[NT][NKS];
  f32x4 acc[NT][NCT];
  float m_run[NT], l_run[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int qi = min(q0 + 16 * nt + n, Sq - 1);
    row_frags(qf[nt], Q + ((int64_t)b * Sq + qi) * ld_q + hoff, g);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[nt] = -INFINITY;
    l_run[nt] = 0.f;
  }

  bf16x8 kreg[PER], vreg[PER];
  float areg = 0.f;
  const int nkt = (Sk + D72_ROWS - 1) / D72_ROWS;
  const int aux_k = aux_slot_row(tid);
  auto load_tile = [&](int kt) {
    tile_load(kreg, Kg, ld_k, kt * D72_ROWS, Sk, tid);
    tile_load(vreg, Vg, ld_v, kt * D72_ROWS, Sk, tid);
    if (tid < D72_ROWS) {
      const int key = kt * D72_ROWS + aux_k;
      areg = key < Sk ? (bias ? bias[key] * LOG2E : 0.f) : -INFINITY;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * BUF;
    tile_store(kreg, base, tid);
    tile_store(vreg, base + TILE_BYTES, tid);
    if (tid < D72_ROWS) ((float*)(base + 2 * TILE_BYTES))[tid] = areg;
  };
  load_tile(0);
  store_tile(0);
  __syncthreads();

  auto tile = [&](int kt, auto rewrite_c) {
    constexpr bool REWRITE = decltype(rewrite_c)::value;     // biased or ragged tile: scores are rewritten in place as x = s scale2 + b2
    const int buf = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TILE_BYTES;
    const float* aux = (const float*)(ks + 2 * TILE_BYTES);

    f32x4 s[4][NT];                                          // S^T[key 16 t + pi(4 g + r)][query 16 nt + n]
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int nt = 0; nt < NT; nt++) s[t][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks_ = 0; ks_ < NKS; ks_++) {
        const bf16x8 a = ln.rows(ks, t, ks_);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) s[t][nt] = D72_MFMA(a, qf[nt][ks_], s[t][nt]);
      }
    }
    f32x4 b4[4];
    if (REWRITE) {
#pragma unroll
      for (int t = 0; t < 4; t++) b4[t] = *(const f32x4*)(aux + 16 * t + 4 * g);
    }
    const float psc = REWRITE ? 1.f : scale2;                // plain tiles keep the RAW score: the scale rides in the exponent's fma
    float m_new[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      float mt = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (REWRITE) s[t][nt][r] = fmaf(s[t][nt][r], scale2, b4[t][r]);
          mt = fmaxf(mt, s[t][nt][r]);
        }
      if (!REWRITE) mt *= scale2;                            // scale2 > 0
      mt = d72_quad_max(mt);
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
      bf16x8 pf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
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
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[nt][ct] = D72_MFMA(a, pf[nt], acc[nt][ct]);
      }
    }
    if (kt + 1 < nkt) store_tile(buf ^ 1);
    __syncthreads();
  };
  const int nplain = bias ? 0 : Sk / D72_ROWS;
  for (int kt = 0; kt < nplain; kt++) tile(kt, std::false_type{});
  for (int kt = nplain; kt < nkt; kt++) tile(kt, std::true_type{});

#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const float l_tot = d72_quad_sum(l_run[nt]);
    const int q = q0 + 16 * nt + n;
    if (q < Sq) {
      store_row(O + ((int64_t)b * Sq + q) * ld_o + hoff, acc[nt], 1.f / l_tot, g, pitch);
      if (g == 0) lse2[bh * Sq + q] = m_run[nt] + __log2f(l_tot);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward: delta and dQ
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(D72_THREADS, NT > 2 ? 1 : 2) k_attn_d72_dq(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                             const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ O, int64_t ld_o,
                                                                             const bf16* __restrict__ dO, int64_t ld_do, const float* __restrict__ lse2,
                                                                             const float* __restrict__ key_bias, bf16* __restrict__ dQ, int64_t ld_dq,
                                                                             float* __restrict__ delta_out, int H, int Sq, int Sk, int pitch, float scale,
                                                                             float scale2) {
  constexpr int AUX = D72_ROWS * 4, BUF = 2 * TILE_BYTES + AUX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head, hoff = (int64_t)head * pitch;
  const int q0 = wg.tile * (64 * NT) + wv * (16 * NT);
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + hoff;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + hoff;
  const float* bias = key_bias ? key_bias + (int64_t)b * Sk : nullptr;
  const Lane ln(lane);

  bf16x8 kreg[PER], vreg[PER];
  float areg = 0.f;
  const int nkt = (Sk + D72_ROWS - 1) / D72_ROWS;
  const int aux_k = aux_slot_row(tid);
  auto load_tile = [&](int kt) {
    tile_load(kreg, Kg, ld_k, kt * D72_ROWS, Sk, tid);
    tile_load(vreg, Vg, ld_v, kt * D72_ROWS, Sk, tid);
    if (tid < D72_ROWS) {
      const int key = kt * D72_ROWS + aux_k;
      areg = key < Sk ? (bias ? bias[key] * LOG2E : 0.f) : -INFINITY;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * BUF;
    tile_store(kreg, base, tid);
    tile_store(vreg, base + TILE_BYTES, tid);
    if (tid < D72_ROWS) ((float*)(base + 2 * TILE_BYTES))[tid] = areg;
  };
  load_tile(0);

  bf16x8 qf[NT][NKS], gf[NT][NKS];
  f32x4 acc[NT][NCT];
  float L[NT], delta[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int q = q0 + 16 * nt + n, qi = min(q, Sq - 1);
    const int64_t row = (int64_t)b * Sq + qi;
    row_frags(qf[nt], Q + row * ld_q + hoff, g);
    row_frags(gf[nt], dO + row * ld_do + hoff, g);
    L[nt] = lse2[bh * Sq + qi];
    // delta = sum_c dO O over channels 0..71: this lane's channels (zeros past 71), then the four lanes of the query
    bf16x8 of[NKS];
    row_frags(of, O + row * ld_o + hoff, g);
    float dsum = 0.f;
#pragma unroll
    for (int ks_ = 0; ks_ < NKS; ks_++)
#pragma unroll
      for (int j = 0; j < 8; j++) dsum = fmaf(bf2f(gf[nt][ks_][j]), bf2f(of[ks_][j]), dsum);
    delta[nt] = d72_quad_sum(dsum);
    if (g == 0 && q < Sq) delta_out[bh * Sq + q] = delta[nt];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  store_tile(0);
  __syncthreads();

  for (int kt = 0; kt < nkt; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* ks = smem + buf * BUF;
    const char* vs = ks + TILE_BYTES;
    const float* aux = (const float*)(ks + 2 * TILE_BYTES);
#pragma unroll
    for (int p = 0; p < 2; p++) {
      f32x4 s[2][NT], dp[2][NT];                             // [tile 2 p + tt][nt]: S^T = K Q^T, dP^T = V dO^T: lane = query column, registers = keys
      f32x4 b4[2];
#pragma unroll
      for (int tt = 0; tt < 2; tt++) {
        b4[tt] = *(const f32x4*)(aux + 32 * p + 16 * tt + 4 * g);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) s[tt][nt] = dp[tt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks_ = 0; ks_ < NKS; ks_++) {
          const bf16x8 ak = ln.rows(ks, 2 * p + tt, ks_), av = ln.rows(vs, 2 * p + tt, ks_);
#pragma unroll
          for (int nt = 0; nt < NT; nt++) {
            s[tt][nt] = D72_MFMA(ak, qf[nt][ks_], s[tt][nt]);
            dp[tt][nt] = D72_MFMA(av, gf[nt][ks_], dp[tt][nt]);
          }
        }
      }
      bf16x8 dsf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        float ds[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int tt = j >> 2, r = j & 3;
          const float pr = fast_exp2(fmaf(s[tt][nt][r], scale2, b4[tt][r]) - L[nt]);      // b2 = -inf past Sk: P = 0 exactly
          ds[j] = pr * (dp[tt][nt][r] - delta[nt]);
        }
        dsf[nt] = pack8(ds);
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {                     // dQ^T[channel][query] += K^T[channel][keys of the pair] dS^T[keys][query]
        const bf16x8 a = ln.cols(ks, p, ct);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[nt][ct] = D72_MFMA(a, dsf[nt], acc[nt][ct]);
      }
    }
    if (kt + 1 < nkt) store_tile(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int q = q0 + 16 * nt + n;
    if (q < Sq) store_row(dQ + ((int64_t)b * Sq + q) * ld_dq + hoff, acc[nt], scale, g, pitch);
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dK and dV
// ------------------------------------------------------------------------------------------------
template <int NT, bool BIAS>
__global__ void __launch_bounds__(D72_THREADS, 2) k_attn_d72_dkv(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                 const bf16* __restrict__ V, int64_t ld_v, const bf16* __restrict__ dO, int64_t ld_do,
                                                                 const float* __restrict__ lse2, const float* __restrict__ delta,
                                                                 const float* __restrict__ key_bias, bf16* __restrict__ dK, int64_t ld_dk,
                                                                 bf16* __restrict__ dV, int64_t ld_dv, int H, int Sq, int Sk, int pitch, float scale,
                                                                 float scale2) {
  constexpr int AUX = 2 * D72_ROWS * 4, BUF = 2 * TILE_BYTES + AUX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head, hoff = (int64_t)head * pitch;
  const int key0 = wg.tile * (64 * NT) + wv * (16 * NT);
  const bool active = key0 < Sk;                   // wave-uniform: a wave whose keys all lie past Sk only helps staging
  const bf16* Qg = Q + (int64_t)b * Sq * ld_q + hoff;
  const bf16* Gg = dO + (int64_t)b * Sq * ld_do + hoff;
  const Lane ln(lane);

  bf16x8 kf[NT][NKS], vf[NT][NKS];
  f32x4 acc_k[NT][NCT], acc_v[NT][NCT];
  float kb2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int kj = min(key0 + 16 * nt + n, Sk - 1);
    row_frags(kf[nt], K + ((int64_t)b * Sk + kj) * ld_k + hoff, g);
    row_frags(vf[nt], V + ((int64_t)b * Sk + kj) * ld_v + hoff, g);
    kb2[nt] = BIAS ? key_bias[(int64_t)b * Sk + kj] * LOG2E : 0.f;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc_k[nt][ct] = acc_v[nt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  bf16x8 qreg[PER], greg[PER];
  float areg = 0.f;
  const int nqt = (Sq + D72_ROWS - 1) / D72_ROWS;
  // per query of the tile, in accumulator order: threads 0..63 carry lse2 (+inf past Sq: P = exp2(-inf) = 0 exactly), threads 64..127 carry delta (0 past Sq)
  const int aux_q = aux_slot_row(tid);
  auto load_tile = [&](int qt) {
    tile_load(qreg, Qg, ld_q, qt * D72_ROWS, Sq, tid);
    tile_load(greg, Gg, ld_do, qt * D72_ROWS, Sq, tid);
    if (tid < 2 * D72_ROWS) {
      const int qq = qt * D72_ROWS + aux_q;
      const float* src = tid < D72_ROWS ? lse2 : delta;
      const float pad = tid < D72_ROWS ? INFINITY : 0.f;
      areg = qq < Sq ? src[bh * Sq + qq] : pad;
    }
  };
  auto store_tile = [&](int buf) {
    char* base = smem + buf * BUF;
    tile_store(qreg, base, tid);
    tile_store(greg, base + TILE_BYTES, tid);
    if (tid < 2 * D72_ROWS) ((float*)(base + 2 * TILE_BYTES))[tid] = areg;
  };
  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int qt = 0; qt < nqt; qt++) {
    const int buf = qt & 1;
    if (qt + 1 < nqt) load_tile(qt + 1);
    const char* qs = smem + buf * BUF;
    const char* gs = qs + TILE_BYTES;
    const float* aux = (const float*)(qs + 2 * TILE_BYTES);
    if (active) {
#pragma unroll
      for (int p = 0; p < 2; p++) {
        f32x4 s[2][NT], dp[2][NT];                           // [tile 2 p + tt][nt]: S = Q K^T, dP = dO V^T: lane = key column, registers = queries
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
#pragma unroll
          for (int nt = 0; nt < NT; nt++) s[tt][nt] = dp[tt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks_ = 0; ks_ < NKS; ks_++) {
            const bf16x8 aq = ln.rows(qs, 2 * p + tt, ks_), ag = ln.rows(gs, 2 * p + tt, ks_);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
              s[tt][nt] = D72_MFMA(aq, kf[nt][ks_], s[tt][nt]);
              dp[tt][nt] = D72_MFMA(ag, vf[nt][ks_], dp[tt][nt]);
            }
          }
        }
        f32x4 l4[2], d4[2];                                  // lse2 / delta of the queries of registers 0..3 of the two tiles
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
          l4[tt] = *(const f32x4*)(aux + 32 * p + 16 * tt + 4 * g);
          d4[tt] = *(const f32x4*)(aux + D72_ROWS + 32 * p + 16 * tt + 4 * g);
        }
        bf16x8 pf[NT], dsf[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
          float pr[8], ds[8];
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const int tt = j >> 2, r = j & 3;
            pr[j] = BIAS ? fast_exp2(fmaf(s[tt][nt][r], scale2, kb2[nt]) - l4[tt][r]) : fast_exp2(fmaf(s[tt][nt][r], scale2, -l4[tt][r]));
            ds[j] = pr[j] * (dp[tt][nt][r] - d4[tt][r]);
          }
          pf[nt] = pack8(pr);
          dsf[nt] = pack8(ds);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {      // dV^T[channel][key] += dO^T[channel][queries] P[queries][key];  dK^T[channel][key] += Q^T[channel][queries] dS[queries][key]
          const bf16x8 ag = ln.cols(gs, p, ct), aq = ln.cols(qs, p, ct);
#pragma unroll
          for (int nt = 0; nt < NT; nt++) {
            acc_v[nt][ct] = D72_MFMA(ag, pf[nt], acc_v[nt][ct]);
            acc_k[nt][ct] = D72_MFMA(aq, dsf[nt], acc_k[nt][ct]);
          }
        }
      }
    }
    if (qt + 1 < nqt) store_tile(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    const int key = key0 + 16 * nt + n;
    if (key < Sk) {
      store_row(dK + ((int64_t)b * Sk + key) * ld_dk + hoff, acc_k[nt], scale, g, pitch);
      store_row(dV + ((int64_t)b * Sk + key) * ld_dv + hoff, acc_v[nt], 1.f, g, pitch);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool d72_block_ok(const void* p, int64_t ld, int H, int pitch) {
  return p && ((uintptr_t)p & 15) == 0 && ld % 8 == 0 && ld >= (int64_t)H * pitch;
}

#define D72_FWD_LDS (2 * (2 * TILE_BYTES + D72_ROWS * 4))
#define D72_DKV_LDS (2 * (2 * TILE_BYTES + 2 * D72_ROWS * 4))

template <int NT>
static void d72_launch_fwd(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const float* key_bias, void* o,
                           int64_t ld_o, float* lse2, int B, int H, int Sq, int Sk, int pitch, float scale) {
  hipLaunchKernelGGL(k_attn_d72_fwd<NT>, dim3((Sq + 64 * NT - 1) / (64 * NT), H, B), dim3(D72_THREADS), D72_FWD_LDS, st, (const bf16*)q, ld_q, (const bf16*)k,
                     ld_k, (const bf16*)v, ld_v, key_bias, (bf16*)o, ld_o, lse2, H, Sq, Sk, pitch, scale * LOG2E);
}

template <int NT>
static void d72_launch_dq(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o, int64_t ld_o,
                          const void* dO, int64_t ld_do, const float* lse2, const float* key_bias, void* dq, int64_t ld_dq, float* delta, int B, int H, int Sq,
                          int Sk, int pitch, float scale) {
  hipLaunchKernelGGL(k_attn_d72_dq<NT>, dim3((Sq + 64 * NT - 1) / (64 * NT), H, B), dim3(D72_THREADS), D72_FWD_LDS, st, (const bf16*)q, ld_q, (const bf16*)k, ld_k,
                     (const bf16*)v, ld_v, (const bf16*)o, ld_o, (const bf16*)dO, ld_do, lse2, key_bias, (bf16*)dq, ld_dq, delta, H, Sq, Sk, pitch, scale,
                     scale * LOG2E);
}

template <int NT, bool BIAS>
static void d72_launch_dkv(hipStream_t st, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* dO, int64_t ld_do,
                           const float* lse2, const float* delta, const float* key_bias, void* dk, int64_t ld_dk, void* dv, int64_t ld_dv, int B, int H, int Sq,
                           int Sk, int pitch, float scale) {
  hipLaunchKernelGGL((k_attn_d72_dkv<NT, BIAS>), dim3((Sk + 64 * NT - 1) / (64 * NT), H, B), dim3(D72_THREADS), D72_DKV_LDS, st, (const bf16*)q, ld_q,
                     (const bf16*)k, ld_k, (const bf16*)v, ld_v, (const bf16*)dO, ld_do, lse2, delta, key_bias, (bf16*)dk, ld_dk, (bf16*)dv, ld_dv, H, Sq, Sk,
                     pitch, scale, scale * LOG2E);
}

extern "C" int st355_attn_d72_fwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const float* key_bias, void* o,
                                  int64_t ld_o, float* lse2, int B, int H, int Sq, int Sk, int d, int pitch, float scale) {
  if (d != D72_HD) { st355_set_error("attn_d72_fwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_d72_fwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(pitch >= D72_HD && pitch % 8 == 0, "attn_d72_fwd: pitch %d: the head pitch must be >= 72 and a multiple of 8", pitch);
  ST_REQUIRE(lse2 && d72_block_ok(q, ld_q, H, pitch) && d72_block_ok(k, ld_k, H, pitch) && d72_block_ok(v, ld_v, H, pitch) && d72_block_ok(o, ld_o, H, pitch),
             "attn_d72_fwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * pitch");
  ST_REQUIRE(!key_bias || ((uintptr_t)key_bias & 3) == 0, "attn_d72_fwd: misaligned key_bias");
  const hipStream_t st = (hipStream_t)stream;
  ProfScope ps(stream, ST355_K_ATTN_FWD, 4.0 * (double)B * H * (double)Sq * Sk * d, 2.0 * (double)B * H * (2.0 * Sq + 2.0 * Sk) * d);
  d72_launch_fwd<2>(st, q, ld_q, k, ld_k, v, ld_v, key_bias, o, ld_o, lse2, B, H, Sq, Sk, pitch, scale);
  return st355_check_launch("attn_d72_fwd");
}

extern "C" size_t st355_attn_d72_bwd_workspace(int B, int H, int Sq, int d) {      // delta [B, H, Sq] fp32
  (void)d;
  return B > 0 && H > 0 && Sq > 0 ? (size_t)B * H * Sq * sizeof(float) : 0;
}

extern "C" int st355_attn_d72_bwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o, int64_t ld_o,
                                  const void* dO, int64_t ld_do, const float* lse2, const float* key_bias, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk, void* dv,
                                  int64_t ld_dv, void* workspace, int B, int H, int Sq, int Sk, int d, int pitch, float scale) {
  if (d != D72_HD) { st355_set_error("attn_d72_bwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_d72_bwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(pitch >= D72_HD && pitch % 8 == 0, "attn_d72_bwd: pitch %d: the head pitch must be >= 72 and a multiple of 8", pitch);
  ST_REQUIRE(lse2 && workspace && ((uintptr_t)workspace & 3) == 0, "attn_d72_bwd: null lse2 / workspace");
  ST_REQUIRE(d72_block_ok(q, ld_q, H, pitch) && d72_block_ok(k, ld_k, H, pitch) && d72_block_ok(v, ld_v, H, pitch) && d72_block_ok(o, ld_o, H, pitch) &&
                 d72_block_ok(dO, ld_do, H, pitch) && d72_block_ok(dq, ld_dq, H, pitch) && d72_block_ok(dk, ld_dk, H, pitch) && d72_block_ok(dv, ld_dv, H, pitch),
             "attn_d72_bwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * pitch");
  ST_REQUIRE(!key_bias || ((uintptr_t)key_bias & 3) == 0, "attn_d72_bwd: misaligned key_bias");
  float* delta = (float*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  const double fl_unit = 2.0 * (double)B * H * (double)Sq * Sk * d;
  {
    ProfScope ps(stream, ST355_K_ATTN_BWD_DQ, 3.0 * fl_unit, 2.0 * (double)B * H * (4.0 * Sq + 2.0 * Sk) * d);
    d72_launch_dq<2>(st, q, ld_q, k, ld_k, v, ld_v, o, ld_o, dO, ld_do, lse2, key_bias, dq, ld_dq, delta, B, H, Sq, Sk, pitch, scale);
    const int rc = st355_check_launch("attn_d72_dq");
    if (rc) return rc;
  }
  ProfScope ps(stream, ST355_K_ATTN_BWD_DKV, 4.0 * fl_unit, 2.0 * (double)B * H * (2.0 * Sq + 4.0 * Sk) * d);
#define D72_DKV(NT, BIAS) d72_launch_dkv<NT, BIAS>(st, q, ld_q, k, ld_k, v, ld_v, dO, ld_do, lse2, delta, key_bias, dk, ld_dk, dv, ld_dv, B, H, Sq, Sk, pitch, scale)
  if (Sk >= D72_LONG) { if (key_bias) D72_DKV(2, true); else D72_DKV(2, false); }
  else { if (key_bias) D72_DKV(1, true); else D72_DKV(1, false); }
#undef D72_DKV
  return st355_check_launch("attn_d72_dkv");
}

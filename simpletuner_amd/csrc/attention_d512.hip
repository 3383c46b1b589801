// attention_d512.hip — fused forward attention for 512-wide heads (the single head of the AutoencoderKL mid block: one head as wide as the block, over all
// S = (H/8)(W/8) latent positions), on TOKEN-MAJOR operands: q / k / v / o are the first columns of column blocks of [B*S, ld] projection buffers (row b*S + i
// holds head h at columns h*512 .. h*512 + 511) — for the VAE the three 512-column thirds of the [B*S, 3C] qkv GEMM output, used in place.  One launch for all
// images and heads; no [Sq, Sk] buffer, no transposed, padded or head-major copy of any operand.
//   O = softmax(scale Q K^T) V,   lse2 = log2 sum_j exp(scale q.k_j)  (written when the pointer is non-NULL)             (log2 convention of attn_common.h)
//
// Why not k_attn_wide_fwd<512>: its 64-row tile image is 64 KiB per operand at this width (K and V double-buffered: 256 KiB against 160 KiB of LDS), and a wave
// that owns 32 queries across the full head holds 256 O^T accumulators + 128 registers of Q.  Here the two contractions are split DIFFERENTLY over the 4 waves of
// a workgroup that owns 64 queries, and P crosses LDS between them:
//   * score phase, split by QUERIES (v_mfma_f32_16x16x32_bf16).  Wave w keeps the Q fragments of queries 16 w .. 16 w + 15 over all 512 channels in registers
//     (the B operand: B[k = 8 g + j][n = lane & 15], g = lane >> 4; 16 k-steps x 4 = 64 VGPRs) and walks the 32-key tile of K in LDS as the A operand
//     (A[i = key][k]: one ds_read_b128 per step), one fp32 chain over the whole d per score.  C[key 4 g + r][query lane & 15]: a lane owns one query, its 8
//     registers hold 8 keys; the row max meets across the four lane groups (two cross-lane exchanges), m and the lane's PARTIAL l stay in registers (the rescale
//     factor is the same in the four lanes of a query, so the partial sums need no exchange until the end).  P = exp2(s scale2 - m) is rounded to bf16 once and
//     written to LDS as P[query][key] with the row's rescale factor alpha = exp2(m_old - m_new) beside it; l sums the fp32 values.
//   * PV phase, split by OUTPUT COLUMNS (v_mfma_f32_32x32x16_bf16, the fragment maps of attn_common.h).  Wave w owns O[:, 128 w .. 128 w + 127] of all 64 queries
//     as O^T: 4 channel tiles x 2 query tiles x 16 = 128 fp32 accumulators.  O^T += V^T P^T: V^T fragments by transposing reads (ds_read_b64_tr_b16) of the
//     row-major V tile, P^T fragments are 16-byte reads of P rows (a lane owns a query column: alpha is one scalar per lane and query tile, applied only when
//     some row's maximum moved).  No wave holds a 512-wide accumulator, none holds Q for more than 16 rows.
//   * LDS: 32-key tiles, row pitch 1024 bytes: K 32 KiB + V 32 KiB, double-buffered = 128 KiB, + two slots of P (4 KiB) and of the 64 row factors: 136.5 KiB, one workgroup per CU.
//     A 1024-byte pitch puts every row on the same bank, so each image has the XOR term of the way it is read: K (16 lanes of a ds_read_b128 read 16 rows at one
//     chunk) XORs the 16-byte chunk index with row & 15 — 16 distinct slots of one 256-byte window; V (the 32 lanes of a transposing read cover 4 rows x 64 bytes)
//     XORs it with (row & 3) << 2 — the four rows land in the four 64-byte quarters of the window.  Both stay inside an aligned group of 16 chunks.  P (64-byte
//     rows) XORs its 4 chunks with (row >> 2) & 3.
//   * staging: the next tile's global loads (a wave fetches whole 1024-byte rows) are issued before the MFMA work into 64 registers and written to the other
//     buffer after it.  The phases run ONE TILE APART — an iteration takes the scores of tile kt and the P V product of tile kt - 1 in one stretch of code, so
//     their independent MFMA chains and LDS reads interleave and the softmax's VALU work runs under the P V MFMAs; the K ring is one tile ahead of the V ring
//     and P / alpha have one slot per tile parity.  One barrier per tile.
//   * grid (query blocks, H, B) through attn_wg_map(): with H*B not a multiple of 8 (the VAE: one head) consecutive workgroups are consecutive query blocks of
//     ONE image, walking its keys in the same order, so K / V tiles are fetched from HBM once and re-read from L2 / Infinity Cache by the others.
//   No atomics; every output has one owner and a fixed summation order: launches are bit-identical, and O does not depend on whether lse2 is written.
//   Ragged tails: loads clamp the row, keys past Sk get a score of -inf (P = 0 exactly), stores are guarded.
#include "attn_common.h"

#define D512_THREADS 256
#define D512_HD 512
#define D512_QB 64                 // queries per workgroup
#define D512_KT 32                 // keys per tile
#define D512_ROWB (D512_HD * 2)    // row pitch of the K / V images, bytes
#define D512_TILE (D512_KT * D512_ROWB)
#define D512_PER (D512_KT * (D512_HD / 8) / D512_THREADS)        // 16-byte chunks per thread and operand tile (8)
#define D512_P_OFF (4 * D512_TILE)
#define D512_P_BYTES (D512_QB * D512_KT * 2)
#define D512_A_OFF (D512_P_OFF + 2 * D512_P_BYTES)      // P and the row factors: two slots each (tile parity)
#define D512_LDS (D512_A_OFF + 2 * D512_QB * 4)


__device__ __forceinline__ int d512_k_off(int row, int chunk) { return row * D512_ROWB + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int d512_v_off(int row, int chunk) { return row * D512_ROWB + ((chunk ^ ((row & 3) << 2)) << 4); }
__device__ __forceinline__ int d512_p_off(int row, int chunk) { return row * (D512_KT * 2) + ((chunk ^ ((row >> 2) & 3)) << 4); }

// rows row0 .. row0 + 31 of one head's column block; rows past nrows - 1 re-read the last valid row.  A wave's 64 lanes fetch one whole row per step.
__device__ __forceinline__ void d512_load(bf16x8 (&reg)[D512_PER], const bf16* base, int64_t ld, int row0, int nrows, int tid) {
#pragma unroll
  for (int p = 0; p < D512_PER; p++) {
    const int id = p * D512_THREADS + tid;
    reg[p] = *(const bf16x8*)(base + (int64_t)min(row0 + (id >> 6), nrows - 1) * ld + (id & 63) * 8);
  }
}
template <bool V>
__device__ __forceinline__ void d512_store(const bf16x8 (&reg)[D512_PER], char* lds, int tid) {
#pragma unroll
  for (int p = 0; p < D512_PER; p++) {
    const int id = p * D512_THREADS + tid;
    *(bf16x8*)(lds + (V ? d512_v_off(id >> 6, id & 63) : d512_k_off(id >> 6, id & 63))) = reg[p];
  }
}

__global__ void __launch_bounds__(D512_THREADS, 1) k_attn_d512_fwd(const bf16* __restrict__ Q, int64_t ld_q, const bf16* __restrict__ K, int64_t ld_k,
                                                                   const bf16* __restrict__ V, int64_t ld_v, bf16* __restrict__ O, int64_t ld_o,
                                                                   float* __restrict__ lse2, int H, int Sq, int Sk, float scale2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, l15 = lane & 15;          // score phase: lane group / query of the wave's stripe
  const int h = lane >> 5, l31 = lane & 31;          // PV phase: half / query of a 32-query tile
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int q0 = wg.tile * D512_QB;
  const bf16* Kg = K + (int64_t)b * Sk * ld_k + (int64_t)head * D512_HD;
  const bf16* Vg = V + (int64_t)b * Sk * ld_v + (int64_t)head * D512_HD;

  // Q of query 16 wv + l15, channels 32 ks + 8 g + 0..7
  bf16x8 qf[D512_HD / 32];
  {
    const bf16* qrow = Q + ((int64_t)b * Sq + min(q0 + 16 * wv + l15, Sq - 1)) * ld_q + (int64_t)head * D512_HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < D512_HD / 32; ks++) qf[ks] = *(const bf16x8*)(qrow + 32 * ks);
  }
  f32x16 acc[4][2];                                  // O^T[channel 128 wv + 32 dt + 8 a + 4 h + b][query 32 qb + l31] in register 4 a + b
#pragma unroll
  for (int dt = 0; dt < 4; dt++)
#pragma unroll
    for (int qb = 0; qb < 2; qb++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[dt][qb][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // transposing reads of the V image: lane = 32 h + 16 ih + 4 r + s supplies channels 16 ih + 4 s .. + 3 of key row 8 h + r (+ 4 for the second read) and
  // receives channel 16 ih + (lane & 15) = lane & 31 of four key rows.  Row & 3 = r for every row a lane reads, so the XOR term is one constant per lane.
  int vtr[4];
  {
    const int ih = (lane >> 4) & 1, r = (lane >> 2) & 3, s = lane & 3;
#pragma unroll
    for (int dt = 0; dt < 4; dt++) vtr[dt] = d512_v_off(8 * h + r, 16 * wv + 4 * dt + 2 * ih + (s >> 1)) + (s & 1) * 8;
  }

  bf16x8 kreg[D512_PER], vreg[D512_PER];
  const int nkt = (Sk + D512_KT - 1) / D512_KT;
  auto kbuf = [&](int kt) { return smem + (kt & 1) * 2 * D512_TILE; };
  auto vbuf = [&](int kt) { return smem + (kt & 1) * 2 * D512_TILE + D512_TILE; };

  // ---- scores of the wave's 16 queries against the 32 keys of tile kt: S^T[key 16 kb + 4 g + r][query l15]
  auto score_mma = [&](int kt, f32x4 (&s)[2]) {
    const char* ks_ = kbuf(kt);
#pragma unroll
    for (int kb = 0; kb < 2; kb++) s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < D512_HD / 32; ks++)
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(ks_ + d512_k_off(16 * kb + l15, 4 * ks + g)), qf[ks], s[kb], 0, 0, 0);
  };
  // ---- online softmax of those scores; P (bf16) and the row's rescale factor go to the tile's LDS slot
  auto softmax_write = [&](int kt, f32x4 (&s)[2]) {
    char* const ps = smem + D512_P_OFF + (kt & 1) * D512_P_BYTES;
    float* const als = (float*)(smem + D512_A_OFF) + (kt & 1) * D512_QB;
    const int key0 = kt * D512_KT;
    float mt = -INFINITY;
    const bool ragged = key0 + D512_KT > Sk;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (ragged && key0 + 16 * kb + 4 * g + r >= Sk) s[kb][r] = -INFINITY;
        mt = fmaxf(mt, s[kb][r]);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = xhalf_max(mt) * scale2;                     // scale2 > 0; every tile holds at least one valid key, so mt is finite
    const float m_new = fmaxf(m_run, mt);
    const float alpha = fast_exp2(m_run - m_new);    // first tile: exp2(-inf) = 0 against zero accumulators
    m_run = m_new;
    float ls[2];
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; r++) e[r] = fast_exp2(fmaf(s[kb][r], scale2, -m_new));
      ls[kb] = (e[0] + e[1]) + (e[2] + e[3]);
      bf16x4 pk;
#pragma unroll
      for (int r = 0; r < 4; r++) pk[r] = f2bf(e[r]);
      *(bf16x4*)(ps + d512_p_off(16 * wv + l15, 2 * kb + (g >> 1)) + (g & 1) * 8) = pk;      // keys 16 kb + 4 g .. + 3 of the query's row
    }
    l_run = fmaf(l_run, alpha, ls[0] + ls[1]);
    if (g == 0) als[16 * wv + l15] = alpha;
  };
  // ---- O^T[128 channels of the wave][64 queries] += V^T P^T of tile kt
  auto pv = [&](int kt) {
    const char* ps = smem + D512_P_OFF + (kt & 1) * D512_P_BYTES;
    const float* als = (const float*)(smem + D512_A_OFF) + (kt & 1) * D512_QB;
    const char* vs = vbuf(kt);
    const float a0 = als[l31], a1 = als[32 + l31];
    if (__builtin_amdgcn_ballot_w64(a0 != 1.f || a1 != 1.f) != 0) {
#pragma unroll
      for (int dt = 0; dt < 4; dt++)
#pragma unroll
        for (int r = 0; r < 16; r++) { acc[dt][0][r] *= a0; acc[dt][1][r] *= a1; }
    }
#pragma unroll
    for (int m = 0; m < 2; m++) {                    // keys 16 m + 8 h + 0..7 are the contraction slots of the lane
      const bf16x8 p0 = *(const bf16x8*)(ps + d512_p_off(l31, 2 * m + h));
      const bf16x8 p1 = *(const bf16x8*)(ps + d512_p_off(32 + l31, 2 * m + h));
#pragma unroll
      for (int dt = 0; dt < 4; dt++) {
        const char* vp = vs + 16 * m * D512_ROWB + vtr[dt];
        const bf16x8 vf = lds_tr16x2(vp, vp + 4 * D512_ROWB);
        acc[dt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, p0, acc[dt][0], 0, 0, 0);
        acc[dt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, p1, acc[dt][1], 0, 0, 0);
      }
    }
  };

  // the two phases run one tile apart: iteration kt takes the scores of tile kt and the P V product of tile kt - 1 in one stretch of code (independent MFMA chains
  // and LDS reads for the scheduler to interleave, the softmax's VALU work under the P V MFMAs), so the K ring runs one tile ahead of the V ring
  f32x4 s[2];
  d512_load(kreg, Kg, ld_k, 0, Sk, tid);
  d512_store<false>(kreg, kbuf(0), tid);
  __syncthreads();
  if (nkt > 1) d512_load(kreg, Kg, ld_k, D512_KT, Sk, tid);
  d512_load(vreg, Vg, ld_v, 0, Sk, tid);
  score_mma(0, s);
  softmax_write(0, s);
  if (nkt > 1) d512_store<false>(kreg, kbuf(1), tid);
  d512_store<true>(vreg, vbuf(0), tid);
  __syncthreads();
  for (int kt = 1; kt < nkt; kt++) {
    if (kt + 1 < nkt) d512_load(kreg, Kg, ld_k, (kt + 1) * D512_KT, Sk, tid);
    d512_load(vreg, Vg, ld_v, kt * D512_KT, Sk, tid);
    score_mma(kt, s);
    pv(kt - 1);
    softmax_write(kt, s);
    if (kt + 1 < nkt) d512_store<false>(kreg, kbuf(kt + 1), tid);      // held K of tile kt - 1: read before the last barrier
    d512_store<true>(vreg, vbuf(kt), tid);                             // held V of tile kt - 2
    __syncthreads();
  }
  pv(nkt - 1);

  // the four lane groups of a query add their partial l; 1 / l crosses LDS to the column owners
  float* const inv_l = (float*)(smem + D512_A_OFF) + (nkt & 1) * D512_QB;      // the slot the last P V product does not read
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot = xhalf_sum(l_tot);
  if (g == 0) {
    inv_l[16 * wv + l15] = 1.f / l_tot;
    const int q = q0 + 16 * wv + l15;
    if (lse2 != nullptr && q < Sq) lse2[((int64_t)b * H + head) * Sq + q] = m_run + __log2f(l_tot);
  }
  __syncthreads();
#pragma unroll
  for (int qb = 0; qb < 2; qb++) {
    const int q = q0 + 32 * qb + l31;
    if (q >= Sq) continue;
    const float inv = inv_l[32 * qb + l31];
    bf16* row = O + ((int64_t)b * Sq + q) * ld_o + (int64_t)head * D512_HD + 128 * wv + 4 * h;
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
#pragma unroll
      for (int a = 0; a < 4; a++) {
        bf16x4 o;
#pragma unroll
        for (int bb = 0; bb < 4; bb++) o[bb] = f2bf(acc[dt][qb][4 * a + bb] * inv);
        *(bf16x4*)(row + 32 * dt + 8 * a) = o;
      }
  }
}

static bool d512_block_ok(const void* p, int64_t ld, int H, int d) { return p && ((uintptr_t)p & 15) == 0 && ld % 8 == 0 && ld >= (int64_t)H * d; }

extern "C" int st355_attn_d512_fwd(void* stream, const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, void* o, int64_t ld_o,
                                   float* lse2, int B, int H, int Sq, int Sk, int d, float scale) {
  if (d != D512_HD) { st355_set_error("attn_d512_fwd: head_dim %d not built", d); return ST355_ENOSYS; }
  ST_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq > 0 && Sk > 0, "attn_d512_fwd: bad shape B=%d H=%d Sq=%d Sk=%d", B, H, Sq, Sk);
  ST_REQUIRE(d512_block_ok(q, ld_q, H, d) && d512_block_ok(k, ld_k, H, d) && d512_block_ok(v, ld_v, H, d) && d512_block_ok(o, ld_o, H, d),
             "attn_d512_fwd: every column block needs a 16-byte aligned start and ld %% 8 == 0, ld >= H * d");
  ST_REQUIRE(scale > 0.f, "attn_d512_fwd: scale must be positive");
  ProfScope ps(stream, ST355_K_ATTN_FWD, 4.0 * (double)B * H * (double)Sq * Sk * d, 2.0 * (double)B * H * 2.0 * (Sq + Sk) * d);
  static St355AttrOnce set;
  if (set.need()) hipFuncSetAttribute((const void*)k_attn_d512_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, D512_LDS);
  hipLaunchKernelGGL(k_attn_d512_fwd, dim3((Sq + D512_QB - 1) / D512_QB, H, B), dim3(D512_THREADS), D512_LDS, (hipStream_t)stream, (const bf16*)q, ld_q,
                     (const bf16*)k, ld_k, (const bf16*)v, ld_v, (bf16*)o, ld_o, lse2, H, Sq, Sk, scale * LOG2E);
  return st355_check_launch("attn_d512_fwd");
}

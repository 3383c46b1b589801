// attention_fwd64x.hip — attention forward at head_dim 64 with 64 queries per wave, every call form of the 32-query kernel (opt-in: st355_attn_set_impl fwd = 2).
//   O = softmax(scale * Q K^T + key_bias) V,   lse2 = log2 sum_j exp2(scale log2e s_j + bias_j log2e),   O_res = bf16(O_fp32 - float(bf16(O_fp32)))
// Operands and results are those of k_attn_fwd4<64> (attention.hip): Q [B,H,Sq,64], K [B,H,Sk,64] head-major, Vt [B,H,64,Skp] with columns [Sk, Skp) zero,
// O / O_res token-major [B Sq, ld_o], lse2 [B,H,Sq]; any Sq >= 1, Sk >= 1, Sq != Sk allowed, optional fp32 key_bias [B, Sk].  Hand-written, not a tools/kgen body.
//
// Why: per score the 32-query kernel pays one LDS fragment read per MFMA and runs its exponentials next to half the MFMAs per tile that head_dim 128 has, so at
// d 64 the matrix pipe waits on LDS issue and on the VALU section.  Here a wave owns FOUR 16-query groups and every fragment it reads from LDS feeds four MFMAs.
//
// gfx950 design
//   * work split: workgroup = 256 threads = 4 waves (one per SIMD, __launch_bounds__(256, 1): the whole 512-register file of a SIMD belongs to one wave), a wave
//     owns 64 query rows as 4 groups of 16, grid (ceil(Sq / 256), H, B) through the XCD-aware map of attn_common.h.  Key tile = 64 keys.
//   * MFMA: v_mfma_f32_16x16x32_bf16 for both products, scores TRANSPOSED: S^T = K Q^T (A = 16 K rows from LDS, B = Q of 16 queries held in registers for the
//     whole key loop, two k-steps).  Result lane (n, g) = (lane & 15, lane >> 4) holds query n, rows 4 g + r of the tile, so a softmax row lives in 4 lanes: the
//     row max is 15 register max + v_permlane16_swap + v_permlane32_swap (VALU, no LDS), the row sum is reduced once, after the key loop.
//   * P never leaves the registers: the K tile is staged in PERMUTED row order — LDS row 16 t + 4 a + r holds key 32 u + 8 a + 4 b + r (t = 2 u + b) — so score
//     tile t leaves key 32 u + 8 g + 4 b + r in register r of lane (n, g), and the lane's registers of tiles 2 u, 2 u + 1, rounded to bf16 once in register order,
//     are keys 32 u + 8 g .. + 7: exactly the B operand of O^T += V^T P^T over keys 32 u .. + 31 against a PLAIN 16-byte read of row-major V^T (A operand, lane
//     (channel, g) reads keys 32 u + 8 g .. + 7).  Both operands use the same lane -> contraction-index map, which is all an MFMA needs.
//   * LDS: two K slots + two V^T slots of 64 x 64 bf16 = 32 KiB per workgroup, shared by the four waves.  Rows are 128 bytes = half of the 64 banks; 16-byte
//     chunk c of row r sits at chunk c ^ ((r >> 1) & 7) (lds_off<128>).  A 16-lane group of a ds_read_b128 reads 16 CONSECUTIVE rows at one chunk index (K: rows
//     16 t + 0..15 thanks to the permuted staging; V^T: channels 16 ct + 0..15): the 8 row pairs land on 8 different chunk positions and the two rows of a pair
//     on the two bank halves, so the 16 reads cover the 64 banks exactly once — conflict-free.  The staging stores (2 consecutive keys x 8 chunks per 16 lanes;
//     keys 2 k, 2 k + 1 map to LDS rows rho, rho + 1 with rho even) cover the banks once in the same way.  A wave reads each K / V^T fragment of a tile ONCE
//     (8 + 8 reads of 16 bytes per lane) for 64 MFMAs: half the LDS fragment traffic per score of the 32-query kernel.
//   * registers per lane: Q 32, scores of the current and the next tile 64 + 64, O^T 64, V^T fragments 32, a K fragment pair 8, P 8, staging 16 (+ 16 bias
//     values).  O^T lives in AGPRs (the MFMAs accumulate there; it comes to the VGPRs only when it is rescaled); hipcc reports 256 VGPRs + 194-198 AGPRs (226 with
//     a key bias), no scratch (profiles/attn_fwd64x_kernel_stats.md).  The allocator still moves score registers through AGPRs in places: see the profile.
//   * pipelining: the body of key tile j has two phases.  Phase 1 is VALU only: the four row maxima and rescale factors, then ONE wave-uniform branch that
//     rescales O^T only while some running max of the wave still moves.  Phase 2 is one straight-line block (the K staging guard kt + 2 < nkt sits before phase 1 and after phase 2):
//     per query group, tile j + 1's score MFMAs (K rows 16 qg .. + 15 against all four query groups: independent of everything around them), tile j's
//     exponentials + pack, tile j's PV MFMAs — so the next tile's score MFMAs and the previous group's PV MFMAs issue under the exponentials.  The two score
//     register sets swap roles in a loop unrolled by two (no copies).  Tile j + 2's K and tile j + 1's V^T travel global -> registers across the whole body
//     and are written to the slots that tile j - 1 used, after the MFMA work; ONE workgroup barrier per key tile.
//   * softmax: the EXACT running max (fp32, log2 domain, scale log2e folded into the exponent's fma), no stale reference: the error model of
//     tests/attn_bounds.py holds term by term as for k_attn_fwd4.  P is rounded to bf16 once (pack8).
//   * edges, all in this body: score columns >= Sk are -inf before the row max (their K rows are loaded from the clamped row Sk - 1, their V^T columns are the
//     zero padding, their P is exactly 0); rows >= Sq are computed from the clamped row Sq - 1 and never stored; every tile holds at least one key < Sk, so with
//     a finite bias the running max is finite from the first tile on and a row whose other keys are biased to -1e4 stays finite.
//   * no atomics, no workspace, fixed summation order: two launches are bit-identical.  Only O, O_res and lse2 are written, with vector / plain stores.
#include <type_traits>
#include "attn_common.h"

#define F64X_KT 8192            // bytes of one 64 x 64 bf16 LDS slot

__device__ __forceinline__ float f64x_max4(float x) {       // max over the four lanes l, l ^ 16, l ^ 32, l ^ 48 that share a query
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_max(fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])));
}
__device__ __forceinline__ float f64x_sum4(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return xhalf_sum(__uint_as_float(a[0]) + __uint_as_float(a[1]));
}

template <int HD, bool BIAS, bool RES>
__global__ void __launch_bounds__(256, 1) k_attn_fwd64x(const bf16* __restrict__ Q, const bf16* __restrict__ K, const bf16* __restrict__ Vt,
                                                        const float* __restrict__ key_bias, bf16* __restrict__ O, int64_t ld_o, bf16* __restrict__ Ores,
                                                        float* __restrict__ lse2, int H, int Sq, int Sk, int Skp, float scale2) {
  static_assert(HD == 64, "k_attn_fwd64x: head_dim 64");
  __shared__ __attribute__((aligned(16))) char smem[4 * F64X_KT];      // K slots 0, 1 then V^T slots 0, 1
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = lane & 15, g = lane >> 4;
  const WgMap wg = attn_wg_map();
  const int head = wg.head, b = wg.b;
  const int64_t bh = (int64_t)b * H + head;
  const int q0 = wg.tile * 256 + wv * 64;
  const bf16* Kg = K + bh * (int64_t)Sk * HD;
  const bf16* Vg = Vt + bh * (int64_t)HD * Skp;
  const int nkt = (Sk + 63) >> 6;

  bf16x8 qf[4][2];
#pragma unroll
  for (int qg = 0; qg < 4; qg++) {
    const bf16* qrow = Q + (bh * Sq + min(q0 + 16 * qg + n, Sq - 1)) * (int64_t)HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) qf[qg][ks] = *(const bf16x8*)(qrow + 32 * ks);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int qg = 0; qg < 4; qg++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[qg][ct][r] = 0.f;
  float m_run[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l_run[4] = {0.f, 0.f, 0.f, 0.f};

  // staging: a 64 x 64 bf16 tile is 512 sixteen-byte chunks, two per thread: chunk id = 256 p + tid -> row id >> 3, chunk column id & 7
  bf16x8 kst[2], vst[2];
  auto load_k = [&](int kt) {          // K rows key0 .. key0 + 63, rows >= Sk clamped to Sk - 1 (their score columns are masked)
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int id = 256 * p + tid;
      kst[p] = *(const bf16x8*)(Kg + (int64_t)min(64 * kt + (id >> 3), Sk - 1) * HD + 8 * (id & 7));
    }
  };
  auto load_v = [&](int kt) {          // V^T columns key0 .. key0 + 63 of the 64 channel rows: inside Skp (nkt * 64 <= Skp), zero past Sk
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int id = 256 * p + tid;
      vst[p] = *(const bf16x8*)(Vg + (int64_t)(id >> 3) * Skp + 64 * kt + 8 * (id & 7));
    }
  };
  auto store_k = [&](int slot) {       // key 32 u + 8 a + 4 b + r -> LDS row 16 (2 u + b) + 4 a + r
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int id = 256 * p + tid, kr = id >> 3;
      const int rho = 16 * (2 * (kr >> 5) + ((kr >> 2) & 1)) + 4 * ((kr >> 3) & 3) + (kr & 3);
      *(bf16x8*)(smem + slot * F64X_KT + lds_off<128>(rho, id & 7)) = kst[p];
    }
  };
  auto store_v = [&](int slot) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int id = 256 * p + tid;
      *(bf16x8*)(smem + (2 + slot) * F64X_KT + lds_off<128>(id >> 3, id & 7)) = vst[p];
    }
  };
  // S^T tiles of all four query groups against the K slot: every K fragment is read once and feeds four MFMAs
  auto scores = [&](int slot, f32x4 (&s)[4][4]) {
    const char* ks = smem + slot * F64X_KT;
    bf16x8 kf[4][2];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int c = 0; c < 2; c++) kf[t][c] = *(const bf16x8*)(ks + lds_off<128>(16 * t + n, 4 * c + g));
#pragma unroll
    for (int qg = 0; qg < 4; qg++)
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        s[qg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][0], qf[qg][0], z, 0, 0, 0);
        s[qg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][1], qf[qg][1], s[qg][t], 0, 0, 0);
      }
  };

  load_k(0);
  load_v(0);
  store_k(0);
  store_v(0);
  if (nkt > 1) {
    load_k(1);
    store_k(1);
  }
  __syncthreads();
  f32x4 sa[4][4], sb[4][4];
  scores(0, sa);
  __syncthreads();                     // tile 0 ends by writing K slot 0 again

  // key tile kt: cur = its scores (raw MFMA sums), nxt = where tile kt + 1's scores go (LAST: untouched)
  auto tile = [&](int kt, f32x4 (&cur)[4][4], f32x4 (&nxt)[4][4], auto masked_c, auto last_c) {
    constexpr bool MASKED = decltype(masked_c)::value, LAST = decltype(last_c)::value;
    const int key0 = 64 * kt;
    if (!LAST) {
      if (kt + 2 < nkt) load_k(kt + 2);      // workgroup-uniform: the last two tiles stage no K
      load_v(kt + 1);
    }
    // MASKED: per-key additive term in log2 units for the lane's 16 keys of the tile (register (t, r) = key0 + 32 (t >> 1) + 8 g + 4 (t & 1) + r), -inf at keys >= Sk
    float kb2[4][4];
    if (MASKED) {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int key = key0 + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r;
          float v = 0.f;
          if (BIAS) v = key_bias[(int64_t)b * Sk + min(key, Sk - 1)] * LOG2E;
          kb2[t][r] = key < Sk ? v : -INFINITY;
        }
    }
    const char* ks = smem + ((kt + 1) & 1) * F64X_KT;
    const char* vs = smem + (2 + (kt & 1)) * F64X_KT;
    // phase 1: the four row maxima and rescale factors (VALU only), then ONE wave-uniform branch: O^T is rescaled only while some running max still moves
    float alpha[4], m_new[4];
#pragma unroll
    for (int qg = 0; qg < 4; qg++) {
      float mt = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (MASKED) cur[qg][t][r] = fmaf(cur[qg][t][r], scale2, kb2[t][r]);      // scores rewritten in place, already scaled
          mt = fmaxf(mt, cur[qg][t][r]);
        }
      if (!MASKED) mt *= scale2;                   // scale2 > 0: max(scale2 s) = scale2 max(s)
      m_new[qg] = fmaxf(m_run[qg], f64x_max4(mt));
      alpha[qg] = fast_exp2(m_run[qg] - m_new[qg]);
      m_run[qg] = m_new[qg];
    }
    if (__builtin_amdgcn_ballot_w64(alpha[0] != 1.f || alpha[1] != 1.f || alpha[2] != 1.f || alpha[3] != 1.f) != 0) {
#pragma unroll
      for (int qg = 0; qg < 4; qg++)
#pragma unroll
        for (int ct = 0; ct < 4; ct++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc[qg][ct][r] *= alpha[qg];
    }
    // phase 2, one straight-line block: per query group tile kt + 1's score MFMAs (independent work), the exponentials + pack, the PV MFMAs
    const float psc = MASKED ? 1.f : scale2;       // plain tiles keep the RAW score: the scale rides in the exponent's fma
    bf16x8 vf[4][2];
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
      for (int u = 0; u < 2; u++) vf[ct][u] = *(const bf16x8*)(vs + lds_off<128>(16 * ct + n, 4 * u + g));
#pragma unroll
    for (int qg = 0; qg < 4; qg++) {
      if (!LAST) {                     // K rows 16 qg .. + 15 of tile kt + 1 against all four query groups: the fragment pair is read once, feeds 8 MFMAs
        const bf16x8 k0 = *(const bf16x8*)(ks + lds_off<128>(16 * qg + n, g)), k1 = *(const bf16x8*)(ks + lds_off<128>(16 * qg + n, 4 + g));
#pragma unroll
        for (int q2 = 0; q2 < 4; q2++) {
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          nxt[q2][qg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[q2][0], z, 0, 0, 0);
          nxt[q2][qg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[q2][1], nxt[q2][qg], 0, 0, 0);
        }
      }
      float ls[2] = {0.f, 0.f};
      bf16x8 pf[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          e[j] = fast_exp2(fmaf(cur[qg][2 * u + (j >> 2)][j & 3], psc, -m_new[qg]));
          ls[j & 1] += e[j];
        }
        pf[u] = pack8(e);
      }
      l_run[qg] = l_run[qg] * alpha[qg] + (ls[0] + ls[1]);
#pragma unroll
      for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int u = 0; u < 2; u++) acc[qg][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[ct][u], pf[u], acc[qg][ct], 0, 0, 0);
    }
    if (!LAST) {
      if (kt + 2 < nkt) store_k(kt & 1);     // K slot of tile kt (read while tile kt - 1 ran) <- tile kt + 2
      store_v((kt + 1) & 1);           // V^T slot of tile kt - 1 <- tile kt + 1
      __syncthreads();
    }
  };
  const std::integral_constant<bool, BIAS> all_masked;
  const std::false_type no;
  const std::true_type yes;
  int kt = 0;
  for (; kt + 2 < nkt; kt += 2) {
    tile(kt, sa, sb, all_masked, no);
    tile(kt + 1, sb, sa, all_masked, no);
  }
  const bool ragged = BIAS || (Sk & 63) != 0;
  if (nkt - kt == 2) {
    tile(kt, sa, sb, all_masked, no);
    if (ragged) tile(kt + 1, sb, sa, yes, yes);
    else tile(kt + 1, sb, sa, no, yes);
  } else {
    if (ragged) tile(kt, sa, sb, yes, yes);
    else tile(kt, sa, sb, no, yes);
  }

  // O^T tile ct of query group qg: lane (n, g) holds channels 16 ct + 4 g + r of query q0 + 16 qg + n
#pragma unroll
  for (int qg = 0; qg < 4; qg++) {
    const float l_tot = f64x_sum4(l_run[qg]);
    const float inv = 1.f / l_tot;
    const int q = q0 + 16 * qg + n;
    if (q < Sq) {
      const int64_t off = ((int64_t)b * Sq + q) * ld_o + (int64_t)head * HD + 4 * g;
#pragma unroll
      for (int ct = 0; ct < 4; ct++) {
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = f2bf(acc[qg][ct][r] * inv);
        *(bf16x4*)(O + off + 16 * ct) = o;
        if (RES) {                     // the rounding residual of O: O + O_res carries 16 mantissa bits of the fp32 output
          bf16x4 rs;
#pragma unroll
          for (int r = 0; r < 4; r++) rs[r] = f2bf(acc[qg][ct][r] * inv - bf2f(o[r]));
          *(bf16x4*)(Ores + off + 16 * ct) = rs;
        }
      }
      if (g == 0) lse2[bh * Sq + q] = m_run[qg] + __log2f(l_tot);
    }
  }
}

// launched by attn_fwd_impl (attention.hip) on the route ST355_ATTN_ROUTE_FWD64X; shapes are checked there
void attn_fwd64x_launch(void* stream, const void* Q, const void* K, const void* Vt, const float* key_bias, void* O, int64_t ld_o, void* O_res, float* lse2,
                        int B, int H, int Sq, int Sk, int Skp, float scale2) {
  const dim3 grid((Sq + 255) / 256, H, B);
#define ST355_FWD64X_LAUNCH(BIAS_, RES_)                                                                                                          \
  hipLaunchKernelGGL((k_attn_fwd64x<64, BIAS_, RES_>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)Q, (const bf16*)K, (const bf16*)Vt, \
                     key_bias, (bf16*)O, ld_o, (bf16*)O_res, lse2, H, Sq, Sk, Skp, scale2)
  if (key_bias && O_res) ST355_FWD64X_LAUNCH(true, true);
  else if (key_bias) ST355_FWD64X_LAUNCH(true, false);
  else if (O_res) ST355_FWD64X_LAUNCH(false, true);
  else ST355_FWD64X_LAUNCH(false, false);
#undef ST355_FWD64X_LAUNCH
}

// tlora.hip — T-LoRA (LyCORIS `algo: tlora`): y_b = base(x_b) + s (mask_b . (x_b A^T)) B^T, mask_b = the first r_b rank columns, r_b a function of sample b's timestep.
//
//   st355_tlora_mask   t[m, g r_pad + j] = +0  iff  j >= r_active(sample(m)),  for g < G and j < rank; in place, everything else untouched
//
// The operand is a rank-space product of a LoraGroup: T = x A_cat^T in the forward and in every recompute pass, U = dy B_blk_T in the backward (bf16, G targets of
// r_pad columns each, `rank` of them real).  sample(m) = m / rows_per_sample over the LOGICAL rows; a row's address comes from row_off() as in lora_dropout.hip
// (compact, or a [B, rows, C] view of a joint buffer).  r_active = table[clamp(trunc(timesteps[sample]), 0, T)]: the table of T + 1 active ranks is built on the
// host once, the timestep is read from the device in the dtype the component received it — nothing is read on the host, so a captured step replays with
// whatever timesteps sit in its static input.
//
// One lane owns one 16-byte group of eight columns (r_pad % 32 == 0: a group never straddles two targets).  Survivors are never read: a group below the active rank
// is skipped, a group inside [r_active, rank) is one 16-byte zero store, and only the group that holds the boundary (of the active rank, or of `rank` against the
// padding columns [rank, r_pad)) is read, edited and written back.  Columns [G r_pad, ld) are outside every lane's range.
#include "common.h"

struct TloraArgs {
  bf16* t;
  int64_t ld, seg_stride;
  uint32_t seg_rows, rows_per_sample, M, B;
  int G, r_pad, rank, T, ts_kind;
  const void* timesteps;
  const int32_t* table;
};

__device__ __forceinline__ int64_t tl_row_off(uint32_t m, int64_t ld, uint32_t seg_rows, int64_t seg_stride) {
  if (seg_rows == 0) return (int64_t)m * ld;
  const uint32_t s = m / seg_rows;
  return ((int64_t)s * seg_stride + (int64_t)(m - s * seg_rows)) * ld;
}
// int(t) of the reference (truncation towards zero), clamped to the table; a NaN reads entry 0
__device__ __forceinline__ int tl_index(const TloraArgs& a, uint32_t b) {
  if (a.ts_kind == ST355_TS_I64) {
    const int64_t v = ((const int64_t*)a.timesteps)[b];
    return v < 0 ? 0 : (v > a.T ? a.T : (int)v);
  }
  const float f = a.ts_kind == ST355_TS_BF16 ? bf2f(((const bf16*)a.timesteps)[b]) : ((const float*)a.timesteps)[b];
  if (!(f >= 1.f)) return 0;
  return f >= (float)a.T ? a.T : (int)f;
}

__global__ void __launch_bounds__(256) k_tlora_mask(TloraArgs a) {
  const int cpr = (a.G * a.r_pad) >> 3;                         // 16-byte groups per row
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.M * cpr) return;
  const uint32_t m = (uint32_t)(idx / cpr);
  const int c = (int)(idx - (int64_t)m * cpr);
  const int j0 = (c << 3) % a.r_pad;                            // first column of this group inside its target
  if (j0 >= a.rank) return;                                     // padding columns only
  uint32_t b = m / a.rows_per_sample;
  if (b >= a.B) b = a.B - 1;                                    // (the host checked M == B rows_per_sample)
  int r = a.table[tl_index(a, b)];
  r = r < 0 ? 0 : (r > a.rank ? a.rank : r);
  if (j0 + 8 <= r) return;                                      // survivors: never read
  bf16* p = a.t + tl_row_off(m, a.ld, a.seg_rows, a.seg_stride) + (c << 3);
  if (j0 >= r && j0 + 8 <= a.rank) {
    *(u32x4*)p = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  u32x4 v = *(const u32x4*)p;                                   // the boundary group
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const int jl = j0 + 2 * w, jh = jl + 1;
    const uint32_t keep = ((jl >= r && jl < a.rank) ? 0u : 0x0000FFFFu) | ((jh >= r && jh < a.rank) ? 0u : 0xFFFF0000u);
    v[w] &= keep;
  }
  *(u32x4*)p = v;
}

extern "C" int st355_tlora_mask(void* stream, void* t, int64_t ld, int64_t seg_rows, int64_t seg_stride, int64_t M, int64_t rows_per_sample, int G, int r_pad,
                                int rank, const void* timesteps, int ts_kind, int64_t B, const int32_t* ranks_table, int T) {
  ST_REQUIRE(t && timesteps && ranks_table, "tlora_mask: null pointer");
  ST_REQUIRE(r_pad == 32 || (r_pad >= 64 && r_pad % 64 == 0), "tlora_mask: r_pad must be 32 or a multiple of 64 (got %d)", r_pad);
  ST_REQUIRE(G >= 1 && G <= 4, "tlora_mask: 1 .. 4 targets (got %d)", G);
  ST_REQUIRE(rank >= 1 && rank <= r_pad, "tlora_mask: rank %d outside 1 .. r_pad = %d", rank, r_pad);
  ST_REQUIRE(ld % 8 == 0 && ld >= (int64_t)G * r_pad && ((uintptr_t)t & 15) == 0, "tlora_mask: the operand needs 16-byte aligned rows of at least G r_pad = %d columns (ld %lld)",
             G * r_pad, (long long)ld);
  ST_REQUIRE(M > 0 && M < (1ll << 31) && B > 0 && rows_per_sample > 0 && M == B * rows_per_sample,
             "tlora_mask: M (%lld) must equal timesteps (%lld) x rows_per_sample (%lld)", (long long)M, (long long)B, (long long)rows_per_sample);
  ST_REQUIRE(seg_rows == 0 || (seg_rows > 0 && M % seg_rows == 0 && seg_stride >= seg_rows), "tlora_mask: seg_rows must divide M, the segment stride be >= seg_rows");
  ST_REQUIRE(ts_kind == ST355_TS_F32 || ts_kind == ST355_TS_BF16 || ts_kind == ST355_TS_I64, "tlora_mask: timesteps must be fp32, bf16 or int64 (kind %d)", ts_kind);
  ST_REQUIRE(T >= 1 && T < (1 << 24), "tlora_mask: the table holds T + 1 entries, 1 <= T < 2^24 (got %d)", T);
  TloraArgs a;
  a.t = (bf16*)t; a.ld = ld; a.seg_stride = seg_stride; a.seg_rows = (uint32_t)seg_rows; a.rows_per_sample = (uint32_t)rows_per_sample; a.M = (uint32_t)M;
  a.B = (uint32_t)B; a.G = G; a.r_pad = r_pad; a.rank = rank; a.T = T; a.ts_kind = ts_kind; a.timesteps = timesteps; a.table = ranks_table;
  const int64_t n = M * ((G * r_pad) >> 3);
  // written at most: every group of [0, rank) zeroed; read: the boundary groups
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 0.0, 2.0 * M * G * rank);
  hipLaunchKernelGGL(k_tlora_mask, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return st355_check_launch("tlora_mask");
}

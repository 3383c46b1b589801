// optim_common.h — the streaming shell shared by the arena optimizer kernels (optim.hip, lion.hip): grid sizing, the fused EMA tail in both
// arena dtypes, and the bf16 mirror of an fp32 arena.  Only what is identical between the optimizers lives here; each update rule stays in its file.
#pragma once
#include "common.h"

// 16 bytes per lane, at most 2048 workgroups of 256, grid-stride
#define OP_THREADS 256
static inline int op_blocks(int64_t items) {
  int64_t b = cdiv64(items, OP_THREADS);
  if (b > 256 * 8) b = 256 * 8;
  if (b < 1) b = 1;
  return (int)b;
}

// s -= (1-d) (s - p)      (ema.py:423: torch._foreach_sub_(s, torch._foreach_sub(s, p), alpha=1-d)); omd = 1 - d.
// THE rounding rule of every EMA update in the library: the reference materialises (s - p) in the parameter dtype (ema.py:393-433), so for
// bf16 the difference is rounded to bf16 before it is scaled; for fp32 the cast is the identity.
template <typename T>
__device__ __forceinline__ T ema_one(T s, T p, float omd) {
  const float sf = (float)s;
  const T diff = (T)(sf - (float)p);
  return (T)(sf - omd * (float)diff);
}

// fused EMA tail of an fp32 arena step: lane i's four updated parameters pv
__device__ __forceinline__ void ema_tail_f32x4(float* ema, int64_t i, f32x4 pv, float omd) {
  f32x4 ev = *(f32x4*)(ema + i * 4);
#pragma unroll
  for (int j = 0; j < 4; j++) ev[j] = ema_one(ev[j], pv[j], omd);
  *(f32x4*)(ema + i * 4) = ev;
}

// fused EMA tail of a bf16 arena step: lane i's eight updated parameters pb
__device__ __forceinline__ void ema_tail_bf16x8(bf16* ema, int64_t i, bf16x8 pb, float omd) {
  bf16x8 eb = *(bf16x8*)(ema + i * 8);
#pragma unroll
  for (int j = 0; j < 8; j++) eb[j] = ema_one(eb[j], pb[j], omd);
  *(bf16x8*)(ema + i * 8) = eb;
}

// bf16 mirror of an fp32 arena (the GEMM operand copy), written in the same pass
__device__ __forceinline__ void mirror_store_bf16x4(bf16* pb, int64_t i, f32x4 pv) {
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = f2bf(pv[j]);
  *(bf16x4*)(pb + i * 4) = o;
}

// the scalar forms of both, for the n % 4 element tail of the fp32 kernels; either pointer may be null.  (The vector pieces above take their
// operands by value and the mirror store below forms its address first: with these spellings k_adamw_* and k_lion_* compile to the same
// instruction stream as the open-coded tails they replace.)
__device__ __forceinline__ void ema_mirror_one(float* ema, bf16* pb, int64_t i, float pv, float omd) {
  if (ema) ema[i] = ema_one(ema[i], pv, omd);
  if (pb) { bf16* q = pb + i; *q = f2bf(pv); }
}

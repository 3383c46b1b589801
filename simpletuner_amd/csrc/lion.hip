// lion.hip — K16c: Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms"; the registry's "optimi-lion") as one streaming pass over
// a flat parameter arena.  One momentum buffer, no square root, no division:
//   fp32 arena: p, m read + written, g read = 20 B/param (+8 with ema, +2 with p_bf16)
//   bf16 arena: p, m, comp read + written, g read = 14 B/param (10 without the compensation buffer, +4 with ema)
// against 28 and 22 for st355_adamw_ema_step*.  Same layout as k_adamw_*: 16 bytes per lane, at most 2048 workgroups of 256, grid-stride.
//
// Per element, fp32 internally, in this order (tests/lion_bounds.py counts its roundings off it):
//   g' = g grad_scale
//   c  = m + (g' - m)(1 - beta1)          s = sign(c) in {-1, 0, +1}   (sign(0) = 0: lora_A's first gradient is exactly 0 while B = 0)
//   m' = m + (g' - m)(1 - beta2)
//   d  = -lr s - (lr wd) p                decoupled decay (optimi's decouple_lr=False)
//   fp32 arena:             p' = p + d
//   bf16 arena, no comp:    p' = bf16(p + d)
//   bf16 arena, comp:       t = comp + d ; p' = bf16(p + t) ; comp' = bf16(t - (p' - p))       (Kahan: what the rounding of p' dropped is carried)
// The decay goes through the compensated sum on purpose: a bf16 p *= 1 - lr wd rounds the decay away whenever lr wd < 2^-9.
#include "optim_common.h"

struct LionC {
  float lr, omb1, omb2, lrwd, grad_scale, ema_omd;   // omb = 1 - beta, lrwd = lr * weight_decay, ema_omd = 1 - ema_decay: all formed in fp32
};

// m is updated in place (fp32); returns d
__device__ __forceinline__ float lion_one(float p, float g, float& m, const LionC& c) {
  g *= c.grad_scale;
  const float diff = g - m;
  const float cc = m + diff * c.omb1;
  const float s = (float)(cc > 0.f) - (float)(cc < 0.f);
  m = m + diff * c.omb2;
  return -c.lr * s - c.lrwd * p;
}
// d == 0 (a zero gradient on a zero momentum, no decay) leaves the parameter's bits alone, also those of -0
__device__ __forceinline__ float lion_apply(float p, float d) { return d == 0.f ? p : p + d; }

__global__ void __launch_bounds__(OP_THREADS) k_lion_f32(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ ema, bf16* __restrict__ pb, int64_t n, LionC c) {
  const int64_t nv = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = *(f32x4*)(p + i * 4), gv = *(const f32x4*)(g + i * 4), mv = *(f32x4*)(m + i * 4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float mj = mv[j];
      const float d = lion_one(pv[j], gv[j], mj, c);
      pv[j] = lion_apply(pv[j], d); mv[j] = mj;
    }
    *(f32x4*)(p + i * 4) = pv;
    *(f32x4*)(m + i * 4) = mv;
    if (ema) ema_tail_f32x4(ema, i, pv, c.ema_omd);
    if (pb) mirror_store_bf16x4(pb, i, pv);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
    const int64_t i = (nv << 2) + threadIdx.x;
    float mv = m[i];
    const float pv = lion_apply(p[i], lion_one(p[i], g[i], mv, c));
    p[i] = pv; m[i] = mv;
    ema_mirror_one(ema, pb, i, pv, c.ema_omd);
  }
}

__global__ void __launch_bounds__(OP_THREADS) k_lion_bf16(bf16* __restrict__ p, const bf16* __restrict__ g, bf16* __restrict__ m,
                                                         bf16* __restrict__ comp, bf16* __restrict__ ema, int64_t n, LionC c) {
  const int64_t nv = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    bf16x8 pb = *(bf16x8*)(p + i * 8), gb = *(const bf16x8*)(g + i * 8), mb = *(bf16x8*)(m + i * 8);
    if (comp) {
      bf16x8 cb = *(bf16x8*)(comp + i * 8);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float pj = bf2f(pb[j]);
        float mj = bf2f(mb[j]);
        const float t = bf2f(cb[j]) + lion_one(pj, bf2f(gb[j]), mj, c);
        const bf16 pn = t == 0.f ? pb[j] : f2bf(pj + t);
        cb[j] = f2bf(t - (bf2f(pn) - pj));
        pb[j] = pn; mb[j] = f2bf(mj);
      }
      *(bf16x8*)(comp + i * 8) = cb;
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float pj = bf2f(pb[j]);
        float mj = bf2f(mb[j]);
        const float d = lion_one(pj, bf2f(gb[j]), mj, c);
        pb[j] = d == 0.f ? pb[j] : f2bf(pj + d); mb[j] = f2bf(mj);
      }
    }
    *(bf16x8*)(p + i * 8) = pb;
    *(bf16x8*)(m + i * 8) = mb;
    if (ema) ema_tail_bf16x8(ema, i, pb, c.ema_omd);
  }
}

static LionC make_lion(float lr, float b1, float b2, float wd, float gs, float ema_decay) {
  LionC c;
  c.lr = lr; c.omb1 = 1.f - b1; c.omb2 = 1.f - b2; c.lrwd = lr * wd; c.grad_scale = gs; c.ema_omd = 1.f - ema_decay;
  return c;
}

extern "C" int st355_lion_step(void* stream, float* p, const float* g, float* m, float* ema, void* p_bf16, int64_t n, float lr, float beta1,
                               float beta2, float weight_decay, float grad_scale, float ema_decay) {
  ST_REQUIRE(p && g && m && n > 0, "lion_step: bad args");
  ST_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)ema % 16 == 0) && ((uintptr_t)p_bf16 % 8 == 0),
             "lion_step: arena must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_OPTIM, 8.0 * n, (20.0 + (ema ? 8.0 : 0.0) + (p_bf16 ? 2.0 : 0.0)) * n);
  LionC c = make_lion(lr, beta1, beta2, weight_decay, grad_scale, ema_decay);
  hipLaunchKernelGGL(k_lion_f32, dim3(op_blocks(n / 4 + 1)), dim3(OP_THREADS), 0, (hipStream_t)stream, p, g, m, ema, (bf16*)p_bf16, n, c);
  return st355_check_launch("lion_step");
}

extern "C" int st355_lion_step_bf16(void* stream, void* p, const void* g, void* m, void* comp, void* ema, int64_t n, float lr, float beta1,
                                    float beta2, float weight_decay, float grad_scale, float ema_decay) {
  ST_REQUIRE(p && g && m && n > 0 && n % 8 == 0, "lion_step_bf16: bad args (n must be a multiple of 8)");
  ST_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)comp % 16 == 0) && ((uintptr_t)ema % 16 == 0),
             "lion_step_bf16: arena must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_OPTIM, 8.0 * n, ((comp ? 14.0 : 10.0) + (ema ? 4.0 : 0.0)) * n);
  LionC c = make_lion(lr, beta1, beta2, weight_decay, grad_scale, ema_decay);
  hipLaunchKernelGGL(k_lion_bf16, dim3(op_blocks(n / 8)), dim3(OP_THREADS), 0, (hipStream_t)stream, (bf16*)p, (const bf16*)g, (bf16*)m,
                     (bf16*)comp, (bf16*)ema, n, c);
  return st355_check_launch("lion_step_bf16");
}

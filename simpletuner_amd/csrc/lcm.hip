// lcm.hip — LCM distillation of the epsilon / v families (distillation_method=lcm; helpers/distillation/lcm/__init__.py, DDPM branch) and its few-step sampler:
// four streaming passes.
//
//   (a_t, s_t) = sched[clamp(t, 0, T - 1)] = (sqrt(acp_t), sqrt(1 - acp_t));   x0 / eps of a prediction p at a sample x:
//       mode 0 (epsilon):  x0 = (x - s p) / a,  eps = p            mode 1 (v):  x0 = a x - s p,  eps = a p + s x
//   boundary scalings of a timestep t, S = timestep_scaling t:   c_skip = 0.25 / (S^2 + 0.25),   c_out = S / sqrt(S^2 + 0.25)      (c_skip(0) = 1, c_out(0) = 0)
//
//   st355_lcm_solver_step   p = p_u + w (p_c - p_u) of the teacher pair [2B, n] (conditional rows first);  x0, eps at (x_s, start);
//                           x_prev = prev[index].0 x0 + prev[index].1 eps, prev = (sqrt(acp_prev), sqrt(1 - acp_prev)) [N, 2]; written in fp32 AND in bf16
//   st355_lcm_target        x0_t of p_t at (x_prev fp32, t);  target = c_skip(t) x_prev + c_out(t) x0_t   in fp32  (t = 0: target = x_prev exactly)
//   st355_lcm_loss          m = c_skip(start) x_s + c_out(start) x0(pred at start);  d = m - target;  l2: d^2, huber: sqrt(d^2 + c^2) - c;  per-sample mean, batch mean;
//                           d(loss)/d(pred) = grad_scale g(d) c_out(start) (dx0/dp) / (B n), g = 2 d or d / sqrt(d^2 + c^2), dx0/dp = -s/a or -s, in ONE bf16 write
//   st355_lcm_sample_step   one LCMScheduler step: denoised = c_skip(t) x + c_out(t) x0(pred at t);  out = sqrt(acp_next) denoised + sqrt(1 - acp_next) noise, or (last
//                           step, t_next < 0) denoised
//
// Every coefficient is gathered in the kernel from device-resident index / timesteps and the fp32 tables (nothing is read on the host), the index clamped before the
// gather.  16 bytes per lane where the per-sample size is a multiple of 8 and the pointers are 16-byte aligned, else the same walk with scalar accesses, the n % 8 tail
// included.  The loss reduction runs in two stages in a fixed order — stage 1: `parts` workgroups per sample, lane tree, wave partials in wave order; stage 2, on the
// device: the partials in index order — so every output repeats bit for bit.  No atomics.
#include "feature_common.h"

#define LCM_THREADS OP_THREADS

extern "C" int64_t st355_lcm_workspace(int64_t batch, int64_t per_sample) {
  if (batch <= 0 || per_sample <= 0) return 0;
  return (int64_t)sizeof(float) * batch * sample_parts(batch, per_sample);
}

__device__ __forceinline__ int64_t lcm_clamp(int64_t t, int len) { return t < 0 ? 0 : (t > len - 1 ? len - 1 : t); }

// (c_skip, c_out) of timestep t (already clamped to the schedule), sigma_data = 0.5
__device__ __forceinline__ void lcm_scalings(int64_t t, float scaling, float& c_skip, float& c_out) {
  const float S = scaling * (float)t;
  const float q = S * S + 0.25f;
  c_skip = 0.25f / q;
  c_out = S / sqrtf(q);
}

template <int MODE>
__device__ __forceinline__ float lcm_x0(float x, float p, float a, float s) {
  return MODE == 0 ? (x - s * p) / a : a * x - s * p;
}

template <int MODE>
__device__ __forceinline__ float lcm_eps(float x, float p, float a, float s) {
  return MODE == 0 ? p : a * p + s * x;
}

// ---- the solver step: CFG combine, x0 / eps, DDIM step.  grid = (parts, B) ----
struct LcmSolverArgs {
  const bf16 *x, *pair;
  const float* w;
  const int64_t *index, *start;
  const float *sched, *prev;
  float* out32;
  bf16* out16;
  int64_t per_sample, batch;
  int sched_len, prev_len;
};

template <int MODE, bool VEC>
__global__ void __launch_bounds__(LCM_THREADS) k_lcm_solver(const LcmSolverArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.per_sample, groups = (n + 7) >> 3;
  const bf16* __restrict__ x_ = a.x + (int64_t)b * n;
  const bf16* __restrict__ pc_ = a.pair + (int64_t)b * n;
  const bf16* __restrict__ pu_ = a.pair + ((int64_t)b + a.batch) * n;
  float* __restrict__ o32 = a.out32 + (int64_t)b * n;
  bf16* __restrict__ o16 = a.out16 + (int64_t)b * n;
  const int64_t ts = lcm_clamp(a.start[b], a.sched_len), ix = lcm_clamp(a.index[b], a.prev_len);          // the gathers never leave their tables
  const float al = a.sched[2 * ts], sg = a.sched[2 * ts + 1];
  const float ap = a.prev[2 * ix], sp = a.prev[2 * ix + 1];
  const float w = a.w[b];
  for (int64_t i = (int64_t)blockIdx.x * LCM_THREADS + threadIdx.x; i < groups; i += (int64_t)gridDim.x * LCM_THREADS) {
    const int64_t e0 = i * 8;
    const int cnt = (n - e0) >= 8 ? 8 : (int)(n - e0);
    float xv[8], cv[8], uv[8], ov[8];
    load8<VEC>(x_, e0, cnt, xv);
    load8<VEC>(pc_, e0, cnt, cv);
    load8<VEC>(pu_, e0, cnt, uv);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = uv[j] + w * (cv[j] - uv[j]);
      ov[j] = ap * lcm_x0<MODE>(xv[j], p, al, sg) + sp * lcm_eps<MODE>(xv[j], p, al, sg);
    }
    store8<VEC>(o32, e0, cnt, ov);
    store8<VEC>(o16, e0, cnt, ov);
  }
}

extern "C" int st355_lcm_solver_step(void* stream, const void* x_s, const void* teacher_pair, const float* w, const int64_t* index, const int64_t* start,
                                     const float* sched, int sched_len, const float* prev, int prev_len, int mode, float* x_prev32, void* x_prev16, int64_t batch,
                                     int64_t per_sample) {
  ST_REQUIRE(x_s && teacher_pair && w && index && start && sched && prev && x_prev32 && x_prev16, "lcm_solver_step: null pointer");
  ST_REQUIRE((mode == 0 || mode == 1) && sched_len > 0 && prev_len > 0 && per_sample > 0 && batch > 0 && batch < 32768,
             "lcm_solver_step: bad args (mode %d, sched_len %d, prev_len %d, batch %ld)", mode, sched_len, prev_len, (long)batch);
  const bool vec = per_sample % 8 == 0 && (((uintptr_t)x_s | (uintptr_t)teacher_pair | (uintptr_t)x_prev32 | (uintptr_t)x_prev16) & 15) == 0;
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 12.0 * n, 12.0 * n);
  LcmSolverArgs a;
  a.x = (const bf16*)x_s; a.pair = (const bf16*)teacher_pair; a.w = w; a.index = index; a.start = start; a.sched = sched; a.prev = prev; a.out32 = x_prev32;
  a.out16 = (bf16*)x_prev16; a.per_sample = per_sample; a.batch = batch; a.sched_len = sched_len; a.prev_len = prev_len;
  const dim3 grid(sample_parts(batch, per_sample), (unsigned)batch), block(LCM_THREADS);
  if (mode == 0) {
    if (vec) hipLaunchKernelGGL((k_lcm_solver<0, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_solver<0, false>), grid, block, 0, (hipStream_t)stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_lcm_solver<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_solver<1, false>), grid, block, 0, (hipStream_t)stream, a);
  }
  return st355_check_launch("lcm_solver_step");
}

// ---- the consistency target.  grid = (parts, B) ----
struct LcmTargetArgs {
  const float* xprev;
  const bf16* pred;
  const int64_t* t;
  const float* sched;
  float* target;
  int64_t per_sample;
  int sched_len;
  float scaling;
};

template <int MODE, bool VEC>
__global__ void __launch_bounds__(LCM_THREADS) k_lcm_target(const LcmTargetArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.per_sample, groups = (n + 7) >> 3;
  const float* __restrict__ x_ = a.xprev + (int64_t)b * n;
  const bf16* __restrict__ p_ = a.pred + (int64_t)b * n;
  float* __restrict__ o_ = a.target + (int64_t)b * n;
  const int64_t t = lcm_clamp(a.t[b], a.sched_len);
  const float al = a.sched[2 * t], sg = a.sched[2 * t + 1];
  float c_skip, c_out;
  lcm_scalings(t, a.scaling, c_skip, c_out);
  for (int64_t i = (int64_t)blockIdx.x * LCM_THREADS + threadIdx.x; i < groups; i += (int64_t)gridDim.x * LCM_THREADS) {
    const int64_t e0 = i * 8;
    const int cnt = (n - e0) >= 8 ? 8 : (int)(n - e0);
    float xv[8], pv[8], ov[8];
    load8<VEC>(x_, e0, cnt, xv);
    load8<VEC>(p_, e0, cnt, pv);
#pragma unroll
    for (int j = 0; j < 8; j++) ov[j] = c_skip * xv[j] + c_out * lcm_x0<MODE>(xv[j], pv[j], al, sg);
    store8<VEC>(o_, e0, cnt, ov);
  }
}

extern "C" int st355_lcm_target(void* stream, const float* x_prev32, const void* pred_t, const int64_t* timesteps, const float* sched, int sched_len, int mode,
                                float timestep_scaling, float* target, int64_t batch, int64_t per_sample) {
  ST_REQUIRE(x_prev32 && pred_t && timesteps && sched && target, "lcm_target: null pointer");
  ST_REQUIRE((mode == 0 || mode == 1) && sched_len > 0 && per_sample > 0 && batch > 0 && batch < 65536, "lcm_target: bad args (mode %d, sched_len %d, batch %ld)", mode,
             sched_len, (long)batch);
  const bool vec = per_sample % 8 == 0 && (((uintptr_t)x_prev32 | (uintptr_t)pred_t | (uintptr_t)target) & 15) == 0;
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n, 10.0 * n);
  LcmTargetArgs a;
  a.xprev = x_prev32; a.pred = (const bf16*)pred_t; a.t = timesteps; a.sched = sched; a.target = target; a.per_sample = per_sample; a.sched_len = sched_len;
  a.scaling = timestep_scaling;
  const dim3 grid(sample_parts(batch, per_sample), (unsigned)batch), block(LCM_THREADS);
  if (mode == 0) {
    if (vec) hipLaunchKernelGGL((k_lcm_target<0, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_target<0, false>), grid, block, 0, (hipStream_t)stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_lcm_target<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_target<1, false>), grid, block, 0, (hipStream_t)stream, a);
  }
  return st355_check_launch("lcm_target");
}

// ---- the loss and its gradient.  grid = (parts, B) ----
struct LcmLossArgs {
  const bf16 *pred, *x;
  const float* target;
  const int64_t* start;
  const float* sched;
  float* ws;
  bf16* dpred;
  int64_t per_sample;
  int sched_len;
  float scaling, huber_c, dscale /* grad_scale / (per_sample B) */;
};

template <int MODE, int LOSS, bool VEC>
__global__ void __launch_bounds__(LCM_THREADS) k_lcm_loss(const LcmLossArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.per_sample, groups = (n + 7) >> 3;
  const bf16* __restrict__ p_ = a.pred + (int64_t)b * n;
  const bf16* __restrict__ x_ = a.x + (int64_t)b * n;
  const float* __restrict__ t_ = a.target + (int64_t)b * n;
  bf16* __restrict__ d_ = a.dpred ? a.dpred + (int64_t)b * n : nullptr;
  const int64_t ts = lcm_clamp(a.start[b], a.sched_len);
  const float al = a.sched[2 * ts], sg = a.sched[2 * ts + 1];
  float c_skip, c_out;
  lcm_scalings(ts, a.scaling, c_skip, c_out);
  const float dx0 = MODE == 0 ? -(sg / al) : -sg;
  const float gcoef = (a.dscale * c_out) * dx0;
  const float c = a.huber_c, c2 = c * c;
  float acc[1] = {0.f};
  for (int64_t i = (int64_t)blockIdx.x * LCM_THREADS + threadIdx.x; i < groups; i += (int64_t)gridDim.x * LCM_THREADS) {
    const int64_t e0 = i * 8;
    const int cnt = (n - e0) >= 8 ? 8 : (int)(n - e0);
    float pv[8], xv[8], tv[8], gv[8];
    load8<VEC>(p_, e0, cnt, pv);
    load8<VEC>(x_, e0, cnt, xv);
    load8<VEC>(t_, e0, cnt, tv);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float m = c_skip * xv[j] + c_out * lcm_x0<MODE>(xv[j], pv[j], al, sg);
      const float d = m - tv[j];
      float l, g;
      if (LOSS == 0) {
        l = d * d;
        g = 2.f * d;
      } else {
        const float r = sqrtf(d * d + c2);
        l = r - c;
        g = d / r;
      }
      if (VEC || j < cnt) acc[0] += l;
      gv[j] = gcoef * g;
    }
    if (d_) store8<VEC>(d_, e0, cnt, gv);
  }
  block_reduce<1>(acc, a.ws, b);
}

template <int MODE, int LOSS>
static void lcm_loss_launch(bool vec, dim3 grid, dim3 block, hipStream_t s, const LcmLossArgs& a) {
  if (vec) hipLaunchKernelGGL((k_lcm_loss<MODE, LOSS, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_lcm_loss<MODE, LOSS, false>), grid, block, 0, s, a);
}

extern "C" int st355_lcm_loss(void* stream, const void* pred, const void* x_s, const float* target, const int64_t* start, const float* sched, int sched_len, int mode,
                              float timestep_scaling, int loss_type, float huber_c, float* loss_out, float* per_sample_out, void* dpred, void* workspace, int64_t batch,
                              int64_t per_sample, float grad_scale) {
  ST_REQUIRE(pred && x_s && target && start && sched && loss_out && per_sample_out && workspace, "lcm_loss: null pointer");
  ST_REQUIRE((mode == 0 || mode == 1) && (loss_type == 0 || loss_type == 1) && sched_len > 0 && per_sample > 0 && batch > 0 && batch < 65536,
             "lcm_loss: bad args (mode %d, loss_type %d, sched_len %d, batch %ld)", mode, loss_type, sched_len, (long)batch);
  ST_REQUIRE(dpred != pred, "lcm_loss: dpred and pred must be different buffers");
  const bool vec = per_sample % 8 == 0 && (((uintptr_t)pred | (uintptr_t)x_s | (uintptr_t)target | (uintptr_t)dpred) & 15) == 0;
  const int parts = sample_parts(batch, per_sample);
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 14.0 * n, (8.0 + (dpred ? 2.0 : 0.0)) * n);
  LcmLossArgs a;
  a.pred = (const bf16*)pred; a.x = (const bf16*)x_s; a.target = target; a.start = start; a.sched = sched; a.ws = (float*)workspace; a.dpred = (bf16*)dpred;
  a.per_sample = per_sample; a.sched_len = sched_len; a.scaling = timestep_scaling; a.huber_c = huber_c;
  a.dscale = grad_scale / ((float)per_sample * (float)batch);
  const dim3 grid(parts, (unsigned)batch), block(LCM_THREADS);
  if (mode == 0) {
    if (loss_type == 0) lcm_loss_launch<0, 0>(vec, grid, block, (hipStream_t)stream, a);
    else lcm_loss_launch<0, 1>(vec, grid, block, (hipStream_t)stream, a);
  } else {
    if (loss_type == 0) lcm_loss_launch<1, 0>(vec, grid, block, (hipStream_t)stream, a);
    else lcm_loss_launch<1, 1>(vec, grid, block, (hipStream_t)stream, a);
  }
  sample_mean_finish((hipStream_t)stream, (const float*)workspace, nullptr, loss_out, per_sample_out, (int)batch, parts, 1.0f / (float)per_sample);
  return st355_check_launch("lcm_loss");
}

// ---- one LCMScheduler step of the validation sampler: every sample at the same (t, t_next).  grid-stride over all elements ----
struct LcmSampleArgs {
  const bf16 *x, *pred, *noise;
  const float* sched;
  bf16* out;
  int64_t total;
  int64_t t, t_next;
  int sched_len;
  float scaling;
};

template <int MODE, bool VEC>
__global__ void __launch_bounds__(LCM_THREADS) k_lcm_sample(const LcmSampleArgs a) {
  const int64_t n = a.total, groups = (n + 7) >> 3;
  const int64_t t = lcm_clamp(a.t, a.sched_len);
  const float al = a.sched[2 * t], sg = a.sched[2 * t + 1];
  float c_skip, c_out;
  lcm_scalings(t, a.scaling, c_skip, c_out);
  const bool last = a.t_next < 0 || a.noise == nullptr;
  const int64_t tn = lcm_clamp(a.t_next, a.sched_len);
  const float an = a.sched[2 * tn], sn = a.sched[2 * tn + 1];
  for (int64_t i = (int64_t)blockIdx.x * LCM_THREADS + threadIdx.x; i < groups; i += (int64_t)gridDim.x * LCM_THREADS) {
    const int64_t e0 = i * 8;
    const int cnt = (n - e0) >= 8 ? 8 : (int)(n - e0);
    float xv[8], pv[8], nv[8], ov[8];
    load8<VEC>(a.x, e0, cnt, xv);
    load8<VEC>(a.pred, e0, cnt, pv);
    if (!last) load8<VEC>(a.noise, e0, cnt, nv);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float den = c_skip * xv[j] + c_out * lcm_x0<MODE>(xv[j], pv[j], al, sg);
      ov[j] = last ? den : an * den + sn * nv[j];
    }
    store8<VEC>(a.out, e0, cnt, ov);
  }
}

extern "C" int st355_lcm_sample_step(void* stream, const void* x, const void* pred, const void* noise, const float* sched, int sched_len, int mode, float timestep_scaling,
                                     int64_t t, int64_t t_next, void* out, int64_t total) {
  ST_REQUIRE(x && pred && sched && out, "lcm_sample_step: null pointer");
  ST_REQUIRE((mode == 0 || mode == 1) && sched_len > 0 && total > 0, "lcm_sample_step: bad args (mode %d, sched_len %d, total %ld)", mode, sched_len, (long)total);
  ST_REQUIRE(t_next < 0 || noise, "lcm_sample_step: every step but the last (t_next < 0) needs its noise");
  const bool vec = total % 8 == 0 && (((uintptr_t)x | (uintptr_t)pred | (uintptr_t)noise | (uintptr_t)out) & 15) == 0;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 10.0 * (double)total, (t_next < 0 ? 6.0 : 8.0) * (double)total);
  LcmSampleArgs a;
  a.x = (const bf16*)x; a.pred = (const bf16*)pred; a.noise = (const bf16*)noise; a.sched = sched; a.out = (bf16*)out; a.total = total; a.t = t; a.t_next = t_next;
  a.sched_len = sched_len; a.scaling = timestep_scaling;
  const dim3 grid(op_blocks(cdiv64(total, 8))), block(LCM_THREADS);
  if (mode == 0) {
    if (vec) hipLaunchKernelGGL((k_lcm_sample<0, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_sample<0, false>), grid, block, 0, (hipStream_t)stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_lcm_sample<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_lcm_sample<1, false>), grid, block, 0, (hipStream_t)stream, a);
  }
  return st355_check_launch("lcm_sample_step");
}

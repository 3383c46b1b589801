// reflexflow.hip — scheduled sampling with ReflexFlow (flow-matching families): the streaming kernels of the loss and of the rollout.
//
//   st355_reflexflow_stats   one pass over pred / noisy / latents [/ clean / biased]: per sample  S_e = sum |clean - biased|,  sum p^2,  sum tau^2,  sum p tau
//                            (tau = noisy - latents), differences and products in fp32
//   st355_reflexflow_loss    st355_cond_loss_masked + the ReflexFlow terms (common.py:6287-6318, 6426-6429): the exposure weight 1 + alpha e / max(S_e, 1e-6) per
//                            element, beta2, the mask, the per-sample mean, + beta1 * sum (p / max(|p|, 1e-6) - tau / max(|tau|, 1e-6))^2, the batch mean;
//                            d(loss)/d(pred) of all of it in ONE bf16 write
//   st355_flow_euler_step    x[b, :] += dt[b] * v[b, :] in place (the rollout's update, rollout.py:163-164), fp32 arithmetic, one rounding
//
// All three stream 16 bytes per lane.  Both reductions run in two stages in a fixed order — stage 1: `parts` workgroups per sample, each lane a strided run of
// vectors, lane tree, then the wave partials in wave order; stage 2, on the device: the `parts` partials in index order — so every output repeats bit for bit, and
// nothing is read on the host.  No atomics.
#include "feature_common.h"

#define RF_THREADS OP_THREADS
#define RF_EPS 1e-6f

extern "C" int64_t st355_reflexflow_workspace(int64_t batch, int64_t per_sample) {
  if (batch <= 0 || per_sample <= 0) return 0;
  return (int64_t)sizeof(float) * 4 * batch * sample_parts(batch, per_sample);
}

// ---- stats ----------------------------------------------------------------------------------------------------------------------------------------
// grid = (parts, B)
template <bool HAS_E>
__global__ void __launch_bounds__(RF_THREADS) k_rf_stats(const bf16* __restrict__ pred, const bf16* __restrict__ noisy, const bf16* __restrict__ latents,
                                                        const bf16* __restrict__ clean, const bf16* __restrict__ biased, float* __restrict__ ws,
                                                        int64_t per_sample) {
  const int b = blockIdx.y;
  const int64_t base = (int64_t)b * per_sample, vecs = per_sample >> 3;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; i < vecs; i += (int64_t)gridDim.x * RF_THREADS) {
    const bf16x8 pv = *(const bf16x8*)(pred + base + i * 8);
    const bf16x8 nv = *(const bf16x8*)(noisy + base + i * 8);
    const bf16x8 lv = *(const bf16x8*)(latents + base + i * 8);
    bf16x8 cv, bv;
    if (HAS_E) {
      cv = *(const bf16x8*)(clean + base + i * 8);
      bv = *(const bf16x8*)(biased + base + i * 8);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = bf2f(pv[j]), tau = bf2f(nv[j]) - bf2f(lv[j]);
      if (HAS_E) acc[0] += fabsf(bf2f(cv[j]) - bf2f(bv[j]));
      acc[1] += p * p;
      acc[2] += tau * tau;
      acc[3] += p * tau;
    }
  }
  block_reduce<4>(acc, ws, b);
}

// stage 2: stats[b, k] = the partials of (b, k) in index order.  grid = B, 64 threads (4 used)
__global__ void k_rf_stats_finish(const float* __restrict__ ws, float* __restrict__ stats, int parts) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= 4) return;
  float s = 0.f;
  for (int p = 0; p < parts; p++) s += ws[((int64_t)b * parts + p) * 4 + k];
  stats[(int64_t)b * 4 + k] = s;
}

extern "C" int st355_reflexflow_stats(void* stream, const void* pred, const void* noisy, const void* latents, const void* clean, const void* biased,
                                      float* stats_out, void* workspace, int64_t batch, int64_t per_sample) {
  ST_REQUIRE(pred && noisy && latents && stats_out && workspace, "reflexflow_stats: null pointer");
  ST_REQUIRE((clean == nullptr) == (biased == nullptr), "reflexflow_stats: clean and biased come together or not at all");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && batch > 0 && batch < 65536, "reflexflow_stats: bad shape (per_sample %ld must be a multiple of 8, batch %ld < 65536)",
             (long)per_sample, (long)batch);
  const int parts = sample_parts(batch, per_sample);
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n, (clean ? 10.0 : 6.0) * n);
  float* ws = (float*)workspace;
  if (clean)
    hipLaunchKernelGGL(k_rf_stats<true>, dim3(parts, (unsigned)batch), dim3(RF_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)noisy,
                       (const bf16*)latents, (const bf16*)clean, (const bf16*)biased, ws, per_sample);
  else
    hipLaunchKernelGGL(k_rf_stats<false>, dim3(parts, (unsigned)batch), dim3(RF_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)noisy,
                       (const bf16*)latents, (const bf16*)nullptr, (const bf16*)nullptr, ws, per_sample);
  hipLaunchKernelGGL(k_rf_stats_finish, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, ws, stats_out, parts);
  return st355_check_launch("reflexflow_stats");
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------------------------
//   l2: d^2 | huber: 2c (sqrt(d^2 + c^2) - c) | smooth_l1: 2 (sqrt(d^2 + c^2) - c)      (k_mse / k_cond_loss of elementwise.hip)
//   ADR (beta1 != 0), per sample: u = p / pn, th = tau / tn, pn = max(|p|, 1e-6), tn = max(|tau|, 1e-6):  adr = sum (u - th)^2
//     d adr / d p = (2 / pn) [(u - th) - u (u . (u - th))]   for |p| > 1e-6   (u is then a unit vector: the projector I - u u^T of d u / d p)
//                 = (2 / 1e-6) (u - th)                       for a clamped norm (pn is then a constant)
//     u . (u - th) = sum p^2 / pn^2 - sum p tau / (pn tn), from the stats
struct RfLossArgs {
  const bf16 *pred, *target, *noisy, *latents, *clean, *biased;
  const float *huber_c, *emask, *stats;
  float* ws;
  bf16* dpred;
  int64_t per_sample, mask_period;
  float alpha, beta1, beta2, dscale /* grad_scale / (per_sample B) */, ascale /* grad_scale 2 beta1 / B */;
};

template <int TYPE>
__global__ void __launch_bounds__(RF_THREADS) k_rf_loss(const RfLossArgs a) {
  const int b = blockIdx.y;
  const int64_t base = (int64_t)b * a.per_sample, vecs = a.per_sample >> 3;
  const bool has_e = a.clean != nullptr && a.alpha != 0.f, has_adr = a.beta1 != 0.f;
  const bool want_grad = a.dpred != nullptr;
  const float* em = a.emask ? a.emask + (int64_t)b * a.mask_period : nullptr;
  const float c = TYPE ? a.huber_c[b] : 0.f, c2 = c * c;
  const float k = (TYPE == 1) ? 2.f * c : 2.f;
  float e_scale = 0.f, inv_pn = 0.f, inv_tn = 0.f, udot = 0.f, gcoef = 0.f;
  if (has_e) e_scale = a.alpha / fmaxf(a.stats[b * 4 + 0], RF_EPS);
  if (has_adr) {
    const float pp = a.stats[b * 4 + 1], tt = a.stats[b * 4 + 2], pt = a.stats[b * 4 + 3];
    const float pnorm = sqrtf(pp), tnorm = sqrtf(tt);
    const float pn = fmaxf(pnorm, RF_EPS), tn = fmaxf(tnorm, RF_EPS);
    inv_pn = 1.f / pn;
    inv_tn = 1.f / tn;
    udot = (pnorm > RF_EPS) ? pp * inv_pn * inv_pn - pt * inv_pn * inv_tn : 0.f;
    gcoef = a.ascale * inv_pn;
  }
  float acc[2] = {0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; i < vecs; i += (int64_t)gridDim.x * RF_THREADS) {
    const bf16x8 pv = *(const bf16x8*)(a.pred + base + i * 8);
    const bf16x8 tv = *(const bf16x8*)(a.target + base + i * 8);
    bf16x8 nv, lv, cv, bv, dv;
    if (has_adr) {
      nv = *(const bf16x8*)(a.noisy + base + i * 8);
      lv = *(const bf16x8*)(a.latents + base + i * 8);
    }
    if (has_e) {
      cv = *(const bf16x8*)(a.clean + base + i * 8);
      bv = *(const bf16x8*)(a.biased + base + i * 8);
    }
    float mk[8];
    if (em) {
      const int64_t off = (i * 8) % a.mask_period;
      const f32x4 m0 = *(const f32x4*)(em + off), m1 = *(const f32x4*)(em + off + 4);
#pragma unroll
      for (int j = 0; j < 4; j++) { mk[j] = m0[j]; mk[j + 4] = m1[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) mk[j] = 1.f;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = bf2f(pv[j]);
      const float d = p - bf2f(tv[j]);
      float l, g;
      if (TYPE == 0) {
        l = d * d;
        g = 2.f * d;
      } else {
        const float r = sqrtf(d * d + c2);
        l = k * (r - c);
        g = k * d / r;
      }
      float w = a.beta2 * mk[j];
      if (has_e) w *= 1.f + e_scale * (bf2f(cv[j]) - bf2f(bv[j]));
      acc[0] += l * w;
      float grad = want_grad ? a.dscale * g * w : 0.f;          // (no dpred: the gradient is neither formed, converted nor written)
      if (has_adr) {
        const float u = p * inv_pn;
        const float q = u - (bf2f(nv[j]) - bf2f(lv[j])) * inv_tn;
        acc[1] += q * q;
        if (want_grad) grad += gcoef * (q - u * udot);
      }
      if (want_grad) dv[j] = f2bf(grad);
    }
    if (want_grad) *(bf16x8*)(a.dpred + base + i * 8) = dv;
  }
  block_reduce<2, 4>(acc, a.ws, b);
}

// stage 2, one workgroup: per sample the partials in index order -> per_sample[b] = sum / n + beta1 adr, adr_out[b] = beta1 adr; then the batch mean in sample order
__global__ void __launch_bounds__(RF_THREADS) k_rf_loss_finish(const float* __restrict__ ws, float* __restrict__ loss, float* __restrict__ per_sample_out,
                                                              float* __restrict__ adr_out, int B, int parts, float inv_per_sample, float beta1) {
  for (int b = threadIdx.x; b < B; b += RF_THREADS) {
    float s = 0.f, q = 0.f;
    for (int p = 0; p < parts; p++) {
      s += ws[((int64_t)b * parts + p) * 4 + 0];
      q += ws[((int64_t)b * parts + p) * 4 + 1];
    }
    const float term = beta1 != 0.f ? beta1 * q : 0.f;
    per_sample_out[b] = s * inv_per_sample + term;
    if (adr_out) adr_out[b] = term;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; b++) s += per_sample_out[b];
    loss[0] = s / (float)B;
  }
}

extern "C" int st355_reflexflow_loss(void* stream, const void* pred, const void* target, const float* huber_c, int loss_type, const float* emask,
                                     int64_t mask_period, const void* noisy, const void* latents, const void* clean, const void* biased, const float* stats,
                                     float alpha, float beta1, float beta2, float* loss_out, float* per_sample_out, float* adr_out, void* dpred,
                                     void* workspace, int64_t batch, int64_t per_sample, float grad_scale) {
  ST_REQUIRE(pred && target && loss_out && per_sample_out && workspace, "reflexflow_loss: null pointer");
  ST_REQUIRE(loss_type >= 0 && loss_type <= 2 && per_sample > 0 && per_sample % 8 == 0 && batch > 0 && batch < 65536, "reflexflow_loss: bad args");
  ST_REQUIRE(loss_type == 0 || huber_c, "reflexflow_loss: huber / smooth_l1 need huber_c [B]");
  ST_REQUIRE(!emask || (mask_period > 0 && mask_period % 8 == 0 && per_sample % mask_period == 0 && ((uintptr_t)emask & 15) == 0),
             "reflexflow_loss: element mask period must be a multiple of 8 dividing per_sample (16-byte aligned)");
  ST_REQUIRE((clean == nullptr) == (biased == nullptr), "reflexflow_loss: clean and biased come together or not at all");
  ST_REQUIRE(beta1 == 0.f || (noisy && latents), "reflexflow_loss: the ADR term (beta1 != 0) needs noisy and latents");
  ST_REQUIRE(stats || (beta1 == 0.f && !(clean && alpha != 0.f)), "reflexflow_loss: the exposure weight and the ADR term need the stats of st355_reflexflow_stats");
  const int parts = sample_parts(batch, per_sample);
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 20.0 * n, (4.0 + (beta1 != 0.f ? 4.0 : 0.0) + (clean && alpha != 0.f ? 4.0 : 0.0) + (dpred ? 2.0 : 0.0)) * n);
  RfLossArgs a;
  a.pred = (const bf16*)pred; a.target = (const bf16*)target; a.noisy = (const bf16*)noisy; a.latents = (const bf16*)latents;
  a.clean = (const bf16*)clean; a.biased = (const bf16*)biased; a.huber_c = huber_c; a.emask = emask; a.stats = stats; a.ws = (float*)workspace;
  a.dpred = (bf16*)dpred; a.per_sample = per_sample; a.mask_period = mask_period; a.alpha = alpha; a.beta1 = beta1; a.beta2 = beta2;
  a.dscale = grad_scale / ((float)per_sample * (float)batch);
  a.ascale = grad_scale * 2.f * beta1 / (float)batch;
  const dim3 grid(parts, (unsigned)batch);
  if (loss_type == 0) hipLaunchKernelGGL(k_rf_loss<0>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, a);
  else if (loss_type == 1) hipLaunchKernelGGL(k_rf_loss<1>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_rf_loss<2>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_rf_loss_finish, dim3(1), dim3(RF_THREADS), 0, (hipStream_t)stream, (const float*)workspace, loss_out, per_sample_out, adr_out, (int)batch,
                     parts, 1.0f / (float)per_sample, beta1);
  return st355_check_launch("reflexflow_loss");
}

// ---- Euler step -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RF_THREADS) k_flow_euler_step(bf16* __restrict__ x, const bf16* __restrict__ v, const float* __restrict__ dt, int64_t batch,
                                                               int64_t per_sample) {
  const int64_t nvec = (batch * per_sample) >> 3, vec_per_sample = per_sample >> 3;
  for (int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * RF_THREADS) {
    const float h = dt[i / vec_per_sample];
    bf16x8 xv = *(const bf16x8*)(x + i * 8);
    const bf16x8 vv = *(const bf16x8*)(v + i * 8);
#pragma unroll
    for (int j = 0; j < 8; j++) xv[j] = f2bf(bf2f(xv[j]) + h * bf2f(vv[j]));
    *(bf16x8*)(x + i * 8) = xv;
  }
}

extern "C" int st355_flow_euler_step(void* stream, void* x, const void* v, const float* dt, int64_t batch, int64_t per_sample) {
  ST_REQUIRE(x && v && dt, "flow_euler_step: null pointer");
  ST_REQUIRE(x != v, "flow_euler_step: x and v must be different buffers");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && batch > 0, "flow_euler_step: per_sample (%ld) must be a multiple of 8", (long)per_sample);
  const int64_t n = batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * n, 6.0 * n);
  hipLaunchKernelGGL(k_flow_euler_step, dim3(op_blocks(n / 8)), dim3(RF_THREADS), 0, (hipStream_t)stream, (bf16*)x, (const bf16*)v, dt, batch, per_sample);
  return st355_check_launch("flow_euler_step");
}

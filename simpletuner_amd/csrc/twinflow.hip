// twinflow.hip — TwinFlow (RCGM) few-step training and its UCGM sampler (flow-matching families): the streaming kernels.
//
//   st355_twinflow_rcgm_step   one step of the RCGM target's teacher integration (common.py `_twinflow_rcgm_target`): with h = t_next[b] - t_prev[b]
//                              x[b, :] <- x + h F_c (bf16 in place, fp32 arithmetic, one rounding) and acc[b, :] (+)= (-h) F_c (fp32), one pass over F_c
//   st355_twinflow_loss        t' = target + ratio (cond - uncond), r = pred - acc - t':  loss_out = { mean clamp(r, +-c)^2, mean (pred - t')^2 } over the whole
//                              tensor, and d(base + realvel)/d(pred) = grad_scale (2 / N) (clamp(r) + (pred - t')) in ONE bf16 write
//   st355_twinflow_ucgm_step   the sampler's step (custom_schedule.py `TwinFlowScheduler.step`), in place:
//                              x <- (1 - s_next) (x - s_cur v) + s_next ((x + (1 - s_cur) v) sqrt(1 - rho) + noise sqrt(rho))
//
// All three stream 16 bytes per lane.  The loss's reduction runs in two stages in a fixed order — stage 1: `parts` workgroups per sample, each lane a strided run
// of vectors, lane tree, then the wave partials in wave order; stage 2, one workgroup: contiguous runs of the partials in (sample, part) order, then the run
// sums in thread order — so every output repeats bit for bit, and nothing is read on the host.  No atomics.
#include "feature_common.h"

#define TF_THREADS OP_THREADS

extern "C" int64_t st355_twinflow_workspace(int64_t batch, int64_t per_sample) {
  if (batch <= 0 || per_sample <= 0) return 0;
  return (int64_t)sizeof(float) * 2 * batch * sample_parts(batch, per_sample);
}

// ---- RCGM step ------------------------------------------------------------------------------------------------------------------------------------
template <bool FIRST>
__global__ void __launch_bounds__(TF_THREADS) k_tf_rcgm_step(bf16* __restrict__ x, float* __restrict__ acc, const bf16* __restrict__ fc,
                                                            const float* __restrict__ t_prev, const float* __restrict__ t_next, int64_t batch,
                                                            int64_t per_sample) {
  const int64_t nvec = (batch * per_sample) >> 3, vec_per_sample = per_sample >> 3;
  for (int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * TF_THREADS) {
    const int64_t b = i / vec_per_sample;
    const float h = t_next[b] - t_prev[b], hn = -h;          // (t_prev - t_next == -(t_next - t_prev) exactly)
    bf16x8 xv = *(const bf16x8*)(x + i * 8);
    const bf16x8 fv = *(const bf16x8*)(fc + i * 8);
    f32x4 a0, a1;
    if (FIRST) {
      a0 = f32x4{0.f, 0.f, 0.f, 0.f};
      a1 = a0;
    } else {
      a0 = *(const f32x4*)(acc + i * 8);
      a1 = *(const f32x4*)(acc + i * 8 + 4);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float f = bf2f(fv[j]);
      xv[j] = f2bf(bf2f(xv[j]) + h * f);
      if (j < 4) a0[j] += hn * f;
      else a1[j - 4] += hn * f;
    }
    *(bf16x8*)(x + i * 8) = xv;
    *(f32x4*)(acc + i * 8) = a0;
    *(f32x4*)(acc + i * 8 + 4) = a1;
  }
}

extern "C" int st355_twinflow_rcgm_step(void* stream, void* x, float* acc, const void* fc, const float* t_prev, const float* t_next, int first, int64_t batch,
                                        int64_t per_sample) {
  ST_REQUIRE(x && acc && fc && t_prev && t_next, "twinflow_rcgm_step: null pointer");
  ST_REQUIRE(x != fc, "twinflow_rcgm_step: x and fc must be different buffers");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && batch > 0, "twinflow_rcgm_step: per_sample (%ld) must be a multiple of 8, batch (%ld) positive",
             (long)per_sample, (long)batch);
  ST_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)fc & 15) == 0 && ((uintptr_t)acc & 15) == 0, "twinflow_rcgm_step: x, fc and acc must be 16-byte aligned");
  const int64_t n = batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 4.0 * n, (first ? 10.0 : 14.0) * n);
  if (first)
    hipLaunchKernelGGL(k_tf_rcgm_step<true>, dim3(op_blocks(n / 8)), dim3(TF_THREADS), 0, (hipStream_t)stream, (bf16*)x, acc, (const bf16*)fc, t_prev, t_next,
                       batch, per_sample);
  else
    hipLaunchKernelGGL(k_tf_rcgm_step<false>, dim3(op_blocks(n / 8)), dim3(TF_THREADS), 0, (hipStream_t)stream, (bf16*)x, acc, (const bf16*)fc, t_prev, t_next,
                       batch, per_sample);
  return st355_check_launch("twinflow_rcgm_step");
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------------------------
// grid = (parts, B); ws[(b * parts + part) * 2 + k]
template <bool HAS_CFG>
__global__ void __launch_bounds__(TF_THREADS) k_tf_loss(const bf16* __restrict__ pred, const bf16* __restrict__ target, const float* __restrict__ accum,
                                                       const bf16* __restrict__ cond, const bf16* __restrict__ uncond, float* __restrict__ ws,
                                                       bf16* __restrict__ dpred, int64_t per_sample, float ratio, float clampv, float gscale) {
  const int b = blockIdx.y;
  const int64_t base = (int64_t)b * per_sample, vecs = per_sample >> 3;
  const bool want_grad = dpred != nullptr;
  float acc[2] = {0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x; i < vecs; i += (int64_t)gridDim.x * TF_THREADS) {
    const bf16x8 pv = *(const bf16x8*)(pred + base + i * 8);
    const bf16x8 tv = *(const bf16x8*)(target + base + i * 8);
    const f32x4 a0 = *(const f32x4*)(accum + base + i * 8), a1 = *(const f32x4*)(accum + base + i * 8 + 4);
    bf16x8 cv, uv, dv;
    if (HAS_CFG) {
      cv = *(const bf16x8*)(cond + base + i * 8);
      uv = *(const bf16x8*)(uncond + base + i * 8);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = bf2f(pv[j]);
      float t = bf2f(tv[j]);
      if (HAS_CFG) t += ratio * (bf2f(cv[j]) - bf2f(uv[j]));
      const float d = p - t;
      const float r = d - (j < 4 ? a0[j] : a1[j - 4]);
      const float rc = fminf(fmaxf(r, -clampv), clampv);
      acc[0] += rc * rc;
      acc[1] += d * d;
      if (want_grad) dv[j] = f2bf(gscale * (rc + d));
    }
    if (want_grad) *(bf16x8*)(dpred + base + i * 8) = dv;
  }
  block_reduce<2>(acc, ws, b);
}

// stage 2, one workgroup: thread t sums its contiguous run of the B * parts partials in index order, then thread k < 2 sums the 256 run sums of k in thread order
// (a fixed order: every launch gives the same bits); loss_out[k] = sum / N
__global__ void __launch_bounds__(TF_THREADS) k_tf_loss_finish(const float* __restrict__ ws, float* __restrict__ loss_out, int64_t count, float inv_n) {
  __shared__ float red[2][TF_THREADS];
  const int64_t chunk = (count + TF_THREADS - 1) / TF_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * chunk;
  const int64_t hi = lo + chunk < count ? lo + chunk : count;
  float s0 = 0.f, s1 = 0.f;
  for (int64_t p = lo; p < hi; p++) {
    s0 += ws[p * 2];
    s1 += ws[p * 2 + 1];
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
    for (int t = 0; t < TF_THREADS; t++) s += red[threadIdx.x][t];
    loss_out[threadIdx.x] = s * inv_n;
  }
}

extern "C" int st355_twinflow_loss(void* stream, const void* pred, const void* target, const float* acc, const void* cond, const void* uncond, float ratio,
                                   float clamp, float* loss_out, void* dpred, void* workspace, int64_t batch, int64_t per_sample, float grad_scale) {
  ST_REQUIRE(pred && target && acc && loss_out && workspace, "twinflow_loss: null pointer");
  ST_REQUIRE((cond == nullptr) == (uncond == nullptr), "twinflow_loss: cond and uncond come together or not at all");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && batch > 0 && batch < 65536, "twinflow_loss: bad shape (per_sample %ld must be a multiple of 8, batch %ld < 65536)",
             (long)per_sample, (long)batch);
  ST_REQUIRE(clamp >= 0.f, "twinflow_loss: the clamp (%g) must not be negative", (double)clamp);
  ST_REQUIRE(((uintptr_t)acc & 15) == 0, "twinflow_loss: acc must be 16-byte aligned");
  const int parts = sample_parts(batch, per_sample);
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 10.0 * n, (8.0 + (cond ? 4.0 : 0.0) + (dpred ? 2.0 : 0.0)) * n);
  const float gscale = (float)((double)grad_scale * 2.0 / n);
  const dim3 grid(parts, (unsigned)batch);
  if (cond)
    hipLaunchKernelGGL(k_tf_loss<true>, grid, dim3(TF_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)target, acc, (const bf16*)cond,
                       (const bf16*)uncond, (float*)workspace, (bf16*)dpred, per_sample, ratio, clamp, gscale);
  else
    hipLaunchKernelGGL(k_tf_loss<false>, grid, dim3(TF_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)target, acc, (const bf16*)nullptr,
                       (const bf16*)nullptr, (float*)workspace, (bf16*)dpred, per_sample, ratio, clamp, gscale);
  hipLaunchKernelGGL(k_tf_loss_finish, dim3(1), dim3(TF_THREADS), 0, (hipStream_t)stream, (const float*)workspace, loss_out, (int64_t)batch * parts, (float)(1.0 / n));
  return st355_check_launch("twinflow_loss");
}

// ---- UCGM step ------------------------------------------------------------------------------------------------------------------------------------
template <bool HAS_NOISE>
__global__ void __launch_bounds__(TF_THREADS) k_tf_ucgm_step(bf16* __restrict__ x, const bf16* __restrict__ v, const bf16* __restrict__ noise, int64_t nvec,
                                                            float s_cur, float s_next, float q_keep, float q_noise) {
  const float g_next = 1.f - s_next, g_cur = 1.f - s_cur;
  for (int64_t i = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * TF_THREADS) {
    bf16x8 xv = *(const bf16x8*)(x + i * 8);
    const bf16x8 vv = *(const bf16x8*)(v + i * 8);
    bf16x8 nv;
    if (HAS_NOISE) nv = *(const bf16x8*)(noise + i * 8);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xs = bf2f(xv[j]), f = bf2f(vv[j]);
      const float x_hat = xs - s_cur * f, z_hat = xs + g_cur * f;
      float z = z_hat * q_keep;
      if (HAS_NOISE) z += bf2f(nv[j]) * q_noise;
      xv[j] = f2bf(g_next * x_hat + s_next * z);
    }
    *(bf16x8*)(x + i * 8) = xv;
  }
}

extern "C" int st355_twinflow_ucgm_step(void* stream, void* x, const void* v, const void* noise, float s_cur, float s_next, float rho, int64_t n) {
  ST_REQUIRE(x && v, "twinflow_ucgm_step: null pointer");
  ST_REQUIRE(x != v && x != noise, "twinflow_ucgm_step: x, v and noise must be different buffers");
  ST_REQUIRE(n > 0 && n % 8 == 0, "twinflow_ucgm_step: the element count (%ld) must be a positive multiple of 8", (long)n);
  ST_REQUIRE(rho >= 0.f && rho <= 1.f, "twinflow_ucgm_step: rho (%g) must lie in [0, 1]", (double)rho);
  ST_REQUIRE(noise || rho == 0.f, "twinflow_ucgm_step: rho > 0 needs noise");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 8.0 * n, (noise && rho != 0.f ? 8.0 : 6.0) * n);
  const float q_keep = sqrtf(1.f - rho), q_noise = sqrtf(rho);
  if (noise && rho != 0.f)
    hipLaunchKernelGGL(k_tf_ucgm_step<true>, dim3(op_blocks(n / 8)), dim3(TF_THREADS), 0, (hipStream_t)stream, (bf16*)x, (const bf16*)v, (const bf16*)noise, n >> 3,
                       s_cur, s_next, q_keep, q_noise);
  else
    hipLaunchKernelGGL(k_tf_ucgm_step<false>, dim3(op_blocks(n / 8)), dim3(TF_THREADS), 0, (hipStream_t)stream, (bf16*)x, (const bf16*)v, (const bf16*)nullptr,
                       n >> 3, s_cur, s_next, q_keep, q_noise);
  return st355_check_launch("twinflow_ucgm_step");
}

// eval_loss.hip — the evaluation loss (eval_steps_interval / eval_epoch_interval; validation.py `Evaluation`, trainer.py `_prepare_custom_timestep_batch`,
// flow-matching families): the two streaming kernels of a pass that stacks K timesteps of the same B samples along the batch axis.
//
//   st355_eval_flow_views   out[k, b, :] = (1 - sigma[k]) x[b, :] + sigma[k] noise[b, :] for every k < K: x and noise are read ONCE, the K loop runs on the
//                           lane's registers.  The expression, its fp32 arithmetic and its single bf16 rounding are st355_flow_noise_mix's: slab k is bit-identical
//                           to that op called with sigma[k] for every row
//   st355_eval_loss         for every slab k of pred [K, B, n] against the ONE target [B, n]: the l2 / huber / smooth_l1 element loss (st355_cond_loss's formulas),
//                           the per-sample mean -> per_sample[k, b], the batch mean -> loss[k].  No gradient, no mask, no weights
//
// Both stream 16 bytes per lane.  The loss's reduction runs in two stages in a fixed order — stage 1: grid (parts, B, K), each workgroup one strided run of sample
// (k, b): lane tree, then the wave partials in wave order; stage 2, one workgroup per k: thread b sums sample b's partials in part order, thread 0 the B sample means
// in sample order.  `parts` follows from B and n alone and no workgroup sees another slab, so loss[k] and per_sample[k, :] have the same bits whatever K is and
// wherever the slab sits in the chunk.  No atomics, nothing read on the host.
#include "feature_common.h"

#define EL_THREADS OP_THREADS
#define EL_MAX_K 64

// (sample_parts over the B samples of ONE slab)
extern "C" int64_t st355_eval_loss_workspace(int64_t batch, int64_t per_sample, int64_t k) {
  if (batch <= 0 || per_sample <= 0 || k <= 0) return 0;
  return (int64_t)sizeof(float) * k * batch * sample_parts(batch, per_sample);
}

// ---- views ----------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EL_THREADS) k_eval_flow_views(const bf16* __restrict__ x, const bf16* __restrict__ noise, const float* __restrict__ sigma,
                                                               bf16* __restrict__ out, int64_t nvec, int K) {
  for (int64_t i = (int64_t)blockIdx.x * EL_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * EL_THREADS) {
    const bf16x8 xv = *(const bf16x8*)(x + i * 8);
    const bf16x8 nv = *(const bf16x8*)(noise + i * 8);
    float xf[8], n[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      xf[j] = bf2f(xv[j]);
      n[j] = bf2f(nv[j]);
    }
    for (int k = 0; k < K; k++) {
      const float s = sigma[k];
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf((1.0f - s) * xf[j] + s * n[j]);          // st355_flow_noise_mix's expression, one rounding
      *(bf16x8*)(out + ((int64_t)k * nvec + i) * 8) = o;
    }
  }
}

static inline bool el_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

extern "C" int st355_eval_flow_views(void* stream, const void* latents, const void* noise, const float* sigma, void* out, int64_t batch, int64_t per_sample,
                                     int64_t k) {
  ST_REQUIRE(latents && noise && sigma && out, "eval_flow_views: null pointer");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && batch > 0, "eval_flow_views: per_sample (%ld) must be a positive multiple of 8, batch (%ld) positive",
             (long)per_sample, (long)batch);
  ST_REQUIRE(k >= 1 && k <= EL_MAX_K, "eval_flow_views: the timestep count (%ld) must lie in [1, %d]", (long)k, EL_MAX_K);
  ST_REQUIRE(((uintptr_t)latents & 15) == 0 && ((uintptr_t)noise & 15) == 0 && ((uintptr_t)out & 15) == 0, "eval_flow_views: latents, noise and out must be 16-byte aligned");
  const int64_t n = batch * per_sample;
  ST_REQUIRE(!el_overlap(out, 2 * k * n, latents, 2 * n) && !el_overlap(out, 2 * k * n, noise, 2 * n), "eval_flow_views: out must not overlap latents or noise");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 4.0 * k * n, (4.0 + 2.0 * k) * n);
  hipLaunchKernelGGL(k_eval_flow_views, dim3(op_blocks(n / 8)), dim3(EL_THREADS), 0, (hipStream_t)stream, (const bf16*)latents, (const bf16*)noise, sigma, (bf16*)out,
                     n >> 3, (int)k);
  return st355_check_launch("eval_flow_views");
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------------------------
// grid = (parts, B, K); ws[(k * B + b) * parts + part].  TYPE 0: d^2;  1: 2c (sqrt(d^2 + c^2) - c);  2: 2 (sqrt(d^2 + c^2) - c)   (common.py:6132-6166)
template <int TYPE>
__global__ void __launch_bounds__(EL_THREADS) k_eval_loss(const bf16* __restrict__ pred, const bf16* __restrict__ target, const float* __restrict__ huber_c,
                                                         float* __restrict__ ws, int64_t per_sample) {
  const int b = blockIdx.y, k = blockIdx.z, B = gridDim.y;
  const int64_t vecs = per_sample >> 3;
  const bf16* p = pred + ((int64_t)k * B + b) * per_sample;
  const bf16* t = target + (int64_t)b * per_sample;
  float c = 0.f, c2 = 0.f, scale = 2.f;
  if (TYPE != 0) {
    c = huber_c[(int64_t)k * B + b];
    c2 = c * c;
    if (TYPE == 1) scale = 2.f * c;
  }
  float acc[1] = {0.f};
  for (int64_t i = (int64_t)blockIdx.x * EL_THREADS + threadIdx.x; i < vecs; i += (int64_t)gridDim.x * EL_THREADS) {
    const bf16x8 pv = *(const bf16x8*)(p + i * 8);
    const bf16x8 tv = *(const bf16x8*)(t + i * 8);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float df = bf2f(pv[j]) - bf2f(tv[j]);
      if (TYPE == 0) acc[0] += df * df;
      else acc[0] += scale * (sqrtf(df * df + c2) - c);
    }
  }
  block_reduce<1>(acc, ws, (int64_t)k * B + b);
}

// stage 2, grid = (K): thread b (strided over the samples) sums sample (k, b)'s partials in part order and writes per_sample[k, b] = sum / n; then thread 0 sums the B
// sample means in sample order: loss[k] = sum / B
__global__ void __launch_bounds__(EL_THREADS) k_eval_loss_finish(const float* __restrict__ ws, float* __restrict__ per_sample_out, float* __restrict__ loss_out, int B,
                                                                int parts, float inv_n) {
  const int k = blockIdx.x;
  for (int b = threadIdx.x; b < B; b += EL_THREADS) {
    const float* w = ws + ((int64_t)k * B + b) * parts;
    float s = 0.f;
    for (int p = 0; p < parts; p++) s += w[p];
    per_sample_out[(int64_t)k * B + b] = s * inv_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; b++) s += per_sample_out[(int64_t)k * B + b];
    loss_out[k] = s / (float)B;
  }
}

extern "C" int st355_eval_loss(void* stream, const void* pred, const void* target, int loss_type, const float* huber_c, float* per_sample, float* loss,
                               void* workspace, int64_t batch, int64_t per_sample_n, int64_t k) {
  ST_REQUIRE(pred && target && per_sample && loss && workspace, "eval_loss: null pointer");
  ST_REQUIRE(loss_type >= 0 && loss_type <= 2, "eval_loss: loss_type (%d) must be 0 (l2), 1 (huber) or 2 (smooth_l1)", loss_type);
  ST_REQUIRE(loss_type == 0 || huber_c, "eval_loss: huber / smooth_l1 need huber_c [K * B]");
  ST_REQUIRE(per_sample_n > 0 && per_sample_n % 8 == 0 && batch > 0 && batch < 65536, "eval_loss: bad shape (per_sample %ld must be a multiple of 8, batch %ld < 65536)",
             (long)per_sample_n, (long)batch);
  ST_REQUIRE(k >= 1 && k <= EL_MAX_K, "eval_loss: the timestep count (%ld) must lie in [1, %d]", (long)k, EL_MAX_K);
  ST_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)target & 15) == 0 && ((uintptr_t)workspace & 3) == 0, "eval_loss: pred and target must be 16-byte aligned");
  const int parts = sample_parts(batch, per_sample_n);
  const double n = (double)batch * per_sample_n;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, (loss_type ? 6.0 : 3.0) * k * n, 2.0 * (k + 1) * n);
  const dim3 grid(parts, (unsigned)batch, (unsigned)k);
  if (loss_type == 0)
    hipLaunchKernelGGL(k_eval_loss<0>, grid, dim3(EL_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)target, huber_c, (float*)workspace, per_sample_n);
  else if (loss_type == 1)
    hipLaunchKernelGGL(k_eval_loss<1>, grid, dim3(EL_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)target, huber_c, (float*)workspace, per_sample_n);
  else
    hipLaunchKernelGGL(k_eval_loss<2>, grid, dim3(EL_THREADS), 0, (hipStream_t)stream, (const bf16*)pred, (const bf16*)target, huber_c, (float*)workspace, per_sample_n);
  hipLaunchKernelGGL(k_eval_loss_finish, dim3((unsigned)k), dim3(EL_THREADS), 0, (hipStream_t)stream, (const float*)workspace, per_sample, loss, (int)batch, parts,
                     (float)(1.0 / (double)per_sample_n));
  return st355_check_launch("eval_loss");
}

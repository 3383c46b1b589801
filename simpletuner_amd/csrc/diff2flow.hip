// diff2flow.hip — the Diff2Flow flow-matching loss of the epsilon / v families (diff2flow/bridge.py, common.py:6231-6248 + 6402-6429): one streaming pass.
//
//   st355_diff2flow_loss   per sample b, (c0, c1) = table[clamp(timesteps[b], 0, T - 1)]:
//                            mode 0 (epsilon): (c0, c1) = (sqrt(1/a), sqrt(1/a - 1));  z = c0 x - c1 p,  f = p - z                      k = 1 + c1
//                            mode 1 (v):       (c0, c1) = (sqrt(a), sqrt(1 - a));      z = c0 x - c1 p,  e = c0 p + c1 x,  f = e - z    k = c0 + c1
//                          d = f - tau;  loss element d^2 * mask;  per-sample mean (* weight[b]);  batch mean;  d(loss)/d(pred) = 2 k d mask weight / (B n) in ONE bf16 write
//
// The coefficient pair is gathered in the kernel from the device timestep (nothing is read on the host: a captured step replays it), the index clamped before
// the gather.  16 bytes per lane; the prediction is read in place through its per-sample stride (PixArt's first channel half).  Where the per-sample size, the
// stride or the mask period is no multiple of 8 (or a pointer is not 16-byte aligned) the same walk runs with scalar loads and stores, the n % 8 tail included.
// The reduction runs in two stages in a fixed order — stage 1: `parts` workgroups per sample, each lane a strided run of 8-element groups, lane tree, then the wave
// partials in wave order; stage 2, on the device: the `parts` partials in index order — so every output repeats bit for bit.  No atomics.
#include "feature_common.h"

#define D2F_THREADS OP_THREADS

extern "C" int64_t st355_diff2flow_workspace(int64_t batch, int64_t per_sample) {
  if (batch <= 0 || per_sample <= 0) return 0;
  return (int64_t)sizeof(float) * batch * sample_parts(batch, per_sample);
}

struct D2fArgs {
  const bf16 *pred, *noisy, *tau;
  const int64_t* timesteps;
  const float *table, *weight, *emask;
  float* ws;
  bf16* dpred;
  int64_t per_sample, pred_stride, mask_period;
  int table_len;
  float dscale /* 2 grad_scale / (per_sample B) */;
};

// grid = (parts, B).  VEC: every per-sample base is 16-byte aligned and the mask period a multiple of 8
template <int MODE, bool VEC>
__global__ void __launch_bounds__(D2F_THREADS) k_d2f_loss(const D2fArgs a) {
  const int b = blockIdx.y;
  const int64_t n = a.per_sample, groups = (n + 7) >> 3;
  const bf16* __restrict__ p_ = a.pred + (int64_t)b * a.pred_stride;
  const bf16* __restrict__ x_ = a.noisy + (int64_t)b * n;
  const bf16* __restrict__ t_ = a.tau + (int64_t)b * n;
  bf16* __restrict__ d_ = a.dpred ? a.dpred + (int64_t)b * n : nullptr;
  const float* __restrict__ em = a.emask ? a.emask + (int64_t)b * a.mask_period : nullptr;
  int64_t t = a.timesteps[b];
  t = t < 0 ? 0 : (t > a.table_len - 1 ? a.table_len - 1 : t);          // the gather never leaves the table, whatever the batch holds
  const float c0 = a.table[2 * t], c1 = a.table[2 * t + 1];
  const float w = a.weight ? a.weight[b] : 1.f;
  const float k = MODE == 0 ? 1.f + c1 : c0 + c1;
  const float gcoef = a.dscale * w * k;
  float acc[1] = {0.f};
  for (int64_t i = (int64_t)blockIdx.x * D2F_THREADS + threadIdx.x; i < groups; i += (int64_t)gridDim.x * D2F_THREADS) {
    const int64_t e0 = i * 8;
    const int cnt = (n - e0) >= 8 ? 8 : (int)(n - e0);
    float pv[8], xv[8], tv[8], mk[8], dv[8];
    load8<VEC>(p_, e0, cnt, pv);
    load8<VEC>(x_, e0, cnt, xv);
    load8<VEC>(t_, e0, cnt, tv);
    if (em) {
      if (VEC) {
        ld8(em + e0 % a.mask_period, mk);
      } else {                                                    // (a scalar group may wrap around the period)
#pragma unroll
        for (int j = 0; j < 8; j++) mk[j] = j < cnt ? em[(e0 + j) % a.mask_period] : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) mk[j] = 1.f;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = pv[j], x = xv[j];
      const float z = c0 * x - c1 * p;
      float f;
      if (MODE == 0) {
        f = p - z;
      } else {
        const float e = c0 * p + c1 * x;
        f = e - z;
      }
      const float d = f - tv[j];
      if (VEC || j < cnt) acc[0] += d * d * mk[j];
      dv[j] = gcoef * d * mk[j];
    }
    if (d_) store8<VEC>(d_, e0, cnt, dv);
  }
  block_reduce<1>(acc, a.ws, b);
}

// stage 2, one workgroup: per sample the partials in index order -> per_sample[b] = weight[b] * sum / n; then the batch mean in sample order
// (weight == nullptr, lcm's loss: s * 1.f * inv is s * inv exactly)
__global__ void __launch_bounds__(D2F_THREADS) k_sample_mean_finish(const float* __restrict__ ws, const float* __restrict__ weight, float* __restrict__ loss,
                                                                   float* __restrict__ per_sample_out, int B, int parts, float inv_per_sample) {
  for (int b = threadIdx.x; b < B; b += D2F_THREADS) {
    float s = 0.f;
    for (int p = 0; p < parts; p++) s += ws[(int64_t)b * parts + p];
    per_sample_out[b] = s * (weight ? weight[b] : 1.f) * inv_per_sample;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; b++) s += per_sample_out[b];
    loss[0] = s / (float)B;
  }
}

// declared in feature_common.h: st355_lcm_loss (lcm.hip) launches it too, with weight == nullptr
void sample_mean_finish(hipStream_t st, const float* ws, const float* weight, float* loss, float* per_sample_out, int B, int parts, float inv_per_sample) {
  hipLaunchKernelGGL(k_sample_mean_finish, dim3(1), dim3(D2F_THREADS), 0, st, ws, weight, loss, per_sample_out, B, parts, inv_per_sample);
}

extern "C" int st355_diff2flow_loss(void* stream, const void* pred, int64_t pred_stride, const void* noisy, const void* tau, const int64_t* timesteps,
                                    const float* table, int table_len, int mode, const float* weight, const float* emask, int64_t mask_period,
                                    float* loss_out, float* per_sample_out, void* dpred, void* workspace, int64_t batch, int64_t per_sample,
                                    float grad_scale) {
  ST_REQUIRE(pred && noisy && tau && timesteps && table && loss_out && per_sample_out && workspace, "diff2flow_loss: null pointer");
  ST_REQUIRE((mode == 0 || mode == 1) && table_len > 0 && per_sample > 0 && batch > 0 && batch < 65536, "diff2flow_loss: bad args (mode %d, table_len %d, batch %ld)",
             mode, table_len, (long)batch);
  ST_REQUIRE(pred_stride >= per_sample, "diff2flow_loss: the prediction's per-sample stride (%ld) must be at least per_sample (%ld)", (long)pred_stride,
             (long)per_sample);
  ST_REQUIRE(!emask || (mask_period > 0 && per_sample % mask_period == 0), "diff2flow_loss: the element mask period must divide per_sample");
  ST_REQUIRE(dpred != pred, "diff2flow_loss: dpred and pred must be different buffers");
  const bool vec = per_sample % 8 == 0 && pred_stride % 8 == 0 && (((uintptr_t)pred | (uintptr_t)noisy | (uintptr_t)tau | (uintptr_t)dpred) & 15) == 0 &&
                   (!emask || (mask_period % 8 == 0 && ((uintptr_t)emask & 15) == 0));
  const int parts = sample_parts(batch, per_sample);
  const double n = (double)batch * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 12.0 * n, (6.0 + (emask ? 4.0 : 0.0) + (dpred ? 2.0 : 0.0)) * n);
  D2fArgs a;
  a.pred = (const bf16*)pred; a.noisy = (const bf16*)noisy; a.tau = (const bf16*)tau; a.timesteps = timesteps; a.table = table; a.weight = weight;
  a.emask = emask; a.ws = (float*)workspace; a.dpred = (bf16*)dpred; a.per_sample = per_sample; a.pred_stride = pred_stride; a.mask_period = mask_period;
  a.table_len = table_len;
  a.dscale = grad_scale * 2.0f / ((float)per_sample * (float)batch);
  const dim3 grid(parts, (unsigned)batch), block(D2F_THREADS);
  if (mode == 0) {
    if (vec) hipLaunchKernelGGL((k_d2f_loss<0, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_d2f_loss<0, false>), grid, block, 0, (hipStream_t)stream, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_d2f_loss<1, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_d2f_loss<1, false>), grid, block, 0, (hipStream_t)stream, a);
  }
  sample_mean_finish((hipStream_t)stream, (const float*)workspace, weight, loss_out, per_sample_out, (int)batch, parts, 1.0f / (float)per_sample);
  return st355_check_launch("diff2flow_loss");
}

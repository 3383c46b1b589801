// flow_dpo.hip — Flow-DPO preference training (distillation_method=flow_dpo; helpers/distillation/flow_dpo/distiller.py): the streaming kernels of the loss.
//
//   st355_flow_dpo_stats   one pass over policy [2B, n], ref [2B, n] (rows [0, B): preferred, [B, 2B): rejected), the two bf16 targets [B, n] and the optional mask:
//                          per pair the four masked errors sum m (x - t)^2 (for the logs), the two anchor sums sum (p - r)^2, the mask sum, and the two
//                          ADVANTAGES accumulated element by element:  sum m (r - p)(r + p - 2 t)  (preferred),  sum m (p - r)(p + r - 2 t)  (rejected)
//   st355_flow_dpo_head    one workgroup: nu, margin = nu (adv_w + adv_l), the auto-beta EMA (one device-resident scalar + its "initialised" flag), beta, the
//                          logits, the loss, the per-pair coefficient c_b = loss_weight beta sigma(-logit_b) / (2 B), and the log vector in one buffer
//   st355_flow_dpo_grad    d loss / d policy [2B, n] in ONE bf16 write:  +-2 c_b nu_b m (p - t) + anchor_alpha (p - r) / (B n),  times the upstream scale
//
// The margin comes from the element-wise advantages, never from E(ref) - E(policy): at LoRA initialisation policy ~ ref, and the difference of two fp32 sums of
// order n loses every digit of a margin that is small against them.  stats and grad stream 16 bytes per lane; the reductions run in two stages in a fixed order —
// stage 1: `parts` workgroups per pair, each lane a strided run of vectors, lane tree, then the wave partials in wave order; stage 2, on the device: the `parts`
// partials in index order — so every output repeats bit for bit, and nothing is read on the host.  No atomics.
#include "feature_common.h"

#define FD_THREADS OP_THREADS
#define FD_NS 9          // E_pw, E_pl, E_rw, E_rl, A_w, A_l, mask sum, adv_w, adv_l

// (sample_parts with the pairs as its samples)
extern "C" int64_t st355_flow_dpo_workspace(int64_t pairs, int64_t per_sample) {
  if (pairs <= 0 || per_sample <= 0) return 0;
  return (int64_t)sizeof(float) * FD_NS * pairs * sample_parts(pairs, per_sample);
}

__device__ __forceinline__ void fd_load_mask(const float* __restrict__ em, int64_t i, int64_t period, float (&mk)[8]) {
  if (em) {
    const int64_t off = (i * 8) % period;
    const f32x4 m0 = *(const f32x4*)(em + off), m1 = *(const f32x4*)(em + off + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) { mk[j] = m0[j]; mk[j + 4] = m1[j]; }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) mk[j] = 1.f;
  }
}

// ---- stats ----------------------------------------------------------------------------------------------------------------------------------------
// grid = (parts, B)
__global__ void __launch_bounds__(FD_THREADS) k_fd_stats(const bf16* __restrict__ policy, const bf16* __restrict__ ref, const bf16* __restrict__ tw,
                                                        const bf16* __restrict__ tl, const float* __restrict__ emask, int64_t mask_period, float* __restrict__ ws,
                                                        int64_t pairs, int64_t per_sample) {
  const int b = blockIdx.y;
  const int64_t win = (int64_t)b * per_sample, lose = ((int64_t)b + pairs) * per_sample, vecs = per_sample >> 3;
  const float* em = emask ? emask + (int64_t)b * mask_period : nullptr;
  float acc[FD_NS];
#pragma unroll
  for (int k = 0; k < FD_NS; k++) acc[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * FD_THREADS + threadIdx.x; i < vecs; i += (int64_t)gridDim.x * FD_THREADS) {
    const bf16x8 pwv = *(const bf16x8*)(policy + win + i * 8), plv = *(const bf16x8*)(policy + lose + i * 8);
    const bf16x8 rwv = *(const bf16x8*)(ref + win + i * 8), rlv = *(const bf16x8*)(ref + lose + i * 8);
    const bf16x8 twv = *(const bf16x8*)(tw + win + i * 8), tlv = *(const bf16x8*)(tl + win + i * 8);
    float mk[8];
    fd_load_mask(em, i, mask_period, mk);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float m = mk[j];
      const float pw = bf2f(pwv[j]), rw = bf2f(rwv[j]), t1 = bf2f(twv[j]);
      const float pl = bf2f(plv[j]), rl = bf2f(rlv[j]), t2 = bf2f(tlv[j]);
      const float epw = pw - t1, erw = rw - t1, epl = pl - t2, erl = rl - t2;
      const float dw = rw - pw, dl = pl - rl;
      acc[0] += m * (epw * epw);
      acc[1] += m * (epl * epl);
      acc[2] += m * (erw * erw);
      acc[3] += m * (erl * erl);
      acc[4] += dw * dw;
      acc[5] += dl * dl;
      acc[6] += m;
      acc[7] += m * (dw * ((rw + pw) - 2.f * t1));
      acc[8] += m * (dl * ((pl + rl) - 2.f * t2));
    }
  }
  block_reduce<FD_NS>(acc, ws, b);
}

// stage 2: stats[b, k] = the partials of (b, k) in index order.  grid = B, 64 threads (FD_NS used)
__global__ void k_fd_stats_finish(const float* __restrict__ ws, float* __restrict__ stats, int parts) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= FD_NS) return;
  float s = 0.f;
  for (int p = 0; p < parts; p++) s += ws[((int64_t)b * parts + p) * FD_NS + k];
  stats[(int64_t)b * FD_NS + k] = s;
}

static bool fd_mask_ok(const float* emask, int64_t mask_period, int64_t per_sample) {
  return !emask || (mask_period > 0 && mask_period % 8 == 0 && per_sample % mask_period == 0 && ((uintptr_t)emask & 15) == 0);
}

extern "C" int st355_flow_dpo_stats(void* stream, const void* policy, const void* ref, const void* target_w, const void* target_l, const float* emask,
                                    int64_t mask_period, float* stats_out, void* workspace, int64_t pairs, int64_t per_sample) {
  ST_REQUIRE(policy && ref && target_w && target_l && stats_out && workspace, "flow_dpo_stats: null pointer");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && pairs > 0 && pairs < 32768, "flow_dpo_stats: bad shape (per_sample %ld must be a multiple of 8, pairs %ld < 32768)",
             (long)per_sample, (long)pairs);
  ST_REQUIRE(fd_mask_ok(emask, mask_period, per_sample), "flow_dpo_stats: element mask period must be a multiple of 8 dividing per_sample (16-byte aligned)");
  const int parts = sample_parts(pairs, per_sample);
  const double n = (double)pairs * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 30.0 * n, 12.0 * n);
  float* ws = (float*)workspace;
  hipLaunchKernelGGL(k_fd_stats, dim3(parts, (unsigned)pairs), dim3(FD_THREADS), 0, (hipStream_t)stream, (const bf16*)policy, (const bf16*)ref,
                     (const bf16*)target_w, (const bf16*)target_l, emask, mask_period, ws, pairs, per_sample);
  hipLaunchKernelGGL(k_fd_stats_finish, dim3((unsigned)pairs), dim3(64), 0, (hipStream_t)stream, ws, stats_out, parts);
  return st355_check_launch("flow_dpo_stats");
}

// ---- head -----------------------------------------------------------------------------------------------------------------------------------------
struct FdHeadArgs {
  const float *stats, *original_loss;
  float *absmean, *ema_state, *pair, *loss, *logs;
  int B, norm_type, has_mask, mode, auto_beta;
  float inv_n, beta, auto_num, decay, beta_min, beta_max, eps, loss_weight, anchor_alpha, sft_weight;
};

// log sigma(x) = min(x, 0) - log1p(exp(-|x|));  sigma(-x) from the same exponential: finite for every finite x
__device__ __forceinline__ void fd_logsig(float x, float& logsig, float& sig_neg) {
  const float e = expf(-fabsf(x));
  logsig = fminf(x, 0.f) - log1pf(e);
  sig_neg = (x >= 0.f ? e : 1.f) / (1.f + e);
}

// one workgroup.  pair[b] = (margin, logit, c, nu).  mode 0: everything;  1: nu, the margins and absmean[0] = mean_b |margin_b| only (the rank mean of that
// scalar follows, outside);  2: everything, with absmean[0] as given
__global__ void __launch_bounds__(FD_THREADS) k_fd_head(const FdHeadArgs a) {
  __shared__ float s_beta;
  const int B = a.B;
  for (int b = threadIdx.x; b < B; b += FD_THREADS) {
    const float* st = a.stats + (int64_t)b * FD_NS;
    float nu = 1.f;
    if (a.norm_type == 1 || (a.norm_type == 2 && !a.has_mask)) nu = a.inv_n;
    else if (a.norm_type == 2) nu = 1.f / fmaxf(st[6], 1.f);
    a.pair[b * 4 + 0] = nu * (st[7] + st[8]);
    a.pair[b * 4 + 3] = nu;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float absmean;
    if (a.mode == 2) {
      absmean = a.absmean[0];
    } else {
      float s = 0.f;
      for (int b = 0; b < B; b++) s += fabsf(a.pair[b * 4 + 0]);
      absmean = s / (float)B;
      a.absmean[0] = absmean;
    }
    float beta = a.beta;
    if (a.mode != 1 && a.auto_beta) {
      float ema = a.ema_state[0];
      ema = (a.ema_state[1] != 0.f) ? a.decay * ema + (1.f - a.decay) * absmean : absmean;
      a.ema_state[0] = ema;
      a.ema_state[1] = 1.f;
      beta = fminf(fmaxf(a.auto_num / fmaxf(ema, a.eps), a.beta_min), a.beta_max);
    }
    s_beta = beta;
  }
  __syncthreads();
  if (a.mode == 1) return;
  const float beta = s_beta;
  for (int b = threadIdx.x; b < B; b += FD_THREADS) {
    const float logit = 0.5f * beta * a.pair[b * 4 + 0];
    float ls, sn;
    fd_logsig(logit, ls, sn);
    a.pair[b * 4 + 1] = logit;
    a.pair[b * 4 + 2] = a.loss_weight * 0.5f * beta * sn / (float)B;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s_ls = 0.f, s_sn = 0.f, s_m = 0.f, s_neg = 0.f, s_wa = 0.f, s_la = 0.f, s_e[4] = {0.f, 0.f, 0.f, 0.f}, s_aw = 0.f, s_al = 0.f;
    for (int b = 0; b < B; b++) {
      const float* st = a.stats + (int64_t)b * FD_NS;
      const float margin = a.pair[b * 4 + 0], nu = a.pair[b * 4 + 3];
      float ls, sn;
      fd_logsig(a.pair[b * 4 + 1], ls, sn);
      s_ls += ls;
      s_sn += sn;
      s_m += margin;
      s_neg += margin < 0.f ? 1.f : 0.f;
      s_wa += nu * st[7];
      s_la += nu * st[8];
#pragma unroll
      for (int k = 0; k < 4; k++) s_e[k] += nu * st[k];
      s_aw += st[4];
      s_al += st[5];
    }
    const float inv_b = 1.f / (float)B;
    const float dpo = -s_ls * inv_b;
    const float anchor = a.anchor_alpha != 0.f ? 0.5f * a.anchor_alpha * (s_aw * inv_b * a.inv_n + s_al * inv_b * a.inv_n) : 0.f;
    const float loss = dpo * a.loss_weight + anchor;
    a.loss[0] = loss;
    float* L = a.logs;
    L[0] = dpo;
    L[1] = beta;
    L[2] = s_m * inv_b;
    L[3] = s_wa * inv_b;
    L[4] = s_la * inv_b;
    L[5] = s_e[0] * inv_b;          // policy, preferred
    L[6] = s_e[1] * inv_b;          // policy, rejected
    L[7] = s_e[2] * inv_b;          // reference, preferred
    L[8] = s_e[3] * inv_b;          // reference, rejected
    L[9] = s_neg * inv_b * 100.f;
    L[10] = s_sn * inv_b;
    L[11] = (a.original_loss && a.sft_weight != 0.f) ? loss + a.sft_weight * a.original_loss[0] : loss;
    L[12] = anchor;
    L[13] = a.absmean[0];
    L[14] = a.auto_beta ? a.ema_state[0] : 0.f;
    L[15] = a.original_loss ? a.original_loss[0] : 0.f;
  }
}

extern "C" int st355_flow_dpo_head(void* stream, const float* stats, int norm_type, int has_mask, int mode, float* absmean_io, float* ema_state, int auto_beta,
                                   float beta, float auto_num, float decay, float beta_min, float beta_max, float eps, float loss_weight, float anchor_alpha,
                                   const float* original_loss, float sft_weight, float* pair_out, float* loss_out, float* logs_out, int64_t pairs,
                                   int64_t per_sample) {
  ST_REQUIRE(stats && absmean_io && pair_out && loss_out && logs_out, "flow_dpo_head: null pointer");
  ST_REQUIRE(norm_type >= 0 && norm_type <= 2 && mode >= 0 && mode <= 2 && pairs > 0 && pairs < 32768 && per_sample > 0, "flow_dpo_head: bad args");
  ST_REQUIRE(!auto_beta || ema_state, "flow_dpo_head: auto beta needs the device-resident EMA state (2 floats)");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 64.0 * pairs, 4.0 * (FD_NS + 4) * pairs);
  FdHeadArgs a;
  a.stats = stats; a.original_loss = original_loss; a.absmean = absmean_io; a.ema_state = ema_state; a.pair = pair_out; a.loss = loss_out; a.logs = logs_out;
  a.B = (int)pairs; a.norm_type = norm_type; a.has_mask = has_mask; a.mode = mode; a.auto_beta = auto_beta;
  a.inv_n = 1.0f / (float)per_sample; a.beta = beta; a.auto_num = auto_num; a.decay = decay; a.beta_min = beta_min; a.beta_max = beta_max; a.eps = eps;
  a.loss_weight = loss_weight; a.anchor_alpha = anchor_alpha; a.sft_weight = sft_weight;
  hipLaunchKernelGGL(k_fd_head, dim3(1), dim3(FD_THREADS), 0, (hipStream_t)stream, a);
  return st355_check_launch("flow_dpo_head");
}

// ---- grad -----------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FD_THREADS) k_fd_grad(const bf16* __restrict__ policy, const bf16* __restrict__ ref, const bf16* __restrict__ tw,
                                                       const bf16* __restrict__ tl, const float* __restrict__ emask, int64_t mask_period,
                                                       const float* __restrict__ pair, bf16* __restrict__ dpred, int64_t pairs, int64_t per_sample, float anchor_k,
                                                       float grad_scale, const float* __restrict__ grad_scale_dev) {
  const int64_t vps = per_sample >> 3, nvec = 2 * pairs * vps;
  const float gs = grad_scale_dev ? grad_scale * grad_scale_dev[0] : grad_scale;
  const float ak = anchor_k * gs;
  for (int64_t i = (int64_t)blockIdx.x * FD_THREADS + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * FD_THREADS) {
    const int64_t row = i / vps, iv = i - row * vps;
    const bool is_win = row < pairs;
    const int64_t b = is_win ? row : row - pairs;
    const float k = (is_win ? 2.f : -2.f) * pair[b * 4 + 2] * pair[b * 4 + 3] * gs;
    const bf16x8 pv = *(const bf16x8*)(policy + i * 8);
    const bf16x8 tv = *(const bf16x8*)((is_win ? tw : tl) + (b * vps + iv) * 8);
    bf16x8 rv, dv;
    if (ref) rv = *(const bf16x8*)(ref + i * 8);
    float mk[8];
    fd_load_mask(emask ? emask + b * mask_period : nullptr, iv, mask_period, mk);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float p = bf2f(pv[j]);
      float g = k * (mk[j] * (p - bf2f(tv[j])));
      if (ref) g += ak * (p - bf2f(rv[j]));
      dv[j] = f2bf(g);
    }
    *(bf16x8*)(dpred + i * 8) = dv;
  }
}

extern "C" int st355_flow_dpo_grad(void* stream, const void* policy, const void* ref, const void* target_w, const void* target_l, const float* emask,
                                   int64_t mask_period, const float* pair, void* dpred, int64_t pairs, int64_t per_sample, float anchor_alpha, float grad_scale,
                                   const float* grad_scale_dev) {
  ST_REQUIRE(policy && target_w && target_l && pair && dpred, "flow_dpo_grad: null pointer");
  ST_REQUIRE(anchor_alpha == 0.f || ref, "flow_dpo_grad: the anchor term (anchor_alpha != 0) needs the reference prediction");
  ST_REQUIRE(per_sample > 0 && per_sample % 8 == 0 && pairs > 0 && pairs < 32768, "flow_dpo_grad: bad shape (per_sample %ld must be a multiple of 8, pairs %ld < 32768)",
             (long)per_sample, (long)pairs);
  ST_REQUIRE(fd_mask_ok(emask, mask_period, per_sample), "flow_dpo_grad: element mask period must be a multiple of 8 dividing per_sample (16-byte aligned)");
  ST_REQUIRE(dpred != policy && dpred != ref, "flow_dpo_grad: dpred must be its own buffer");
  const double n = 2.0 * (double)pairs * per_sample;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * n, (anchor_alpha != 0.f ? 8.0 : 6.0) * n);
  const float anchor_k = anchor_alpha != 0.f ? anchor_alpha / ((float)pairs * (float)per_sample) : 0.f;
  hipLaunchKernelGGL(k_fd_grad, dim3(op_blocks((int64_t)(2 * pairs * per_sample / 8))), dim3(FD_THREADS), 0, (hipStream_t)stream, (const bf16*)policy,
                     (const bf16*)(anchor_alpha != 0.f ? ref : nullptr), (const bf16*)target_w, (const bf16*)target_l, emask, mask_period, pair, (bf16*)dpred, pairs,
                     per_sample, anchor_k, grad_scale, grad_scale_dev);
  return st355_check_launch("flow_dpo_grad");
}

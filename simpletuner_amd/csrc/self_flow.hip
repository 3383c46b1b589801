// self_flow.hip — Self-Flow (the reference's CREPA with crepa_feature_source=self_flow; helpers/training/crepa.py, helpers/models/common.py
// `_prepare_image_crepa_self_flow_batch`): the student sees a mixed tokenwise noise schedule, the EMA teacher the cleaner homogeneous view, and one student block is
// aligned to a deeper teacher block through the projector LayerNorm(D, eps 1e-5) -> Linear(D -> D).  All arithmetic fp32, bf16 only in memory, no atomics, every
// reduction in a fixed order (two calls give the same bits).  The projection, g = G W' and P = G^T xhat run on st355_gemm_bf16 / st355_gemm_tn_bf16, the cosine and
// G = d sim / d proj on st355_layersync_fwd, the LayerNorm backward on st355_nextlat_ln_bwd_add.  Here (fold, rows and wgrad on the kernels of feature_common.h):
//   st355_self_flow_views   both noisy views, the student's token timesteps and the teacher's sigma / timestep in ONE streaming pass (16 bytes per lane)
//   st355_self_flow_fold    W' = bf16(gamma * W) [D, D], its transpose, c = bf16(W beta + b): 64 x 64 tiles through LDS
//   st355_self_flow_rows    xhat, rstd of nn.LayerNorm's default eps 1e-5
//   st355_self_flow_wgrad   dW, db, d gamma, d beta from P [D, D] and db
#include "feature_common.h"

#define SF_MAX_D 4096                 // (the eps of nn.LayerNorm(hidden_size), crepa.py `attach_to_model`, is RowEps1e5)

// ---- the two views ----
// VEC elements per lane (8 bf16 / 4 fp32 = 16 bytes).  blockIdx.y = sample; a lane owns elements [VEC i, VEC i + VEC) of the sample's C * H * W (any of which may
// lie in another image row or token: the (y, x) and the token of the first come from the lane's only divisions, the others step from them).  The mask is a function of the token alone, so the
// channel never enters.  The lanes of a sample also walk its tokens (timesteps) in a stride of the sample's lane count; lane 0 writes the teacher's pair.
template <typename T, int VEC> struct sf_vec;
template <> struct sf_vec<bf16, 8> { typedef bf16x8 type; };
template <> struct sf_vec<float, 4> { typedef f32x4 type; };

template <typename T, int VEC>
__global__ void __launch_bounds__(256) k_sf_views(const T* __restrict__ lat, const T* __restrict__ noise, int64_t lat_bstride, int64_t noise_bstride,
                                                  const float* __restrict__ sigma, const float* __restrict__ sigma_alt, const float* __restrict__ ts,
                                                  const float* __restrict__ ts_alt, const float* __restrict__ uniforms, float ratio, int p, T* __restrict__ noisy_s,
                                                  T* __restrict__ noisy_t, float* __restrict__ tok_t, float* __restrict__ sigma_T, float* __restrict__ t_T,
                                                  float* __restrict__ sigma_grid, int H, int W, int64_t per) {
  typedef typename sf_vec<T, VEC>::type vec_t;
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, lanes = (int64_t)gridDim.x * 256;
  const int wt = W / p, ntok = (H / p) * wt, HW = H * W;
  const float s0 = sigma[b], s1 = sigma_alt[b], t0 = ts[b], t1 = ts_alt[b];
  const float sT = fminf(s0, s1);
  const float* ub = uniforms + (int64_t)b * ntok;
  for (int64_t k = i; k < ntok; k += lanes) tok_t[(int64_t)b * ntok + k] = ub[k] < ratio ? t1 : t0;
  if (i == 0) {
    sigma_T[b] = sT;
    t_T[b] = fminf(t0, t1);
  }
  const int64_t e0 = i * VEC;
  if (e0 >= per) return;                                          // per % VEC == 0: a lane's elements lie wholly inside or outside
  // the first element's (y, x) and its token (ty, tx) with the offsets (ry, rx) inside the patch: the only divisions of the lane (32-bit: per < 2^31); the
  // others step from it.  All token indices first, then their uniforms as independent loads (neighbours share a token: L1 hits), then the arithmetic — a load that
  // waited for the previous element's compare made the lane a chain of memory latencies
  const int rem = (int)((uint32_t)e0 % (uint32_t)HW);
  int y = rem / W, x = rem - y * W;
  int ty = y / p, ry = y - ty * p, tx = x / p, rx = x - tx * p;
  int tk[VEC];
#pragma unroll
  for (int j = 0; j < VEC; j++) {
    tk[j] = ty * wt + tx;                                         // ty < H / p, tx < W / p always: inside the sample's uniforms
    ++x;
    if (++rx == p) { rx = 0; ++tx; }
    if (x == W) {                                                 // the next image row (behind the last one: the next channel's first)
      x = 0; tx = 0; rx = 0;
      ++y;
      if (++ry == p) { ry = 0; ++ty; }
      if (y == H) { y = 0; ty = 0; ry = 0; }
    }
  }
  const vec_t lv = *(const vec_t*)(lat + (int64_t)b * lat_bstride + e0), nv = *(const vec_t*)(noise + (int64_t)b * noise_bstride + e0);
  float uu[VEC];
#pragma unroll
  for (int j = 0; j < VEC; j++) uu[j] = ub[tk[j]];
  vec_t os, ot;
#pragma unroll
  for (int j = 0; j < VEC; j++) {
    const float sg = uu[j] < ratio ? s1 : s0;
    const float l = (float)lv[j], n = (float)nv[j];
    os[j] = (T)fmaf(sg, n, (1.f - sg) * l);
    ot[j] = (T)fmaf(sT, n, (1.f - sT) * l);
    if (sigma_grid && e0 + j < HW) sigma_grid[(int64_t)b * HW + e0 + j] = sg;      // channel 0's lanes cover every (y, x) once
  }
  *(vec_t*)(noisy_s + (int64_t)b * per + e0) = os;
  *(vec_t*)(noisy_t + (int64_t)b * per + e0) = ot;
}

extern "C" int st355_self_flow_views(void* stream, const void* latents, const void* noise, int in_bf16, int64_t lat_bstride, int64_t noise_bstride, const float* sigma,
                                     const float* sigma_alt, const float* timesteps, const float* timesteps_alt, const float* uniforms, float ratio, int patch,
                                     void* noisy_student, void* noisy_teacher, float* token_timesteps, float* sigma_teacher, float* timestep_teacher,
                                     float* sigma_grid, int B, int Cc, int H, int W) {
  ST_REQUIRE(latents && noise && sigma && sigma_alt && timesteps && timesteps_alt && uniforms && noisy_student && noisy_teacher && token_timesteps && sigma_teacher &&
                 timestep_teacher,
             "self_flow_views: bad args");
  ST_REQUIRE(B > 0 && B <= 65535 && Cc > 0 && H > 0 && W > 0 && patch > 0, "self_flow_views: B in [1, 65535], C, H, W and the patch size positive");
  ST_REQUIRE(H % patch == 0 && W % patch == 0,
             "self_flow_views: H %% patch_size != 0 or W %% patch_size != 0 (H = %d, W = %d, patch_size = %d): the reference's repeat_interleave and slice are not a "
             "defined computation there",
             H, W, patch);
  ST_REQUIRE(ratio >= 0.f && ratio <= 0.5f, "self_flow_views: the mask ratio must lie in [0, 0.5] (got %g)", (double)ratio);
  const int vec = in_bf16 ? 8 : 4;
  const int64_t per = (int64_t)Cc * H * W;
  ST_REQUIRE(per <= 0x7fffffff && per % vec == 0, "self_flow_views: C * H * W must be a multiple of %d elements (16 bytes per lane) below 2^31, got %lld", vec, (long long)per);
  ST_REQUIRE(lat_bstride >= per && noise_bstride >= per && lat_bstride % vec == 0 && noise_bstride % vec == 0,
             "self_flow_views: the batch strides must be at least C * H * W and multiples of %d elements", vec);
  ST_REQUIRE(((uintptr_t)latents | (uintptr_t)noise | (uintptr_t)noisy_student | (uintptr_t)noisy_teacher) % 16 == 0, "self_flow_views: operands must be 16-byte aligned");
  const int64_t blocks = cdiv64(per / vec, 256);
  ST_REQUIRE(blocks <= 0x7fffffff, "self_flow_views: too many elements per sample");
  const double es = in_bf16 ? 2.0 : 4.0;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * B * per, 4.0 * es * B * per);
  const dim3 grid((unsigned)blocks, (unsigned)B), block(256);
  if (in_bf16)
    hipLaunchKernelGGL((k_sf_views<bf16, 8>), grid, block, 0, (hipStream_t)stream, (const bf16*)latents, (const bf16*)noise, lat_bstride, noise_bstride, sigma, sigma_alt,
                       timesteps, timesteps_alt, uniforms, ratio, patch, (bf16*)noisy_student, (bf16*)noisy_teacher, token_timesteps, sigma_teacher, timestep_teacher,
                       sigma_grid, H, W, per);
  else
    hipLaunchKernelGGL((k_sf_views<float, 4>), grid, block, 0, (hipStream_t)stream, (const float*)latents, (const float*)noise, lat_bstride, noise_bstride, sigma,
                       sigma_alt, timesteps, timesteps_alt, uniforms, ratio, patch, (float*)noisy_student, (float*)noisy_teacher, token_timesteps, sigma_teacher,
                       timestep_teacher, sigma_grid, H, W, per);
  return st355_check_launch("self_flow_views");
}

// ---- fold ----
// W [D, D] fp32 -> Wf = bf16(W * gamma[col]) and WfT its transpose: k_fold_mat.  c[n] = bf16(sum_d W[n, d] beta[d] + b[n]): a wave per row n
__global__ void __launch_bounds__(ROWS_PER_BLOCK* WAVE) k_sf_fold_vec(const float* __restrict__ W, const float* __restrict__ beta, const float* __restrict__ b,
                                                                      bf16* __restrict__ c, int D) {
  const int lane = threadIdx.x & (WAVE - 1), n = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (n >= D) return;                                             // wave-uniform
  fold_row_dot(W, beta, b, c, D, n, lane);
}

#define SF_REQUIRE_D(name) ST_REQUIRE(D > 0 && D % 8 == 0 && D <= SF_MAX_D, name ": D must be a multiple of 8, at most %d (got %d)", SF_MAX_D, D)

extern "C" int st355_self_flow_fold(void* stream, const float* gamma, const float* beta, const float* W, const float* b, void* Wf, void* WfT, void* c, int D) {
  ST_REQUIRE(gamma && beta && W && b && Wf && WfT && c, "self_flow_fold: bad args");
  SF_REQUIRE_D("self_flow_fold");
  ST_REQUIRE(((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W | (uintptr_t)Wf | (uintptr_t)WfT) % 16 == 0, "self_flow_fold: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 3.0 * D * D, 12.0 * D * D);
  const int tiles = (D + FOLD_TILE - 1) / FOLD_TILE;
  hipLaunchKernelGGL(k_fold_mat<float>, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, W, gamma, (bf16*)Wf, (bf16*)WfT, D, D);
  hipLaunchKernelGGL(k_sf_fold_vec, dim3((D + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, W, beta, b, (bf16*)c, D);
  return st355_check_launch("self_flow_fold");
}

// ---- the row pass: k_rows_fwd with eps 1e-5 ----
extern "C" int st355_self_flow_rows(void* stream, const void* h, void* xhat, float* rstd, int B, int rows, int D, int64_t ld, int64_t bstride) {
  ST_REQUIRE(h && xhat && rstd && B > 0 && rows > 0, "self_flow_rows: bad args");
  SF_REQUIRE_D("self_flow_rows");
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "self_flow_rows: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)h | (uintptr_t)xhat) % 16 == 0, "self_flow_rows: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  ST_REQUIRE(cdiv64(n, ROWS_PER_BLOCK) <= 0x7fffffff, "self_flow_rows: too many rows");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * n * D, 4.0 * n * D);
  rows_fwd_launch<RowEps1e5>((hipStream_t)stream, (const bf16*)h, (bf16*)xhat, rstd, rows, D, n, ld, bstride);
  return st355_check_launch("self_flow_rows");
}

// ---- weight gradients: k_wgrad_up / k_wgrad_up_final over the N = D rows of W, fp32 parameters ----
extern "C" int64_t st355_self_flow_wgrad_workspace(int D) { return D > 0 ? wgrad_up_workspace(D, D) : 0; }

extern "C" int st355_self_flow_wgrad(void* stream, const void* P, const float* db, const float* gamma, const float* beta, const float* W, const float* scale_dev,
                                     float* g_gamma, float* g_beta, float* g_W, float* g_b, int D, int accumulate, void* ws) {
  ST_REQUIRE(P && db && gamma && beta && W && scale_dev && g_gamma && g_beta && g_W && g_b && ws, "self_flow_wgrad: bad args");
  SF_REQUIRE_D("self_flow_wgrad");
  ST_REQUIRE(((uintptr_t)P | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W | (uintptr_t)g_W | (uintptr_t)ws) % 16 == 0, "self_flow_wgrad: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * D * D, 10.0 * D * D);
  wgrad_up_launch<float, true>((hipStream_t)stream, P, db, gamma, beta, W, scale_dev, g_gamma, g_beta, g_W, g_b, (float*)ws, D, D, accumulate);
  return st355_check_launch("self_flow_wgrad");
}

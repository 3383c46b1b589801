// self_flow.hip — Self-Flow (the reference's CREPA with crepa_feature_source=self_flow; helpers/training/crepa.py, helpers/models/common.py
// `_prepare_image_crepa_self_flow_batch`): the student sees a mixed tokenwise noise schedule, the EMA teacher the cleaner homogeneous view, and one student block is
// aligned to a deeper teacher block through the projector LayerNorm(D, eps 1e-5) -> Linear(D -> D).  All arithmetic fp32, bf16 only in memory, no atomics, every
// reduction in a fixed order (two calls give the same bits).  The projection, g = G W' and P = G^T xhat run on st355_gemm_bf16 / st355_gemm_tn_bf16, the cosine and
// G = d sim / d proj on st355_layersync_fwd, the LayerNorm backward on st355_nextlat_ln_bwd_add.  Here, because no existing entry has the contract:
//   st355_self_flow_views   both noisy views, the student's token timesteps and the teacher's sigma / timestep in ONE streaming pass (16 bytes per lane)
//   st355_self_flow_fold    W' = bf16(gamma * W) [D, D], its transpose, c = bf16(W beta + b): 64 x 64 tiles through LDS (st355_nextlat_fold takes two matrices of 2D rows)
//   st355_self_flow_rows    xhat, rstd of nn.LayerNorm's default eps 1e-5 (st355_ig_head_fwd has the heads' 1e-6 compiled in)
//   st355_self_flow_wgrad   dW, db, d gamma, d beta from P [D, D] and db (st355_nextlat_wgrad_up has 2D rows compiled in)
#include "common.h"

#define SF_MAX_D 4096
#define SF_EPS 1e-5f                  // nn.LayerNorm(hidden_size): the default eps (crepa.py `attach_to_model`)
#define SF_PASS_COLS 512              // 64 lanes x 8 bf16
#define SF_MAX_PASSES 8               // D <= 4096
#define SF_ROWS_PER_BLOCK 4           // row kernels: one wave per row
#define SF_TILE 64                    // fold: tile edge
#define SF_WG_ROWS 256                // wgrad: rows of W per workgroup
#define SF_WG_COLS 64                 //        and columns

__device__ __forceinline__ void sf_ld8(const float* p, float (&v)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void sf_ld8(const bf16* p, float (&v)[8]) {
  const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = bf2f(a[j]);
}
__device__ __forceinline__ void sf_st8(float* p, const float (&v)[8], int accumulate) {
  float o[8];
  if (accumulate) {
    sf_ld8(p, o);
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] += v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = v[j];
  }
  *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
  *(float4*)(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

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
// W [D, D] fp32 -> Wf = bf16(W * gamma[col]) and WfT its transpose.  A workgroup owns a 64 x 64 tile: thread (row = tid >> 3, chunk = tid & 7) converts 8 columns of
// rows row and row + 32, stores them straight (8 lanes = 128 contiguous bytes of a row) and into the LDS tile; behind the barrier thread (col = tid >> 3, i = tid & 7)
// gathers rows 8 i .. 8 i + 7 of columns col and col + 32 and stores 16 bytes of WfT.  The 16-byte chunk index of a tile row is XORed with (row >> 3) & 7, so the
// gather's eight row groups land in eight different chunks (a plain row pitch of 128 bytes would put them all on the same banks).
__global__ void __launch_bounds__(256) k_sf_fold_mat(const float* __restrict__ W, const float* __restrict__ gamma, bf16* __restrict__ Wf, bf16* __restrict__ WfT, int D) {
  __shared__ __attribute__((aligned(16))) bf16 tile[SF_TILE * SF_TILE];
  const int tid = threadIdx.x, r0 = blockIdx.y * SF_TILE, c0 = blockIdx.x * SF_TILE, ch = tid & 7;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int r = (tid >> 3) + 32 * k, gr = r0 + r, gc = c0 + ch * 8;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = f2bf(0.f);
    if (gr < D && gc < D) {                                       // D % 8 == 0: a chunk lies wholly inside or outside
      float v[8], s[8];
      sf_ld8(W + (int64_t)gr * D + gc, v);
      sf_ld8(gamma + gc, s);
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf(v[j] * s[j]);
      *(bf16x8*)(Wf + (int64_t)gr * D + gc) = o;
    }
    *(bf16x8*)(&tile[r * SF_TILE + ((ch ^ ((r >> 3) & 7)) << 3)]) = o;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int cc = (tid >> 3) + 32 * k, i = tid & 7, gcc = c0 + cc, gr = r0 + 8 * i;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = tile[(8 * i + j) * SF_TILE + ((((cc >> 3) ^ i) << 3) | (cc & 7))];
    if (gcc < D && gr < D) *(bf16x8*)(WfT + (int64_t)gcc * D + gr) = o;
  }
}

// c[n] = bf16(sum_d W[n, d] beta[d] + b[n]): a wave per row n, a lane's partial in column order, then the xor butterfly
__global__ void __launch_bounds__(SF_ROWS_PER_BLOCK* WAVE) k_sf_fold_vec(const float* __restrict__ W, const float* __restrict__ beta, const float* __restrict__ b,
                                                                         bf16* __restrict__ c, int D) {
  const int lane = threadIdx.x & (WAVE - 1), n = blockIdx.x * SF_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (n >= D) return;                                             // wave-uniform
  float a = 0.f;
  for (int d = lane * 8; d < D; d += SF_PASS_COLS) {
    float w[8], be[8];
    sf_ld8(W + (int64_t)n * D + d, w);
    sf_ld8(beta + d, be);
#pragma unroll
    for (int j = 0; j < 8; j++) a = fmaf(w[j], be[j], a);
  }
  a = wave_sum(a);
  if (lane == 0) c[n] = f2bf(a + b[n]);
}

#define SF_REQUIRE_D(name) ST_REQUIRE(D > 0 && D % 8 == 0 && D <= SF_MAX_D, name ": D must be a multiple of 8, at most %d (got %d)", SF_MAX_D, D)

extern "C" int st355_self_flow_fold(void* stream, const float* gamma, const float* beta, const float* W, const float* b, void* Wf, void* WfT, void* c, int D) {
  ST_REQUIRE(gamma && beta && W && b && Wf && WfT && c, "self_flow_fold: bad args");
  SF_REQUIRE_D("self_flow_fold");
  ST_REQUIRE(((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W | (uintptr_t)Wf | (uintptr_t)WfT) % 16 == 0, "self_flow_fold: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 3.0 * D * D, 12.0 * D * D);
  const int tiles = (D + SF_TILE - 1) / SF_TILE;
  hipLaunchKernelGGL(k_sf_fold_mat, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, W, gamma, (bf16*)Wf, (bf16*)WfT, D);
  hipLaunchKernelGGL(k_sf_fold_vec, dim3((D + SF_ROWS_PER_BLOCK - 1) / SF_ROWS_PER_BLOCK), dim3(SF_ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, W, beta, b, (bf16*)c, D);
  return st355_check_launch("self_flow_fold");
}

// ---- the row pass ----
// a wave per row of the [B, rows, D] view; a lane keeps its elements (packed bf16, 8 per pass) between the two reductions and the store: mean, CENTRED variance
__global__ void __launch_bounds__(SF_ROWS_PER_BLOCK* WAVE) k_sf_rows(const bf16* __restrict__ h, bf16* __restrict__ xhat, float* __restrict__ rstd, int rows, int D,
                                                                     int64_t n_rows, int64_t ld, int64_t bstride, float inv_d) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t row = (int64_t)blockIdx.x * SF_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                      // wave-uniform: the last block may be partly empty
  const bf16* hp = h + (row / rows) * bstride + (row % rows) * ld;
  bf16x8 v[SF_MAX_PASSES];
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < SF_MAX_PASSES; p++) {
    const int c = p * SF_PASS_COLS + lane * 8;
    if (c < D) {                                                  // D % 8 == 0 keeps a lane's 8 columns together
      v[p] = *(const bf16x8*)(hp + c);
#pragma unroll
      for (int j = 0; j < 8; j++) s += bf2f(v[p][j]);
    }
  }
  const float mean = wave_sum(s) * inv_d;                         // xor butterfly: every lane holds the same bits
  float q = 0.f;
#pragma unroll
  for (int p = 0; p < SF_MAX_PASSES; p++) {
    if (p * SF_PASS_COLS + lane * 8 < D) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = bf2f(v[p][j]) - mean;
        q = fmaf(d, d, q);
      }
    }
  }
  const float rs = 1.f / sqrtf(wave_sum(q) * inv_d + SF_EPS);
  if (lane == 0) rstd[row] = rs;
  bf16* xp = xhat + row * (int64_t)D;
#pragma unroll
  for (int p = 0; p < SF_MAX_PASSES; p++) {
    const int c = p * SF_PASS_COLS + lane * 8;
    if (c < D) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = f2bf((bf2f(v[p][j]) - mean) * rs);
      *(bf16x8*)(xp + c) = o;
    }
  }
}

extern "C" int st355_self_flow_rows(void* stream, const void* h, void* xhat, float* rstd, int B, int rows, int D, int64_t ld, int64_t bstride) {
  ST_REQUIRE(h && xhat && rstd && B > 0 && rows > 0, "self_flow_rows: bad args");
  SF_REQUIRE_D("self_flow_rows");
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "self_flow_rows: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)h | (uintptr_t)xhat) % 16 == 0, "self_flow_rows: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * rows;
  ST_REQUIRE(cdiv64(n, SF_ROWS_PER_BLOCK) <= 0x7fffffff, "self_flow_rows: too many rows");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * n * D, 4.0 * n * D);
  hipLaunchKernelGGL(k_sf_rows, dim3((unsigned)cdiv64(n, SF_ROWS_PER_BLOCK)), dim3(SF_ROWS_PER_BLOCK * WAVE), 0, (hipStream_t)stream, (const bf16*)h, (bf16*)xhat, rstd,
                     rows, D, n, ld, bstride, (float)(1.0 / (double)D));
  return st355_check_launch("self_flow_rows");
}

// ---- weight gradients ----
// stage 1: workgroup (column tile, row chunk) owns 64 columns x 256 rows of W.  Thread (cg = tid & 7, rl = tid >> 3) walks rows rl, rl + 32, ... of its 8 columns: dW on
// the way, its partial sums of W * P and W * db in row order; the 32 row lanes meet in LDS ([32][65] fp32) and are added in row-lane order into ws[chunk][0 / 1][D].
// Column tile 0 also writes db of its rows.  stage 2 adds the chunks in order.
__global__ void __launch_bounds__(256) k_sf_wgrad(const bf16* __restrict__ P, const float* __restrict__ db, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ W, const float* __restrict__ scale, float* g_W, float* g_b, float* __restrict__ ws, int D,
                                                  int accumulate) {
  __shared__ float sg[32][SF_WG_COLS + 1], sb[32][SF_WG_COLS + 1];
  const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
  const int c = blockIdx.x * SF_WG_COLS + cg * 8, n0 = blockIdx.y * SF_WG_ROWS;
  const float s = scale[0];
  if (blockIdx.x == 0 && n0 + tid < D) {
    const float v = s * db[n0 + tid];
    g_b[n0 + tid] = accumulate ? g_b[n0 + tid] + v : v;
  }
  float dg[8], dbe[8];
#pragma unroll
  for (int j = 0; j < 8; j++) dg[j] = dbe[j] = 0.f;
  if (c < D) {
    float ga[8], be[8];
    sf_ld8(gamma + c, ga);
    sf_ld8(beta + c, be);
#pragma unroll 2
    for (int i = 0; i < SF_WG_ROWS / 32; i++) {
      const int n = n0 + rl + 32 * i;
      if (n < D) {
        float p[8], w[8], o[8];
        sf_ld8(P + (int64_t)n * D + c, p);
        sf_ld8(W + (int64_t)n * D + c, w);
        const float bn = db[n];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          o[j] = s * fmaf(p[j], ga[j], bn * be[j]);
          dg[j] = fmaf(w[j], p[j], dg[j]);
          dbe[j] = fmaf(w[j], bn, dbe[j]);
        }
        sf_st8(g_W + (int64_t)n * D + c, o, accumulate);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    sg[rl][cg * 8 + j] = dg[j];
    sb[rl][cg * 8 + j] = dbe[j];
  }
  __syncthreads();
  if (tid < 2 * SF_WG_COLS) {
    const int col = tid & (SF_WG_COLS - 1), which = tid >> 6, d = blockIdx.x * SF_WG_COLS + col;      // wave 0: gamma sums, wave 1: beta sums
    if (d < D) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 32; k++) a += which ? sb[k][col] : sg[k][col];
      ws[((int64_t)blockIdx.y * 2 + which) * D + d] = a;
    }
  }
}

__global__ void __launch_bounds__(256) k_sf_wgrad_final(const float* __restrict__ ws, const float* __restrict__ scale, float* g_gamma, float* g_beta, int D, int chunks,
                                                        int accumulate) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < chunks; k++) {
    a += ws[((int64_t)k * 2) * D + d];
    b += ws[((int64_t)k * 2 + 1) * D + d];
  }
  const float s = scale[0];
  g_gamma[d] = accumulate ? g_gamma[d] + s * a : s * a;
  g_beta[d] = accumulate ? g_beta[d] + s * b : s * b;
}

extern "C" int64_t st355_self_flow_wgrad_workspace(int D) { return D > 0 ? (int64_t)((D + SF_WG_ROWS - 1) / SF_WG_ROWS) * 2 * D * 4 : 0; }

extern "C" int st355_self_flow_wgrad(void* stream, const void* P, const float* db, const float* gamma, const float* beta, const float* W, const float* scale_dev,
                                     float* g_gamma, float* g_beta, float* g_W, float* g_b, int D, int accumulate, void* ws) {
  ST_REQUIRE(P && db && gamma && beta && W && scale_dev && g_gamma && g_beta && g_W && g_b && ws, "self_flow_wgrad: bad args");
  SF_REQUIRE_D("self_flow_wgrad");
  ST_REQUIRE(((uintptr_t)P | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)W | (uintptr_t)g_W | (uintptr_t)ws) % 16 == 0, "self_flow_wgrad: operands must be 16-byte aligned");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 6.0 * D * D, 10.0 * D * D);
  const int chunks = (D + SF_WG_ROWS - 1) / SF_WG_ROWS;
  hipLaunchKernelGGL(k_sf_wgrad, dim3((D + SF_WG_COLS - 1) / SF_WG_COLS, chunks), dim3(256), 0, (hipStream_t)stream, (const bf16*)P, db, gamma, beta, W, scale_dev, g_W, g_b,
                     (float*)ws, D, accumulate);
  hipLaunchKernelGGL(k_sf_wgrad_final, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)ws, scale_dev, g_gamma, g_beta, D, chunks, accumulate);
  return st355_check_launch("self_flow_wgrad");
}

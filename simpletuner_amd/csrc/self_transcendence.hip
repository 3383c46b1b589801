// self_transcendence.hip — the projector of Self-Transcendence (helpers/distillation/self_transcendence/distiller.py): Linear(D -> Hp) -> SiLU -> Linear(Hp -> Hp) -> SiLU ->
// Linear(Hp -> D) on one block's image-token rows [B, S, D], trained under a per-sample MSE that only the samples with timestep_min <= sigma_b <= timestep_max take part
// in: against the patchified diffusion target (stage `vae`: the first P = C ph pw columns of the projection) or against the frozen teacher's feature-space CFG target
// u + s (c - u) (stage `self`).  All arithmetic fp32, bf16 only in memory, no atomics, every reduction in a fixed order (two calls give the same bits).  The GEMMs
// (U1 = X W1^T + b1, U2 = A1 W2^T + b2, pred = A2 W3^T + b3, dA2 = G W3, dA1 = dU2 W2, dX = dU1 W1, the three P = dY^T A products) run on st355_gemm_bf16 /
// st355_gemm_tn_bf16, SiLU and its derivative on st355_silu / st355_silu_bwd, the bias sums on st355_colsum_prod.  Here:
//   st355_st_fold       ONE launch: bf16(W1) [Hp, D], bf16(W2) [Hp, Hp], the first P3 rows of bf16(W3) [D, Hp], each with its transpose, and the three biases (the
//                       first P3 of b3).  64 x 64 tiles through LDS: both the straight and the transposed store write 128 contiguous bytes per 8 lanes.
//   st355_st_vae_loss   pred [B S, P] against target[b, c, i ph + a, j pw + e] read in place (token (i, j) of the gh x gw grid, column (c, a, e)).
//   st355_st_cfg_loss   pred [B S, D] against u + s (c - u), c / u the rows of samples b and B + b of the teacher's [2B, S, D] capture, formed in fp32.
//                       Both: per-(sample, chunk) partial sums of (pred - t)^2 in a workspace, then one workgroup adds each sample's chunks in index order, takes
//                       the per-sample means, the mask from sigma on the device, and the mean over the active samples in sample order; stats = (loss, n_active,
//                       1 / (n_active S P) or 0).  G = 2 (pred - t) of an active sample, exactly 0 of an inactive one, written over pred (one bf16 rounding).
//   st355_st_wgrad      g_W [R, Cc] (+)= s P, g_b [R] (+)= s db: P bf16 from gemm_tn, db fp32 from colsum_prod, s ONE fp32 on the device.
//   st355_st_dx_add     dx[b, r, :] = bf16(float(dx) + s g[b rows + r, :]): a compact [B rows, D] addend into a strided [B, rows, D] view.
// s is ONE fp32 on the device (weight x the upstream gradient x the accumulation division x stats[2]): G stays unscaled through the bf16 chain.
#include "feature_common.h"

#define STR_BLOCK 256
#define STR_MAX_CHUNKS 256            // loss: workgroups per sample
#define STR_MAX_B 4096

// ---- fold ----
// the three matrices tile by tile on fold_tile of feature_common.h (fp32 sources, no column scale)
struct StrFold {
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  bf16 *W1h, *W1T, *b1h, *W2h, *W2T, *b2h, *W3h, *W3T, *b3h;
  int D, Hp, P3;
  int t1, t2, t3;                       // tiles of the three matrices; the workgroups behind them convert the biases
};

// workgroup-uniform dispatch on blockIdx.x: [0, t1) W1 [Hp, D], [t1, t1 + t2) W2 [Hp, Hp], [.., + t3) the first P3 rows of W3 [D, Hp], then b1 | b2 | b3[:P3], 8 per lane
__global__ void __launch_bounds__(STR_BLOCK) k_str_fold(StrFold a) {
  __shared__ __attribute__((aligned(16))) bf16 tile[FOLD_TILE * FOLD_TILE];
  int blk = blockIdx.x;
  const int tcD = (a.D + FOLD_TILE - 1) / FOLD_TILE, tcH = (a.Hp + FOLD_TILE - 1) / FOLD_TILE;
  if (blk < a.t1) {
    fold_tile(tile, a.W1, (const float*)nullptr, a.W1h, a.W1T, a.Hp, a.D, (blk / tcD) * FOLD_TILE, (blk % tcD) * FOLD_TILE);
    return;
  }
  blk -= a.t1;
  if (blk < a.t2) {
    fold_tile(tile, a.W2, (const float*)nullptr, a.W2h, a.W2T, a.Hp, a.Hp, (blk / tcH) * FOLD_TILE, (blk % tcH) * FOLD_TILE);
    return;
  }
  blk -= a.t2;
  if (blk < a.t3) {
    fold_tile(tile, a.W3, (const float*)nullptr, a.W3h, a.W3T, a.P3, a.Hp, (blk / tcH) * FOLD_TILE, (blk % tcH) * FOLD_TILE);
    return;
  }
  blk -= a.t3;
  const int e = (blk * STR_BLOCK + threadIdx.x) * 8;            // Hp % 8 == 0 and P3 % 8 == 0: a chunk lies inside one bias
  const float* src;
  bf16* dst;
  if (e < a.Hp) { src = a.b1 + e; dst = a.b1h + e; }
  else if (e < 2 * a.Hp) { src = a.b2 + (e - a.Hp); dst = a.b2h + (e - a.Hp); }
  else if (e < 2 * a.Hp + a.P3) { src = a.b3 + (e - 2 * a.Hp); dst = a.b3h + (e - 2 * a.Hp); }
  else return;
  float v[8];
  ld8(src, v);
  st8(dst, v, 0);
}

extern "C" int st355_st_fold(void* stream, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3, void* W1h, void* W1T,
                             void* b1h, void* W2h, void* W2T, void* b2h, void* W3h, void* W3T, void* b3h, int D, int Hp, int P3) {
  ST_REQUIRE(W1 && b1 && W2 && b2 && W3 && b3 && W1h && W1T && b1h && W2h && W2T && b2h && W3h && W3T && b3h, "st_fold: bad args");
  ST_REQUIRE(D > 0 && D % 8 == 0 && Hp > 0 && Hp % 8 == 0 && P3 > 0 && P3 % 8 == 0 && P3 <= D && D <= 16384 && Hp <= 16384,
             "st_fold: D, Hp and P3 must be positive multiples of 8, P3 <= D, at most 16384 (got D = %d, Hp = %d, P3 = %d)", D, Hp, P3);
  ST_REQUIRE(((uintptr_t)W1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)b2 | (uintptr_t)W3 | (uintptr_t)b3 | (uintptr_t)W1h | (uintptr_t)W1T | (uintptr_t)b1h |
              (uintptr_t)W2h | (uintptr_t)W2T | (uintptr_t)b2h | (uintptr_t)W3h | (uintptr_t)W3T | (uintptr_t)b3h) % 16 == 0, "st_fold: operands must be 16-byte aligned");
  StrFold a;
  a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3;
  a.W1h = (bf16*)W1h; a.W1T = (bf16*)W1T; a.b1h = (bf16*)b1h; a.W2h = (bf16*)W2h; a.W2T = (bf16*)W2T; a.b2h = (bf16*)b2h;
  a.W3h = (bf16*)W3h; a.W3T = (bf16*)W3T; a.b3h = (bf16*)b3h;
  a.D = D; a.Hp = Hp; a.P3 = P3;
  const int tcD = (D + FOLD_TILE - 1) / FOLD_TILE, tcH = (Hp + FOLD_TILE - 1) / FOLD_TILE, trP = (P3 + FOLD_TILE - 1) / FOLD_TILE;
  a.t1 = tcH * tcD; a.t2 = tcH * tcH; a.t3 = trP * tcH;
  const int vec_blocks = ((2 * Hp + P3) / 8 + STR_BLOCK - 1) / STR_BLOCK;
  const double el = (double)Hp * D + (double)Hp * Hp + (double)P3 * Hp;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, el, 8.0 * el);          // 4 bytes read, 2 x 2 written per element
  hipLaunchKernelGGL(k_str_fold, dim3(a.t1 + a.t2 + a.t3 + vec_blocks), dim3(STR_BLOCK), 0, (hipStream_t)stream, a);
  return st355_check_launch("st_fold");
}

// ---- the masked per-sample MSE ----
// A sample's S * Pc prediction elements are one flat run of n8 = S Pc / 8 16-byte chunks (Pc % 8 == 0: a chunk lies inside one token row).  Workgroup (b, k) of
// (B, nch) walks chunks k 256 + tid, (k + nch) 256 + tid, ...: a lane adds its squares in that order, butterfly per wave, the 4 waves in order -> ws[b nch + k].
// The mask of sample b is taken from sigma[b] here as in the final pass (the same fp32 comparison), so G needs no second pass over pred.
struct StrVae {                         // target [B, C, H, W]: element (b, c, y, x) at b * bstride + (c * H + y) * W + x
  const void* target;
  int target_bf16;
  int64_t bstride;
  int H, W, gw, ph, pw;
};
struct StrCfg {                         // c / u: [B, S, D] views (row stride ld, batch stride bstride, elements)
  const bf16 *c, *u;
  int64_t ld, bstride;
  float scale;
};

__device__ __forceinline__ bool str_active(const float* __restrict__ sigma, int b, float tmin, float tmax) {
  const float s = sigma[b];
  return s >= tmin && s <= tmax;
}

template <int CFG>
__global__ void __launch_bounds__(STR_BLOCK) k_str_loss(bf16* pred, StrVae va, StrCfg ca, const float* __restrict__ sigma, float tmin, float tmax,
                                                        float* __restrict__ partial, int Pc, int64_t n8, int nch) {
  __shared__ float part[STR_BLOCK / WAVE];
  const int b = blockIdx.x / nch, k = blockIdx.x % nch, lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  const bool on = str_active(sigma, b, tmin, tmax);
  bf16* pb = pred + (int64_t)b * n8 * 8;
  float acc = 0.f;
  for (int64_t q = (int64_t)k * STR_BLOCK + threadIdx.x; q < n8; q += (int64_t)nch * STR_BLOCK) {
    const int64_t e = q * 8;
    const int r = (int)(e / Pc), col = (int)(e % Pc);
    const bf16x8 p = *(const bf16x8*)(pb + e);
    float t[8];
    if (CFG) {
      const int64_t off = (int64_t)b * ca.bstride + (int64_t)r * ca.ld + col;
      float c[8], u[8];
      ld8(ca.c + off, c);
      ld8(ca.u + off, u);
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = fmaf(ca.scale, c[j] - u[j], u[j]);
    } else {
      const int i = r / va.gw, jx = r % va.gw, pp = va.ph * va.pw;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int cj = col + j, ch = cj / pp, ay = (cj % pp) / va.pw, ex = cj % va.pw;
        const int64_t off = (int64_t)b * va.bstride + ((int64_t)ch * va.H + (i * va.ph + ay)) * va.W + (jx * va.pw + ex);
        t[j] = va.target_bf16 ? bf2f(((const bf16*)va.target)[off]) : ((const float*)va.target)[off];
      }
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float d = bf2f(p[j]) - t[j];
      acc = fmaf(d, d, acc);
      o[j] = f2bf(on ? 2.f * d : 0.f);
    }
    *(bf16x8*)(pb + e) = o;
  }
  acc = wave_sum(acc);
  if (lane == 0) part[w] = acc;
  __syncthreads();
  // (pairwise, not block_reduce's wave order: this kernel's bits since its first release)
  if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one workgroup: thread b adds sample b's chunks in index order -> per_sample[b] = sum / (S Pc); then thread 0 walks the samples in order
__global__ void __launch_bounds__(STR_BLOCK) k_str_loss_final(const float* __restrict__ partial, const float* __restrict__ sigma, float tmin, float tmax, int B, int nch,
                                                              float inv_sp, float* __restrict__ per_sample, float* __restrict__ stats) {
  for (int b = threadIdx.x; b < B; b += STR_BLOCK) {
    float a = 0.f;
    for (int k = 0; k < nch; k++) a += partial[(int64_t)b * nch + k];
    per_sample[b] = a * inv_sp;
  }
  __syncthreads();                      // (per_sample is read back through global memory by thread 0 of the same workgroup)
  if (threadIdx.x == 0) {
    float a = 0.f;
    int n = 0;
    for (int b = 0; b < B; b++)
      if (str_active(sigma, b, tmin, tmax)) {
        a += per_sample[b];
        n++;
      }
    stats[0] = n ? a / (float)n : 0.f;
    stats[1] = (float)n;
    stats[2] = n ? inv_sp / (float)n : 0.f;
  }
}

static inline int str_chunks(int64_t n8) {
  const int64_t c = cdiv64(n8, STR_BLOCK);
  return (int)(c < STR_MAX_CHUNKS ? c : STR_MAX_CHUNKS);
}

extern "C" int64_t st355_st_loss_workspace(int B, int64_t per_sample_elems) {
  return B > 0 && per_sample_elems > 0 ? (int64_t)B * str_chunks(per_sample_elems / 8) * 4 : 0;
}

#define STR_REQUIRE_COMMON(name)                                                                                                                          \
  ST_REQUIRE(pred && sigma && per_sample && stats && ws && B > 0 && B <= STR_MAX_B && S > 0, name ": bad args (1 <= B <= %d)", STR_MAX_B);                \
  ST_REQUIRE(tmin <= tmax, name ": the timestep range must satisfy min <= max (got %g, %g)", (double)tmin, (double)tmax);                                \
  ST_REQUIRE((uintptr_t)pred % 16 == 0 && ((uintptr_t)ws | (uintptr_t)sigma | (uintptr_t)per_sample | (uintptr_t)stats) % 4 == 0,                         \
             name ": pred must be 16-byte aligned")

extern "C" int st355_st_vae_loss(void* stream, void* pred, const void* target, int target_bf16, int64_t target_bstride, const float* sigma, float tmin, float tmax, int B,
                                 int S, int C, int H, int W, int gh, int gw, float* per_sample, float* stats, void* ws) {
  STR_REQUIRE_COMMON("st_vae_loss");
  ST_REQUIRE(target && C > 0 && H > 0 && W > 0 && gh > 0 && gw > 0, "st_vae_loss: bad args");
  ST_REQUIRE((int64_t)gh * gw == S && H % gh == 0 && W % gw == 0, "st_vae_loss: the token grid %d x %d must hold S = %d tokens and divide the latent %d x %d", gh, gw, S, H, W);
  const int ph = H / gh, pw = W / gw, P = C * ph * pw;
  ST_REQUIRE(P % 8 == 0, "st_vae_loss: P = C ph pw must be a multiple of 8 (got %d)", P);
  ST_REQUIRE(target_bstride >= (int64_t)C * H * W, "st_vae_loss: the target's batch stride must be at least C H W");
  ST_REQUIRE((uintptr_t)target % (target_bf16 ? 2 : 4) == 0, "st_vae_loss: the target must be aligned to its element");
  const int64_t n8 = (int64_t)S * P / 8;
  const int nch = str_chunks(n8);
  StrVae va;
  va.target = target; va.target_bf16 = target_bf16; va.bstride = target_bstride; va.H = H; va.W = W; va.gw = gw; va.ph = ph; va.pw = pw;
  StrCfg ca = {};
  const double n = (double)B * S * P;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 5.0 * n, (4.0 + (target_bf16 ? 2.0 : 4.0)) * n);
  hipLaunchKernelGGL(k_str_loss<0>, dim3(B * nch), dim3(STR_BLOCK), 0, (hipStream_t)stream, (bf16*)pred, va, ca, sigma, tmin, tmax, (float*)ws, P, n8, nch);
  hipLaunchKernelGGL(k_str_loss_final, dim3(1), dim3(STR_BLOCK), 0, (hipStream_t)stream, (const float*)ws, sigma, tmin, tmax, B, nch,
                     (float)(1.0 / ((double)S * (double)P)), per_sample, stats);
  return st355_check_launch("st_vae_loss");
}

extern "C" int st355_st_cfg_loss(void* stream, void* pred, const void* cond, const void* uncond, int64_t ld, int64_t bstride, float cfg_scale, const float* sigma,
                                 float tmin, float tmax, int B, int S, int D, float* per_sample, float* stats, void* ws) {
  STR_REQUIRE_COMMON("st_cfg_loss");
  ST_REQUIRE(cond && uncond && D > 0 && D % 8 == 0, "st_cfg_loss: D must be a positive multiple of 8 (got %d)", D);
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && bstride >= 0, "st_cfg_loss: strides must be multiples of 8 elements, ld >= D");
  ST_REQUIRE(((uintptr_t)cond | (uintptr_t)uncond) % 16 == 0, "st_cfg_loss: the teacher rows must be 16-byte aligned");
  const int64_t n8 = (int64_t)S * D / 8;
  const int nch = str_chunks(n8);
  StrVae va = {};
  StrCfg ca;
  ca.c = (const bf16*)cond; ca.u = (const bf16*)uncond; ca.ld = ld; ca.bstride = bstride; ca.scale = cfg_scale;
  const double n = (double)B * S * D;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 7.0 * n, 8.0 * n);
  hipLaunchKernelGGL(k_str_loss<1>, dim3(B * nch), dim3(STR_BLOCK), 0, (hipStream_t)stream, (bf16*)pred, va, ca, sigma, tmin, tmax, (float*)ws, D, n8, nch);
  hipLaunchKernelGGL(k_str_loss_final, dim3(1), dim3(STR_BLOCK), 0, (hipStream_t)stream, (const float*)ws, sigma, tmin, tmax, B, nch,
                     (float)(1.0 / ((double)S * (double)D)), per_sample, stats);
  return st355_check_launch("st_cfg_loss");
}

// ---- weight gradients ----
// g_W = s P (8 elements per lane, the last workgroup ragged); the workgroups behind the matrix write g_b = s db, one element per lane
__global__ void __launch_bounds__(STR_BLOCK) k_str_wgrad(const bf16* __restrict__ P, const float* __restrict__ db, const float* __restrict__ scale, float* g_W, float* g_b,
                                                         int64_t n8, int mat_blocks, int R, int accumulate) {
  const float s = scale[0];
  if ((int)blockIdx.x >= mat_blocks) {
    const int r = ((int)blockIdx.x - mat_blocks) * STR_BLOCK + threadIdx.x;
    if (r < R) g_b[r] = accumulate ? g_b[r] + s * db[r] : s * db[r];
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * STR_BLOCK + threadIdx.x;
  if (i >= n8) return;
  float v[8], o[8];
  ld8(P + i * 8, v);
  if (accumulate) {
    ld8(g_W + i * 8, o);
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = fmaf(s, v[j], o[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = s * v[j];
  }
  *(float4*)(g_W + i * 8) = make_float4(o[0], o[1], o[2], o[3]);
  *(float4*)(g_W + i * 8 + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

extern "C" int st355_st_wgrad(void* stream, const void* P, const float* db, const float* scale_dev, float* g_W, float* g_b, int R, int Cc, int accumulate) {
  ST_REQUIRE(P && db && scale_dev && g_W && g_b, "st_wgrad: bad args");
  ST_REQUIRE(R > 0 && Cc > 0 && Cc % 8 == 0, "st_wgrad: expected R > 0 rows of Cc columns, Cc a multiple of 8 (got %d x %d)", R, Cc);
  ST_REQUIRE((uintptr_t)P % 16 == 0 && (uintptr_t)g_W % 16 == 0 && ((uintptr_t)db | (uintptr_t)g_b | (uintptr_t)scale_dev) % 4 == 0,
             "st_wgrad: P and g_W must be 16-byte aligned");
  const int64_t n8 = (int64_t)R * Cc / 8;
  ST_REQUIRE(cdiv64(n8, STR_BLOCK) + (R + STR_BLOCK - 1) / STR_BLOCK <= 0x7fffffff, "st_wgrad: too many elements");
  const int mat_blocks = (int)cdiv64(n8, STR_BLOCK), vec_blocks = (R + STR_BLOCK - 1) / STR_BLOCK;
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * R * Cc, (accumulate ? 10.0 : 6.0) * R * Cc);
  hipLaunchKernelGGL(k_str_wgrad, dim3(mat_blocks + vec_blocks), dim3(STR_BLOCK), 0, (hipStream_t)stream, (const bf16*)P, db, scale_dev, g_W, g_b, n8, mat_blocks, R,
                     accumulate);
  return st355_check_launch("st_wgrad");
}

// ---- dX into the strided view ----
__global__ void __launch_bounds__(STR_BLOCK) k_str_dx_add(const bf16* __restrict__ g, const float* __restrict__ scale, bf16* dx, int rows, int D, int64_t n8, int64_t ld,
                                                          int64_t bstride) {
  const int64_t q = (int64_t)blockIdx.x * STR_BLOCK + threadIdx.x;
  if (q >= n8) return;
  const int64_t e = q * 8, row = e / D;
  const int col = (int)(e % D);
  bf16* dp = dx + (row / rows) * bstride + (row % rows) * ld + col;
  const float s = scale[0];
  const bf16x8 a = *(const bf16x8*)(g + e), o = *(const bf16x8*)dp;
  bf16x8 w;
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = f2bf(fmaf(s, bf2f(a[j]), bf2f(o[j])));
  *(bf16x8*)dp = w;
}

extern "C" int st355_st_dx_add(void* stream, const void* g, const float* scale_dev, void* dx, int B, int rows, int D, int64_t ld, int64_t bstride) {
  ST_REQUIRE(g && scale_dev && dx && B > 0 && rows > 0, "st_dx_add: bad args");
  ST_REQUIRE(D > 0 && D % 8 == 0, "st_dx_add: D must be a positive multiple of 8 (got %d)", D);
  ST_REQUIRE(ld >= D && ld % 8 == 0 && bstride % 8 == 0 && (B == 1 || bstride >= (int64_t)rows * ld), "st_dx_add: strides must be multiples of 8 elements, ld >= D, samples apart");
  ST_REQUIRE(((uintptr_t)g | (uintptr_t)dx) % 16 == 0, "st_dx_add: operands must be 16-byte aligned");
  const int64_t n8 = (int64_t)B * rows * D / 8;
  ST_REQUIRE(cdiv64(n8, STR_BLOCK) <= 0x7fffffff, "st_dx_add: too many elements");
  ProfScope ps(stream, ST355_K_ELEMENTWISE, 2.0 * n8 * 8, 6.0 * n8 * 8);
  hipLaunchKernelGGL(k_str_dx_add, dim3((unsigned)cdiv64(n8, STR_BLOCK)), dim3(STR_BLOCK), 0, (hipStream_t)stream, (const bf16*)g, scale_dev, (bf16*)dx, rows, D, n8, ld,
                     bstride);
  return st355_check_launch("st_dx_add");
}

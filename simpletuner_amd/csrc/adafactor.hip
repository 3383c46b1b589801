// adafactor.hip — K16f: Adafactor (Shazeer & Stern 2018; the registry's "torch-adafactor" = torch.optim.Adafactor, _single_tensor_adafactor) over a flat
// parameter arena, driven by a device-resident plan with one record per parameter tensor.  Five launches per step whatever the number of tensors:
//   stats    reads g, p        per-tile partial row / column sums of g'^2 and one partial of sum p^2 per tile          (g' = grad_scale g)
//   factors  (small)           finishes the partials, lerps row_var / col_var, forms the clamped row-variance mean per (tensor, batch)
//   unorm    reads g           per-tile partials of sum u^2,  u = g' / sqrt(max(v, eps1^2)),  v = (row_var / max(mean(row_var), eps1)) col_var
//   coef     (small)           one workgroup per tensor finishes sum p^2 and sum u^2 into alpha / denom on the device: no host read
//   apply    reads g, p        p <- p (1 - lr wd) - (alpha / denom) u, written with ONE rounding into the arena dtype
// bf16 arena: 2 + 2, 2, 2 + 2 + 2 = 12 B/param (fp32 arena: 24), plus the partials (1 / 16 B/param).  State is sub-linear: R + C floats per matrix.
//
// Work items are (tensor, tile) pairs found by a binary search over the records' first-item fields.  A tensor is one of
//   VEC    1-D: `variance` like p; items of 1024 elements; its lerp happens in the stats pass (element-wise, no reduction)
//   MAT    [batch, R, C], factored over the last two dims: tiles of 64 rows x 256 columns, wave w owns 16 rows, lane l the four columns 4 l + k — one
//          8-byte (bf16) / 16-byte (fp32) access per row where C and the tensor's start are multiples of 4 elements, scalar accesses elsewhere
//   SMALL  batch > 1 matrices of at most 64 elements (conv kernels, the 2 x 2 patch embedding): ONE LANE owns one matrix and does its row / column
//          sums, both lerps and the row mean in the stats pass.  Correct, not tuned.
// Every reduction is fp32 in a fixed order (lane accumulators, xor butterfly, the waves in order, the tiles in a thread-strided order then the same
// block reduction): no floating-point atomics, bit-identical run to run.  Only elements inside a tensor are ever read or written: the pad elements
// between tensors take part in nothing.  tests/adafactor_bounds.py counts its roundings off the expressions below.
#include "optim_common.h"

#define AF_REC ST355_ADAFACTOR_PLAN_RECORD
#define AF_HDR ST355_ADAFACTOR_PLAN_HEADER
#define AF_TR 64
#define AF_TC 256
#define AF_VEC_ITEM 1024
#define AF_SMALL_MAX 64
enum { AF_VEC = 0, AF_MAT = 1, AF_SMALL = 2 };
// record fields
enum { F_OFF = 0, F_KIND, F_BATCH, F_R, F_C, F_NUMEL, F_RV, F_CV, F_VAR, F_TILE0, F_NTR, F_NTC, F_FACT0, F_ROWPART, F_COLPART, F_RMEAN };
// header fields
enum { H_N = 0, H_TILES, H_FACTS, H_RV, H_CV, H_VAR, H_WS, H_PPART };

struct AfC {
  float gs, omb2, eps1, eps1sq, eps2, rho, decay, d;   // decay = 1 - lr weight_decay (1 when weight_decay == 0)
};

// torch's lerp: a + w (b - a) below w = 0.5, b - (b - a)(1 - w) from there on (step 1 has w = 1: exactly b)
__device__ __forceinline__ float af_lerp(float a, float b, float w) {
  const float diff = b - a;
  return w < 0.5f ? a + w * diff : b - diff * (1.f - w);
}
// u = g' / sqrt(max(v, eps1^2)) with v_rsq_f32 (1 ulp): an IEEE square root and an IEEE quotient per element are ~40 VALU instructions, enough to make
// the unorm and apply passes VALU-bound on a bf16 arena.  For the same reason the quotient row_var / mean is formed once per row: v = (row_var / mean) col_var
__device__ __forceinline__ float af_u(float g, float v, const AfC& c) { return g * __builtin_amdgcn_rsqf(fmaxf(v, c.eps1sq)); }

// a lane's four consecutive elements from e on, `left` of them inside the row (<= 0: none); what lies outside reads as 0 and is never stored.
// vec: the row length and the tensor's start are multiples of 4 elements, so `left` is 0 or >= 4 and the access is naturally aligned
template <typename T> struct AfVec4;
template <> struct AfVec4<float> { typedef f32x4 type; };
template <> struct AfVec4<bf16> { typedef bf16x4 type; };
template <typename T>
__device__ __forceinline__ void af_load4(const T* x, int64_t e, int64_t left, bool vec, float (&o)[4]) {
  if (vec && left > 0) {
    const typename AfVec4<T>::type v = *(const typename AfVec4<T>::type*)(x + e);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (float)v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = k < left ? (float)x[e + k] : 0.f;
  }
}
template <typename T>
__device__ __forceinline__ void af_store4(T* x, int64_t e, int64_t left, bool vec, const float (&o)[4]) {
  if (vec && left > 0) {
    typename AfVec4<T>::type v;
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (T)o[k];
    *(typename AfVec4<T>::type*)(x + e) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < left) x[e + k] = (T)o[k];
  }
}
template <typename T>
__device__ __forceinline__ bool af_vec_ok(const T* p, const T* g, int64_t off, int64_t C) {
  return (C & 3) == 0 && ((uintptr_t)(p + off) % (4 * sizeof(T))) == 0 && ((uintptr_t)(g + off) % (4 * sizeof(T))) == 0;
}

// the record whose first item (field f) is the last one <= item
__device__ __forceinline__ const int64_t* af_find(const int64_t* plan, int64_t n, int64_t item, int f) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (plan[AF_HDR + mid * AF_REC + f] <= item) lo = mid; else hi = mid - 1;
  }
  return plan + AF_HDR + lo * AF_REC;
}

// total of v over the 256 threads, the same value in every thread; sh: 4 floats
__device__ __forceinline__ float af_block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return t;
}

// ---- stats -------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_af_stats(const int64_t* __restrict__ plan, const T* __restrict__ p, const T* __restrict__ g,
                                                  float* __restrict__ rv, float* __restrict__ cv, float* __restrict__ var, float* __restrict__ ws, AfC c) {
  __shared__ float cs_sh[4 * AF_TC];
  __shared__ float red[4];
  const int64_t n = plan[H_N], n_tiles = plan[H_TILES];
  float* ppart = ws + plan[H_PPART];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int64_t item = blockIdx.x; item < n_tiles; item += gridDim.x) {
    const int64_t* rec = af_find(plan, n, item, F_TILE0);
    const int64_t li = item - rec[F_TILE0], off = rec[F_OFF], R = rec[F_R], C = rec[F_C], batch = rec[F_BATCH];
    const int kind = (int)rec[F_KIND];
    float pp = 0.f;
    if (kind == AF_VEC) {
      for (int k = 0; k < AF_VEC_ITEM / 256; k++) {
        const int64_t e = li * AF_VEC_ITEM + tid + 256 * k;
        if (e < C) {
          const float gj = (float)g[off + e] * c.gs, pj = (float)p[off + e];
          float* vp = var + rec[F_VAR] + e;
          *vp = af_lerp(*vp, gj * gj, c.omb2);
          pp += pj * pj;
        }
      }
    } else if (kind == AF_SMALL) {
      const int64_t b = li * 256 + tid;
      if (b < batch) {
        const int64_t base = off + b * R * C;
        float* rvb = rv + rec[F_RV] + b * R;
        float* cvb = cv + rec[F_CV] + b * C;
        float rsum = 0.f;
        for (int64_t r = 0; r < R; r++) {
          float s = 0.f;
          for (int64_t cc = 0; cc < C; cc++) {
            const float gj = (float)g[base + r * C + cc] * c.gs, pj = (float)p[base + r * C + cc];
            s += gj * gj;
            pp += pj * pj;
          }
          const float nv = af_lerp(rvb[r], s / (float)C, c.omb2);
          rvb[r] = nv;
          rsum += nv;
        }
        for (int64_t cc = 0; cc < C; cc++) {
          float s = 0.f;
          for (int64_t r = 0; r < R; r++) {
            const float gj = (float)g[base + r * C + cc] * c.gs;
            s += gj * gj;
          }
          cvb[cc] = af_lerp(cvb[cc], s / (float)R, c.omb2);
        }
        ws[rec[F_RMEAN] + b] = fmaxf(rsum / (float)R, c.eps1);
      }
    } else {
      const int64_t ntr = rec[F_NTR], ntc = rec[F_NTC];
      const int64_t b = li / (ntr * ntc), rem = li - b * ntr * ntc, tr = rem / ntc, tc = rem - tr * ntc;
      const int64_t base = off + b * R * C, c0 = tc * AF_TC, r0 = tr * AF_TR + w * (AF_TR / 4);
      const int64_t cc = c0 + 4 * lane;
      const bool vec = af_vec_ok(p, g, off, C);
      float cs[4] = {0.f, 0.f, 0.f, 0.f};
      for (int i = 0; i < AF_TR / 4; i++) {
        const int64_t r = r0 + i;
        if (r >= R) break;                         // wave-uniform
        float gv[4], pv[4];
        af_load4(g, base + r * C + cc, C - cc, vec, gv);
        af_load4(p, base + r * C + cc, C - cc, vec, pv);
        float rs = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {              // (columns past C read as 0 and add exact zeros)
          const float gj = gv[k] * c.gs;
          const float g2 = gj * gj;
          rs += g2;
          cs[k] += g2;
          pp += pv[k] * pv[k];
        }
        rs = wave_sum(rs);
        if (lane == 0) ws[rec[F_ROWPART] + (b * R + r) * ntc + tc] = rs;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) cs_sh[w * AF_TC + 4 * lane + k] = cs[k];
      __syncthreads();
      if (c0 + tid < C)
        ws[rec[F_COLPART] + (b * ntr + tr) * C + c0 + tid] = ((cs_sh[tid] + cs_sh[AF_TC + tid]) + cs_sh[2 * AF_TC + tid]) + cs_sh[3 * AF_TC + tid];
    }
    const float tot = af_block_sum(pp, red);       // (also the barrier that frees cs_sh for the next item)
    if (tid == 0) ppart[item] = tot;
  }
}

// ---- factors (MAT tensors only): per (tensor, batch) one ROW item, then one COL item per 256 columns ----------------------------------------------
__global__ void __launch_bounds__(256) k_af_factors(const int64_t* __restrict__ plan, float* __restrict__ rv, float* __restrict__ cv,
                                                    float* __restrict__ ws, AfC c) {
  __shared__ float red[4];
  const int64_t n = plan[H_N], n_facts = plan[H_FACTS];
  const int tid = threadIdx.x;
  for (int64_t item = blockIdx.x; item < n_facts; item += gridDim.x) {
    const int64_t* rec = af_find(plan, n, item, F_FACT0);
    const int64_t li = item - rec[F_FACT0], R = rec[F_R], C = rec[F_C], ntr = rec[F_NTR], ntc = rec[F_NTC];
    const int64_t per_b = 1 + (C + 255) / 256, b = li / per_b, j = li - b * per_b;
    if (j == 0) {
      const float* part = ws + rec[F_ROWPART] + b * R * ntc;
      float* rvb = rv + rec[F_RV] + b * R;
      float acc = 0.f;
      for (int64_t r = tid; r < R; r += 256) {
        float s = 0.f;
        for (int64_t t = 0; t < ntc; t++) s += part[r * ntc + t];
        const float nv = af_lerp(rvb[r], s / (float)C, c.omb2);
        rvb[r] = nv;
        acc += nv;
      }
      const float tot = af_block_sum(acc, red);
      if (tid == 0) ws[rec[F_RMEAN] + b] = fmaxf(tot / (float)R, c.eps1);
    } else {
      const int64_t cc = (j - 1) * 256 + tid;
      if (cc < C) {
        const float* part = ws + rec[F_COLPART] + b * ntr * C + cc;
        float s = 0.f;
        for (int64_t t = 0; t < ntr; t++) s += part[t * C];
        float* cp = cv + rec[F_CV] + b * C + cc;
        *cp = af_lerp(*cp, s / (float)R, c.omb2);
      }
    }
  }
}

// ---- coef: one workgroup per tensor finishes sum p^2 and sum u^2 over the tensor's tiles (thread-strided, then the block reduction) into alpha / denom ----
__global__ void __launch_bounds__(256) k_af_coef(const int64_t* __restrict__ plan, float* __restrict__ ws, AfC c) {
  __shared__ float red[4];
  const int64_t n = plan[H_N], n_tiles = plan[H_TILES];
  const float* ppart = ws + plan[H_PPART];
  const float* upart = ppart + n_tiles;
  const int tid = threadIdx.x;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t* rec = plan + AF_HDR + i * AF_REC;
    const int64_t t0 = rec[F_TILE0], t1 = i + 1 < n ? rec[AF_REC + F_TILE0] : n_tiles;
    float sp = 0.f, su = 0.f;
    for (int64_t t = t0 + tid; t < t1; t += 256) { sp += ppart[t]; su += upart[t]; }
    sp = af_block_sum(sp, red);
    su = af_block_sum(su, red);
    const float rn = sqrtf((float)rec[F_NUMEL]);
    const float alpha = fmaxf(c.eps2, sqrtf(sp) / rn) * c.rho;
    const float denom = fmaxf(1.f, sqrtf(su) / (rn * c.d));
    if (tid == 0) ws[plan[H_PPART] + 2 * n_tiles + i] = alpha / denom;
  }
}

// ---- unorm (APPLY = false): partials of sum u^2;  apply (APPLY = true): p <- p decay - (alpha / denom) u -------------------------------------------
template <typename T, bool APPLY>
__global__ void __launch_bounds__(256) k_af_update(const int64_t* __restrict__ plan, T* __restrict__ p, const T* __restrict__ g,
                                                   const float* __restrict__ rv, const float* __restrict__ cv, const float* __restrict__ var,
                                                   float* __restrict__ ws, AfC c) {
  __shared__ float red[4];
  const int64_t n = plan[H_N], n_tiles = plan[H_TILES];
  float* upart = ws + plan[H_PPART] + n_tiles;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int64_t item = blockIdx.x; item < n_tiles; item += gridDim.x) {
    const int64_t* rec = af_find(plan, n, item, F_TILE0);
    const int64_t li = item - rec[F_TILE0], off = rec[F_OFF], R = rec[F_R], C = rec[F_C], batch = rec[F_BATCH];
    const int kind = (int)rec[F_KIND];
    const float coef = APPLY ? upart[n_tiles + (rec - plan - AF_HDR) / AF_REC] : 0.f;      // alpha / denom of the tile's tensor (k_af_coef)
    float uu = 0.f;
    if (kind == AF_VEC) {
      for (int k = 0; k < AF_VEC_ITEM / 256; k++) {
        const int64_t e = li * AF_VEC_ITEM + tid + 256 * k;
        if (e < C) {
          const float u = af_u((float)g[off + e] * c.gs, var[rec[F_VAR] + e], c);
          if (APPLY) p[off + e] = (T)((float)p[off + e] * c.decay - coef * u);
          else uu += u * u;
        }
      }
    } else if (kind == AF_SMALL) {
      const int64_t b = li * 256 + tid;
      if (b < batch) {
        const int64_t base = off + b * R * C;
        const float* rvb = rv + rec[F_RV] + b * R;
        const float* cvb = cv + rec[F_CV] + b * C;
        const float rm = ws[rec[F_RMEAN] + b];
        for (int64_t r = 0; r < R; r++) {
          const float rf = rvb[r] / rm;
          for (int64_t cc = 0; cc < C; cc++) {
            const int64_t e = base + r * C + cc;
            const float u = af_u((float)g[e] * c.gs, rf * cvb[cc], c);
            if (APPLY) p[e] = (T)((float)p[e] * c.decay - coef * u);
            else uu += u * u;
          }
        }
      }
    } else {
      const int64_t ntr = rec[F_NTR], ntc = rec[F_NTC];
      const int64_t b = li / (ntr * ntc), rem = li - b * ntr * ntc, tr = rem / ntc, tc = rem - tr * ntc;
      const int64_t base = off + b * R * C, c0 = tc * AF_TC, r0 = tr * AF_TR + w * (AF_TR / 4);
      const float* rvb = rv + rec[F_RV] + b * R;
      const float* cvb = cv + rec[F_CV] + b * C;
      const float rm = ws[rec[F_RMEAN] + b];
      const int64_t cc = c0 + 4 * lane;
      const bool vec = af_vec_ok((const T*)p, g, off, C);
      float cvk[4];
#pragma unroll
      for (int k = 0; k < 4; k++) cvk[k] = cc + k < C ? cvb[cc + k] : 0.f;
      for (int i = 0; i < AF_TR / 4; i++) {
        const int64_t r = r0 + i;
        if (r >= R) break;
        const float rf = rvb[r] / rm;
        const int64_t e = base + r * C + cc;
        float gv[4], pv[4];
        af_load4(g, e, C - cc, vec, gv);
        if (APPLY) af_load4((const T*)p, e, C - cc, vec, pv);
#pragma unroll
        for (int k = 0; k < 4; k++) {              // columns past C are neither summed nor stored: with eps1^2 = 0 (eps1 below 1e-19) their u is 0 * inf
          const float u = af_u(gv[k] * c.gs, rf * cvk[k], c);
          if (APPLY) pv[k] = pv[k] * c.decay - coef * u;
          else if (cc + k < C) uu += u * u;
        }
        if (APPLY) af_store4(p, e, C - cc, vec, pv);
      }
    }
    if (!APPLY) {
      const float tot = af_block_sum(uu, red);
      if (tid == 0) upart[item] = tot;
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------------
extern "C" int st355_adafactor_plan(const int64_t* offsets, const int64_t* batch, const int32_t* rows, const int32_t* cols, int n, int64_t* plan,
                                    int64_t* ws_floats) {
  ST_REQUIRE(offsets && batch && rows && cols && plan && ws_floats && n > 0, "adafactor_plan: bad args");
  int64_t tiles = 0, facts = 0, rvn = 0, cvn = 0, varn = 0, rowpart = 0, colpart = 0, rmean = 0, end = 0;
  for (int i = 0; i < n; i++) {
    int64_t* rec = plan + AF_HDR + (int64_t)i * AF_REC;
    const int64_t R = rows[i], C = cols[i], B = batch[i];
    ST_REQUIRE(R >= 0 && C > 0 && B > 0 && (R > 0 || B == 1), "adafactor_plan: tensor %d has batch %lld, rows %lld, cols %lld", i, (long long)B, (long long)R,
               (long long)C);
    ST_REQUIRE(offsets[i] >= end, "adafactor_plan: tensor %d overlaps its predecessor (offsets must ascend)", i);
    const int64_t numel = B * (R > 0 ? R : 1) * C;
    end = offsets[i] + numel;
    const int kind = R == 0 ? AF_VEC : (B > 1 && R * C <= AF_SMALL_MAX ? AF_SMALL : AF_MAT);
    rec[F_OFF] = offsets[i]; rec[F_KIND] = kind; rec[F_BATCH] = B; rec[F_R] = R; rec[F_C] = C; rec[F_NUMEL] = numel;
    rec[F_RV] = rvn; rec[F_CV] = cvn; rec[F_VAR] = varn; rec[F_TILE0] = tiles; rec[F_FACT0] = facts;
    rec[F_NTR] = rec[F_NTC] = 0; rec[F_ROWPART] = rec[F_COLPART] = rec[F_RMEAN] = 0;
    if (kind == AF_VEC) {
      varn += C;
      tiles += cdiv64(C, AF_VEC_ITEM);
    } else {
      rvn += B * R; cvn += B * C;
      rec[F_RMEAN] = rmean; rmean += B;
      if (kind == AF_SMALL) {
        tiles += cdiv64(B, 256);
      } else {
        const int64_t ntr = cdiv64(R, AF_TR), ntc = cdiv64(C, AF_TC);
        rec[F_NTR] = ntr; rec[F_NTC] = ntc;
        rec[F_ROWPART] = rowpart; rowpart += B * R * ntc;
        rec[F_COLPART] = colpart; colpart += B * ntr * C;
        tiles += B * ntr * ntc;
        facts += B * (1 + cdiv64(C, 256));
      }
    }
  }
  // workspace: row partials | column partials | clamped row means | sum p^2 partials | sum u^2 partials | alpha / denom per tensor
  for (int i = 0; i < n; i++) {
    int64_t* rec = plan + AF_HDR + (int64_t)i * AF_REC;
    rec[F_COLPART] += rowpart;
    rec[F_RMEAN] += rowpart + colpart;
  }
  plan[H_N] = n; plan[H_TILES] = tiles; plan[H_FACTS] = facts; plan[H_RV] = rvn; plan[H_CV] = cvn; plan[H_VAR] = varn;
  plan[H_PPART] = rowpart + colpart + rmean;
  plan[H_WS] = plan[H_PPART] + 2 * tiles + n;
  *ws_floats = plan[H_WS];
  return ST355_OK;
}

extern "C" int64_t st355_adafactor_workspace_floats(const int64_t* plan_host) { return plan_host ? plan_host[H_WS] : 0; }

static inline int af_blocks(int64_t items) { return (int)(items < 1 ? 1 : (items > (1 << 20) ? (1 << 20) : items)); }

template <typename T>
static int af_step(hipStream_t s, const int64_t* ph, const int64_t* pd, T* p, const T* g, float* rv, float* cv, float* var, float* ws, const AfC& c) {
  const int nb = af_blocks(ph[H_TILES]);
  hipLaunchKernelGGL(k_af_stats<T>, dim3(nb), dim3(256), 0, s, pd, (const T*)p, g, rv, cv, var, ws, c);
  if (ph[H_FACTS] > 0) hipLaunchKernelGGL(k_af_factors, dim3(af_blocks(ph[H_FACTS])), dim3(256), 0, s, pd, rv, cv, ws, c);
  hipLaunchKernelGGL((k_af_update<T, false>), dim3(nb), dim3(256), 0, s, pd, p, g, (const float*)rv, (const float*)cv, (const float*)var, ws, c);
  hipLaunchKernelGGL(k_af_coef, dim3(af_blocks(ph[H_N])), dim3(256), 0, s, pd, ws, c);
  hipLaunchKernelGGL((k_af_update<T, true>), dim3(nb), dim3(256), 0, s, pd, p, g, (const float*)rv, (const float*)cv, (const float*)var, ws, c);
  return st355_check_launch("adafactor_step");
}

extern "C" int st355_adafactor_step(void* stream, const int64_t* plan_host, const int64_t* plan_dev, void* p, const void* g, int elem_bytes, int64_t n_arena,
                                    float* row_var, float* col_var, float* variance, float* ws, int64_t ws_floats, float grad_scale, double one_minus_beta2,
                                    double rho, double eps1, double eps2, double d, double lr_weight_decay) {
  ST_REQUIRE(plan_host && plan_dev && p && g && ws, "adafactor_step: bad args");
  ST_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "adafactor_step: the arena is bf16 (2) or fp32 (4), got elem_bytes %d", elem_bytes);
  ST_REQUIRE(ws_floats >= plan_host[H_WS], "adafactor_step: workspace of %lld floats, the plan needs %lld", (long long)ws_floats, (long long)plan_host[H_WS]);
  ST_REQUIRE((plan_host[H_RV] == 0 || (row_var && col_var)) && (plan_host[H_VAR] == 0 || variance), "adafactor_step: a state buffer the plan needs is NULL");
  const int64_t* last = plan_host + AF_HDR + (plan_host[H_N] - 1) * AF_REC;
  ST_REQUIRE(last[F_OFF] + last[F_NUMEL] <= n_arena, "adafactor_step: the plan reaches element %lld of an arena of %lld", (long long)(last[F_OFF] + last[F_NUMEL]),
             (long long)n_arena);
  ST_REQUIRE(d >= 1.0 && eps1 >= 0.0 && eps2 >= 0.0, "adafactor_step: d >= 1, eps >= 0");
  AfC c;
  c.gs = grad_scale; c.omb2 = (float)one_minus_beta2; c.eps1 = (float)eps1; c.eps1sq = (float)(eps1 * eps1); c.eps2 = (float)eps2; c.rho = (float)rho;
  c.decay = (float)(1.0 - lr_weight_decay); c.d = (float)d;
  double numel = 0;
  for (int64_t i = 0; i < plan_host[H_N]; i++) numel += (double)plan_host[AF_HDR + i * AF_REC + F_NUMEL];
  ProfScope ps(stream, ST355_K_OPTIM, 12.0 * numel, 6.0 * elem_bytes * numel);
  if (elem_bytes == 2)
    return af_step<bf16>((hipStream_t)stream, plan_host, plan_dev, (bf16*)p, (const bf16*)g, row_var, col_var, variance, ws, c);
  return af_step<float>((hipStream_t)stream, plan_host, plan_dev, (float*)p, (const float*)g, row_var, col_var, variance, ws, c);
}

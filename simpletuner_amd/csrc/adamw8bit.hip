// adamw8bit.hip — K16e: AdamW with block-wise 8-bit moments (Dettmers et al. 2022, "8-bit Optimizers via Block-wise Quantization"; the registry's
// "ao-adamw8bit") over a flat fp32 or bf16 arena of many tensors, ONE launch per step whatever the number of tensors.
//
// State of a quantised tensor (numel >= 4096 and numel % 256 == 0): one code byte per element for m and one for v, one fp32 scale per 256-element
// block for each = 2.03 B / param.  Every other tensor ("plain") keeps fp32 m and v.  Traffic per element of a quantised block: p read + written,
// g read, two code bytes read + written = 16 B (fp32 arena) or 10 B (bf16 arena), against 28 / 22 B for st355_adamw_ema_step*.
//
// Work split.  A work item is a 256-element chunk of one segment of the host-built table: a whole quantisation block, or up to 256 elements of a
// plain tensor (only a tensor's last chunk is short).  One wave owns one item: 64 lanes x 4 elements, so both block maxima reduce inside the wave by
// cross-lane exchanges and no barrier is needed after the tables are in LDS.  A workgroup is 4 waves; waves walk the items grid-stride.  A wave
// finds its item's segment by binary search over the table's cumulative item counts and keeps the segment while its items stay inside it, so the
// search is paid once per segment, not once per item.
//
// Data movement.  With the chunk full and its first element a multiple of 4, lane l holds elements 4l .. 4l+3: p and g move as one 16-byte (fp32)
// or 8-byte (bf16) access, the codes as one 4-byte word, plain moments as 16 bytes.  Otherwise (a short last chunk, a tensor at an odd element
// offset) lane l holds elements l, l+64, l+128, l+192 with scalar, still coalesced, accesses.  Which elements a lane holds changes no result.
//
// Codebooks.  Four 256-entry fp32 tables are staged in LDS once per workgroup (4 KB): the signed and unsigned codebooks and, for each, its 255
// decision points (the midpoint of neighbours k and k+1 rounded toward -inf, so that `x > point` is exactly "x is nearer to k+1" for every fp32 x
// and an exact tie takes the lower index).  Dequantisation is one LDS read; quantisation is a branch-free binary search, 8 dependent LDS reads.
// The first three levels read one of at most 7 addresses (broadcast or near it); the data-dependent later levels conflict — measured in
// profiles/adamw8bit_kernel_stats.md.
//
// Per element, fp32, in this order (tests/adamw8bit_ref.py counts its roundings off it):
//   g' = g grad_scale ; p1 = p - (lr wd) p ; m' = m + (1 - b1)(g' - m) ; v' = v + (1 - b2)(g' g' - v)
//   p' = p1 - step_size (m' / (sqrtf(v') / bc2_sqrt + eps)),  step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t) from the host in double
// then per block s = max(max |x|, 1e-12), code = index of the codebook value nearest to x / s.  No atomics: two calls on equal inputs are bit-identical.
#include "optim_common.h"

#define A8_BLOCK 256            // elements per quantisation block = per work item
#define A8_WAVES 4
#define A8_REC ST355_ADAMW8BIT_RECORD

struct A8C {
  float lrwd, omb1, omb2, step_size, bc2_sqrt, eps, grad_scale;   // lrwd = lr * wd, omb = 1 - beta: formed in fp32
};

__device__ __forceinline__ void a8_one(float& p, float g, float& m, float& v, const A8C& c) {
  g *= c.grad_scale;
  p = p - c.lrwd * p;
  m = m + c.omb1 * (g - m);
  v = v + c.omb2 * (g * g - v);
  p = p - c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.eps));
}

// index of the codebook value nearest to x: pts[k] separates k from k + 1; 8 dependent LDS reads
__device__ __forceinline__ uint32_t a8_code(const float* pts, float x) {
  uint32_t idx = 0;
#pragma unroll
  for (int step = 128; step >= 1; step >>= 1) idx += (x > pts[idx + step - 1]) ? step : 0;
  return idx;
}

template <typename T> struct A8Vec;
template <> struct A8Vec<float> { typedef f32x4 type; };
template <> struct A8Vec<bf16> { typedef bf16x4 type; };

template <typename T>
__global__ void __launch_bounds__(A8_WAVES * 64) k_adamw8bit(T* __restrict__ p, const T* __restrict__ g, uint8_t* __restrict__ m_codes,
                                                            uint8_t* __restrict__ v_codes, float* __restrict__ m_scale, float* __restrict__ v_scale,
                                                            float* __restrict__ m_plain, float* __restrict__ v_plain,
                                                            const int64_t* __restrict__ table, int n_segs, int n_items,
                                                            const float* __restrict__ books, A8C c) {
  typedef typename A8Vec<T>::type VT;
  __shared__ float lds[4 * 256];       // signed codebook | unsigned codebook | signed decision points | unsigned decision points
  for (int i = threadIdx.x; i < 4 * 256; i += A8_WAVES * 64) lds[i] = books[i];
  __syncthreads();
  const float* cb_m = lds;
  const float* cb_v = lds + 256;
  const float* pt_m = lds + 512;
  const float* pt_v = lds + 768;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int seg = -1, seg_first = 0, seg_items = 0;          // the segment the wave is in (wave-uniform)
  int64_t s_start = 0, s_count = 0, s_kind = 0, s_code = 0, s_scale = 0, s_state = 0;
  for (int item = blockIdx.x * A8_WAVES + wave; item < n_items; item += gridDim.x * A8_WAVES) {
    if (item >= seg_first + seg_items) {                // items ascend: the next segment lies after the current one
      int lo = seg + 1, hi = n_segs - 1;                // last segment whose first item is <= item
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)table[(int64_t)mid * A8_REC + 6] <= item) lo = mid; else hi = mid - 1;
      }
      seg = lo;
      const int64_t* r = table + (int64_t)seg * A8_REC;
      s_start = r[0]; s_count = r[1]; s_kind = r[2]; s_code = r[3]; s_scale = r[4]; s_state = r[5];
      seg_first = (int)r[6]; seg_items = (int)r[7];
    }
    const int64_t chunk = item - seg_first;
    const int64_t base = s_start + chunk * A8_BLOCK;                       // first arena element of the item
    const int64_t left = s_count - chunk * A8_BLOCK;
    const int cnt = left < A8_BLOCK ? (int)left : A8_BLOCK;
    const bool vec = cnt == A8_BLOCK && (base & 3) == 0;
    const bool quant = s_kind == ST355_ADAMW8BIT_QUANT;                   // a quantised segment's chunks are always full

    float pv[4], gv[4], mv[4], vv[4];
    bool ok[4];
    if (vec) {
      const VT pl = *(const VT*)(p + base + 4 * lane), gl = *(const VT*)(g + base + 4 * lane);
#pragma unroll
      for (int j = 0; j < 4; j++) { pv[j] = (float)pl[j]; gv[j] = (float)gl[j]; ok[j] = true; }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int e = lane + 64 * j;
        ok[j] = e < cnt;
        pv[j] = ok[j] ? (float)p[base + e] : 0.f;
        gv[j] = ok[j] ? (float)g[base + e] : 0.f;
      }
    }
    if (quant) {
      const int64_t cbase = s_code + chunk * A8_BLOCK;
      const float sm = m_scale[s_scale + chunk], sv = v_scale[s_scale + chunk];
      uint32_t mc, vc;                                                   // the lane's four code bytes, element j in byte j
      if (vec) {
        mc = *(const uint32_t*)(m_codes + cbase + 4 * lane);
        vc = *(const uint32_t*)(v_codes + cbase + 4 * lane);
      } else {
        mc = vc = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          mc |= (uint32_t)m_codes[cbase + lane + 64 * j] << (8 * j);
          vc |= (uint32_t)v_codes[cbase + lane + 64 * j] << (8 * j);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        mv[j] = cb_m[(mc >> (8 * j)) & 255u] * sm;
        vv[j] = cb_v[(vc >> (8 * j)) & 255u] * sv;
      }
    } else {
      const int64_t sbase = s_state + chunk * A8_BLOCK;                  // s_state is a multiple of 4: 16-byte accesses on full chunks
      if (vec) {
        const f32x4 ml = *(const f32x4*)(m_plain + sbase + 4 * lane), vl = *(const f32x4*)(v_plain + sbase + 4 * lane);
#pragma unroll
        for (int j = 0; j < 4; j++) { mv[j] = ml[j]; vv[j] = vl[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          mv[j] = ok[j] ? m_plain[sbase + lane + 64 * j] : 0.f;
          vv[j] = ok[j] ? v_plain[sbase + lane + 64 * j] : 0.f;
        }
      }
    }

#pragma unroll
    for (int j = 0; j < 4; j++) a8_one(pv[j], gv[j], mv[j], vv[j], c);

    if (vec) {
      VT po;
#pragma unroll
      for (int j = 0; j < 4; j++) po[j] = (T)pv[j];
      *(VT*)(p + base + 4 * lane) = po;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (ok[j]) p[base + lane + 64 * j] = (T)pv[j];
    }

    if (quant) {
      const float am = wave_max(fmaxf(fmaxf(fabsf(mv[0]), fabsf(mv[1])), fmaxf(fabsf(mv[2]), fabsf(mv[3]))));
      const float av = wave_max(fmaxf(fmaxf(fabsf(vv[0]), fabsf(vv[1])), fmaxf(fabsf(vv[2]), fabsf(vv[3]))));
      const float sm = fmaxf(am, 1e-12f), sv = fmaxf(av, 1e-12f);
      uint32_t mc = 0, vc = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        mc |= a8_code(pt_m, mv[j] / sm) << (8 * j);
        vc |= a8_code(pt_v, vv[j] / sv) << (8 * j);
      }
      const int64_t cbase = s_code + chunk * A8_BLOCK;
      if (vec) {
        *(uint32_t*)(m_codes + cbase + 4 * lane) = mc;
        *(uint32_t*)(v_codes + cbase + 4 * lane) = vc;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          m_codes[cbase + lane + 64 * j] = (uint8_t)(mc >> (8 * j));
          v_codes[cbase + lane + 64 * j] = (uint8_t)(vc >> (8 * j));
        }
      }
      if (lane == 0) { m_scale[s_scale + chunk] = sm; v_scale[s_scale + chunk] = sv; }
    } else {
      const int64_t sbase = s_state + chunk * A8_BLOCK;
      if (vec) {
        f32x4 mo, vo;
#pragma unroll
        for (int j = 0; j < 4; j++) { mo[j] = mv[j]; vo[j] = vv[j]; }
        *(f32x4*)(m_plain + sbase + 4 * lane) = mo;
        *(f32x4*)(v_plain + sbase + 4 * lane) = vo;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (ok[j]) { m_plain[sbase + lane + 64 * j] = mv[j]; v_plain[sbase + lane + 64 * j] = vv[j]; }
      }
    }
  }
}

// every offset the kernel forms from the table, checked on the host copy before anything is launched
static int a8_check_table(const int64_t* t, int n_segs, int64_t n_items, int64_t n_arena, int64_t n_codes, int64_t n_scales, int64_t n_plain) {
  int64_t end = 0, items = 0;
  for (int i = 0; i < n_segs; i++) {
    const int64_t* r = t + (int64_t)i * A8_REC;
    const int64_t start = r[0], count = r[1], kind = r[2], code = r[3], scale = r[4], state = r[5], first = r[6], n = r[7];
    ST_REQUIRE(start >= end && count > 0 && count <= n_arena && start <= n_arena - count, "adamw8bit_step: segment %d [%lld, +%lld) leaves the arena of %lld or overlaps its predecessor",
               i, (long long)start, (long long)count, (long long)n_arena);
    ST_REQUIRE(first == items && n == cdiv64(count, A8_BLOCK), "adamw8bit_step: segment %d has a wrong work-item range", i);
    if (kind == ST355_ADAMW8BIT_QUANT) {
      ST_REQUIRE(count % A8_BLOCK == 0, "adamw8bit_step: quantised segment %d of %lld elements is not whole blocks of 256", i, (long long)count);
      ST_REQUIRE(code >= 0 && code % 4 == 0 && code <= n_codes - count, "adamw8bit_step: segment %d's codes leave the code buffers of %lld bytes", i, (long long)n_codes);
      ST_REQUIRE(scale >= 0 && scale <= n_scales - count / A8_BLOCK, "adamw8bit_step: segment %d's scales leave the scale buffers of %lld", i, (long long)n_scales);
    } else {
      ST_REQUIRE(kind == ST355_ADAMW8BIT_PLAIN, "adamw8bit_step: segment %d has kind %lld", i, (long long)kind);
      ST_REQUIRE(state >= 0 && state % 4 == 0 && state <= n_plain - count, "adamw8bit_step: segment %d's fp32 moments leave the buffers of %lld", i, (long long)n_plain);
    }
    end = start + count;
    items += n;
  }
  ST_REQUIRE(items == n_items, "adamw8bit_step: the table holds %lld work items, the call says %lld", (long long)items, (long long)n_items);
  return ST355_OK;
}

extern "C" int st355_adamw8bit_step(void* stream, void* p, const void* g, int elem_bytes, int64_t n_arena, uint8_t* m_codes, uint8_t* v_codes, int64_t n_codes,
                                    float* m_scale, float* v_scale, int64_t n_scales, float* m_plain, float* v_plain, int64_t n_plain,
                                    const int64_t* table_host, const int64_t* table_dev, int n_segs, int64_t n_items, const float* books,
                                    float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale) {
  ST_REQUIRE(p && g && table_host && table_dev && books && n_arena > 0 && n_segs > 0 && step >= 1, "adamw8bit_step: bad args");
  ST_REQUIRE(elem_bytes == 4 || (elem_bytes == 2 && n_arena % 8 == 0), "adamw8bit_step: the arena is fp32 (elem_bytes 4) or bf16 (elem_bytes 2, n a multiple of 8)");
  ST_REQUIRE(n_items > 0 && n_items < (int64_t)1 << 31, "adamw8bit_step: %lld work items", (long long)n_items);
  ST_REQUIRE(n_codes >= 0 && n_scales >= 0 && n_plain >= 0 && (n_codes == 0 || (m_codes && v_codes && m_scale && v_scale)) && (n_plain == 0 || (m_plain && v_plain)),
             "adamw8bit_step: a state buffer is missing");
  ST_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m_codes % 4 == 0) && ((uintptr_t)v_codes % 4 == 0) && ((uintptr_t)m_plain % 16 == 0) &&
             ((uintptr_t)v_plain % 16 == 0) && ((uintptr_t)books % 4 == 0), "adamw8bit_step: the arena and the fp32 moments must be 16-byte aligned, the codes 4-byte aligned");
  if (int rc = a8_check_table(table_host, n_segs, n_items, n_arena, n_codes, n_scales, n_plain)) return rc;
  A8C c;
  c.lrwd = lr * weight_decay; c.omb1 = 1.f - beta1; c.omb2 = 1.f - beta2; c.eps = eps; c.grad_scale = grad_scale;
  c.step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
  c.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  ProfScope ps(stream, ST355_K_OPTIM, 30.0 * n_arena, (3.0 * elem_bytes + 4.0) * n_arena);
  int64_t blocks = cdiv64(n_items, A8_WAVES);
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(k_adamw8bit<float>, dim3((int)blocks), dim3(A8_WAVES * 64), 0, (hipStream_t)stream, (float*)p, (const float*)g, m_codes, v_codes, m_scale,
                       v_scale, m_plain, v_plain, table_dev, n_segs, (int)n_items, books, c);
  else
    hipLaunchKernelGGL(k_adamw8bit<bf16>, dim3((int)blocks), dim3(A8_WAVES * 64), 0, (hipStream_t)stream, (bf16*)p, (const bf16*)g, m_codes, v_codes, m_scale,
                       v_scale, m_plain, v_plain, table_dev, n_segs, (int)n_items, books, c);
  return st355_check_launch("adamw8bit_step");
}

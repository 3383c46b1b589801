// norm_route.h — every instance decision of the normalisation / token-sum launchers (norm_rope.hip, stats.hip, groupnorm.hip).  The launchers and
// st355_norm_plan (norm_rope.hip) call these same helpers, so the plan reports what a launch would run without launching anything.  Host code only.
#pragma once
#include <stdint.h>

// LayerNorm (+ modulation) forward / backward, k_ln_mod_fwd<NC> / k_ln_mod_bwd<NC>: NC 16-byte chunks per lane, one wave per row
static inline int ln_route_nc(int D) { return D <= 512 ? 1 : D <= 1024 ? 2 : D <= 1536 ? 3 : D <= 2048 ? 4 : D <= 3072 ? 6 : 8; }
// k_ln_param_partials<NC> (D <= 2048)
static inline int lnp_route_nc(int D) { return D <= 512 ? 1 : D <= 1024 ? 2 : D <= 1536 ? 3 : 4; }
// k_ln_mod_bwd_stats<NC, GS> (D <= 3072)
static inline int ln_stats_route_nc(int D) { return D <= 512 ? 1 : D <= 1024 ? 2 : D <= 1536 ? 3 : D <= 2048 ? 4 : 6; }
// stats.hip: workgroups of 64 rows of one batch element per batch element
static inline int stats_route_chunks(int64_t rows_per_batch) { return (int)((rows_per_batch + 63) / 64); }

// GroupNorm: nch chunks of rows_per_chunk grid rows per image (stats and row-walking apply passes share them)
static inline int gn_route_chunks(int B, int H, int W, int* rows_per_chunk) {
  const int rows_img = (H + 2) * (W + 2);
  int nch = (768 + B - 1) / B;
  if (nch > (rows_img + 31) / 32) nch = (rows_img + 31) / 32;
  if (nch < 1) nch = 1;
  *rows_per_chunk = (rows_img + nch - 1) / nch;
  return (rows_img + *rows_per_chunk - 1) / *rows_per_chunk;
}
// launch geometry of the row-walking passes: channel windows of <= 256 chunks of equal width, RT rows per pass
static inline void gn_route_rows_geom(int C, int* nwin, int* cw, int* RT) {
  const int c8 = C / 8;
  *nwin = (c8 + 255) / 256;
  *cw = (c8 + *nwin - 1) / *nwin;
  *RT = 256 / *cw;
  if (*RT < 1) *RT = 1;
}

// q / k norm-weight gradient: two-level fixed-order reduction of the nblk per-workgroup partials, ns slices of `per` partials per weight
static inline void qk_wgrad_route_slices(int nblk, int* ns, int* per) {
  *ns = nblk < 64 * 32 ? (nblk + 31) / 32 : 64;
  *per = (nblk + *ns - 1) / *ns;
}

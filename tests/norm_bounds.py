"""Element-wise error bounds for the normalisation family (norm_rope.hip K5 / K6, groupnorm.hip) and the token-axis sums that feed it parameter gradients
(norm_rope.hip layernorm_param_grads, stats.hip, reduce.hip colsum_prod), against an fp64 reference of the SAME bf16 inputs (and the same fp32 cos / sin tables).

Where the bound comes from.  Every input is bf16, exact in fp64.  The kernels compute in fp32 with u = 2^-24 per rounding, and round each stored bf16 output
once (RNE, f2bf).  Their only long computations are sums, and a sum taken along a tree whose longest chain has L additions is off by at most L u sum|terms|.
L is read off the kernel's actual tree, never the total count:
    LayerNorm statistics (k_ln_mod_*, k_ln_param_partials, k_ln_mod_bwd_stats): 8 NC values per lane, then wave_sum (6)        L = 8 NC + 6
    layernorm_param_grads: ceil(rows / 512) rows per wave, then 512 partials as 8 slices of 64 and the 8 slices                L = ceil(rows/512) + 64 + 8
    stats.hip / colsum_prod: 16 rows per wave, the 4 waves in 2 levels, then ceil(chunks / 8) per slice and the 8 slices       L = 16 + 2 + ceil(c/8) + 8
    GroupNorm: a thread's chain over ceil(rows_per_chunk / RT) rows, the LDS combine over RT, then ceil(nch cg / 64) per lane
               in finalize and wave_sum (6); the parameter sums add ceil(B nch / 8) + 8 instead of the finalize
    q / k RMSNorm: 8 channels per thread + log2(HD / 8) shuffles; the norm-weight gradient 64 / TOK_PER_PASS tokens per thread,
               the TOK_PER_PASS LDS rows, ceil(per / 4) + 3 in a slice, ceil(ns / 4) + 3 in the final kernel
(1 billion terms summed in one chain would bound nothing; the trees above keep L in the hundreds even for a 1024^2 VAE GroupNorm.)
Each statistic's error is carried through the output expression in fp64, with a few u for the fp32 operations that follow (rsqrtf: 4 u; __expf in SiLU:
2^-21 (2 + |z|) relative), and the output gets one RNE rounding on top:

    tol = 1/2 ulp_bf16(|ref| + e) + e

Mean and variance.  The mean's error is L u sum|x| / n (+ the division).  A variance taken from sum (x - m)^2 (two passes, or one pass over values shifted by a
pivot that is one of the group's own values) is off by at most L u sum (x - p)^2 <= L u (2 sum (x - mean)^2 + 2 n max (x - mean)^2) plus n dmean^2: relative to
the variance this does not grow with mean / std.  No bound here is widened by (mean / std)^2: the one-pass sum x^2 / n - mean^2 needs that and is an error.

Cancelling backward terms.  dx = r (g - mean g - x_hat mean(g x_hat)) cancels; the rounding terms are scaled by |g| + |mean g| + |x_hat mean(g x_hat)|, not by
|dx|.  Chained outputs are checked against fp64 of the kernel's own stored values: dxg = gate * dx from dx as stored, d gate from dx as stored, d bias from dxg
as stored, the GroupNorm backward from the statistics the forward stored, qk_rope_norm_bwd from the roped bf16 Q / K and the fp32 1 / rms of the projection.

Coherent errors.  A wrong mean or rstd moves a whole row (or GroupNorm (image, group)) by an amount each element may hide under its bound.  fit_rows() fits each
row's error by weighted least squares onto two columns, the derivative of the output with respect to the mean (for y = x_hat a + b: a r, an offset) and with
respect to log rstd (ref - b, a slope).  The noise of a correctly rounded row is one RNE rounding per distinct output value, RMS ulp / sqrt(12), independent
(equal outputs share their rounding, so each distinct value counts once); from it the fit's standard error follows for that row's length and values.  A coefficient may exceed the fp32 statistics bound above by at most Z_LIMIT = 6 standard errors (a
correct row passes with probability 1 - 2e-9).  A rstd off by 2^-7 on a 1024-wide row is ~200 standard errors.

The parameter-gradient sums are fp32 outputs (no output rounding to count in ulps): besides the per-element bound, each block of 64 columns (x 64 batch rows)
keeps RMS(min(err / e, 4)) <= 0.5 — the random-walk fp32 error of a correct sum is far below its worst case.  bf16 sums (d bias into a bf16 row, the q / k norm
weight gradient) use the GEMM checker's 64 x 64 block RMS limit of 0.5 ulp (tests/gemm_bounds.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from tests import gemm_bounds as GB

F64 = torch.float64
U = 2.0 ** -24
U_RSQ = 4 * U
Z_LIMIT = 6.0
SUM_RMS_LIMIT = 0.5

ulp_bf16 = GB.ulp_bf16
rel_l2 = GB.rel_l2


def cdiv(a, b):
    return -(-int(a) // int(b))


# ---- reduction-tree chain lengths (the kernels' trees; see the module docstring) ----------------------------------------------------------------------
def L_ln(nc):
    return 8 * nc + 6


def L_ln_params(rows):
    return cdiv(rows, 512) + 64 + 8


def L_stats(chunks):
    """stats.hip / reduce.hip: chunks = the number of 64-row partial rows summed by the finalize kernel into one output"""
    return 16 + 2 + cdiv(chunks, 8) + 8


def L_gn(rows_per_chunk, RT, nch, cg):
    return cdiv(rows_per_chunk, RT) + RT + cdiv(nch * cg, 64) + 6


def L_gn_params(rows_per_chunk, RT, nch, B):
    return cdiv(rows_per_chunk, RT) + RT + cdiv(B * nch, 8) + 8


def gn_stats_RT(C):
    """k_gn_stats: RT rows per pass of the channel window holding the most channels (windows of <= 256 8-channel chunks)"""
    c8 = C // 8
    return 256 // min(c8, 256)


def L_qk(hd):
    return 8 + int(math.log2(hd // 8))


def L_qk_wgrad(hd, ns, per):
    tok = 256 // (hd // 8)
    return 64 // tok + tok + cdiv(per, 4) + 3 + cdiv(ns, 4) + 3


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Stats:
    mu: torch.Tensor       # [G] fp64 mean of each normalised row / group
    r: torch.Tensor        # [G] fp64 rstd = 1 / sqrt(var + eps)
    e_mu: torch.Tensor     # [G] bound on |mean_fp32 - mu|
    e_r: torch.Tensor      # [G] bound on |rstd_fp32 / r - 1|


def ln_stats(x, eps, L, pivoted=False):
    """x: [G, n] fp64 (each row one normalisation group).  The error bound of the fp32 mean / rstd of a two-pass kernel (pivoted=False) or of shifted sums
    about a pivot taken from the group's own values (pivoted=True: GroupNorm's one pass)."""
    n = x.shape[1]
    mu = x.mean(1)
    d = x - mu[:, None]
    m2 = (d * d).sum(1)
    var = m2 / n
    r = 1.0 / torch.sqrt(var + eps)
    if pivoted:
        mx = d.abs().amax(1)
        e_mu = (L + 2) * U * (d.abs().sum(1) / n + 3 * mx) + 2 * U * mu.abs()
        mag2 = 2 * m2 + 2 * n * mx * mx
    else:
        e_mu = (L + 1) * U * x.abs().sum(1) / n + U * mu.abs()
        mag2 = m2
    e_m2 = (L + 4) * U * mag2 + n * e_mu * e_mu
    e_var = e_m2 / n + U * var
    e_r = 0.5 * (e_var + U * (var + eps)) / (var + eps) + U_RSQ
    return Stats(mu, r, e_mu, e_r)


def norm_fwd(x, st, a, b, silu=False):
    """y = x_hat a + b [-> SiLU], x_hat = (x - mean) rstd.  x [G, n]; a / b broadcastable to [G, n] (fp64).  Returns (want, e, dmu, dlr): the derivatives of
    the output with respect to the mean (per unit) and to log rstd, for fit_rows."""
    r, mu = st.r[:, None], st.mu[:, None]
    t = (x - mu) * r
    e_t = r * st.e_mu[:, None] + t.abs() * (st.e_r[:, None] + 3 * U)
    z = t * a + b
    e_z = a.abs() * (e_t + U * t.abs()) + 2 * U * ((t * a).abs() + b.abs())
    dmu, dlr = -a * r, t * a
    if not silu:
        return z, e_z, dmu, dlr
    s = torch.sigmoid(z)
    y = z * s
    dy = s * (1 + z * (1 - s))
    e = dy.abs() * e_z + y.abs() * (2.0 ** -21 * (2 + z.abs()) + 3 * U)
    return y, e, dmu * dy, dlr * dy


def ln_bwd(dy, x, a, st, L, dres=None):
    """dx = r (g - mean g - x_hat mean(g x_hat)) [+ dres], g = dy a.  x, dy: [R, D]; a broadcastable.  Returns (want, e)."""
    D = x.shape[1]
    r, mu = st.r[:, None], st.mu[:, None]
    xh = (x - mu) * r
    e_xh = r * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * U)
    g = dy * a
    e_g = U * g.abs() + dy.abs() * U * a.abs()
    c1 = g.mean(1, keepdim=True)
    c2 = (g * xh).mean(1, keepdim=True)
    e_c1 = ((L + 2) * U * g.abs().sum(1, keepdim=True) + e_g.sum(1, keepdim=True)) / D
    e_c2 = ((L + 3) * U * (g * xh).abs().sum(1, keepdim=True) + (g.abs() * e_xh + e_g * xh.abs()).sum(1, keepdim=True)) / D
    inner = g - c1 - xh * c2
    mag = g.abs() + c1.abs() + (xh * c2).abs()
    want = r * inner
    e = r * (e_g + e_c1 + e_xh * c2.abs() + xh.abs() * e_c2 + 4 * U * mag) + (r * inner).abs() * st.e_r[:, None] + U * want.abs()
    if dres is not None:
        want = want + dres
        e = e + U * want.abs()
    return want, e


def mul_stored(a, b):
    """an output the kernel computes as one fp32 product of two exact values (dxg = dx_stored * gate, scale_cols' a * gate): want, e"""
    w = a * b
    return w, U * w.abs()


def colsum(t, L, e_t=None):
    """sum over dim -2 of terms t [..., rows, N] (fp64) in a tree of chain L: (want, e); e_t: per-term errors (of a fp32 product: pass U |t|)"""
    w = t.sum(-2)
    e = L * U * t.abs().sum(-2)
    if e_t is not None:
        e = e + e_t.sum(-2)
    return w, e


def rope_pairs(v, cs, sn):
    """out0 = v0 c0 - v1 s0 ; out1 = v1 c1 + v0 s1 on interleaved pairs (k_qk_norm_rope_fwd); v [..., HD], cs / sn broadcastable; returns (out, |terms|)"""
    v0, v1 = v[..., 0::2], v[..., 1::2]
    c0, c1, s0, s1 = cs[..., 0::2], cs[..., 1::2], sn[..., 0::2], sn[..., 1::2]
    o = torch.stack([v0 * c0 - v1 * s0, v1 * c1 + v0 * s1], -1).flatten(-2)
    m = torch.stack([(v0 * c0).abs() + (v1 * s0).abs(), (v1 * c1).abs() + (v0 * s1).abs()], -1).flatten(-2)
    return o, m


def rope_pairs_t(g, cs, sn):
    """the transpose of rope_pairs: d0 = g0 c0 + g1 s1 ; d1 = g1 c1 - g0 s0"""
    g0, g1 = g[..., 0::2], g[..., 1::2]
    c0, c1, s0, s1 = cs[..., 0::2], cs[..., 1::2], sn[..., 0::2], sn[..., 1::2]
    o = torch.stack([g0 * c0 + g1 * s1, g1 * c1 - g0 * s0], -1).flatten(-2)
    m = torch.stack([(g0 * c0).abs() + (g1 * s1).abs(), (g1 * c1).abs() + (g0 * s0).abs()], -1).flatten(-2)
    return o, m


def rms_stats(x, eps, hd):
    """x [..., HD] fp64: r = rsqrt(mean x^2 + eps) and its relative error bound"""
    ms = (x * x).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(ms + eps)
    e_r = 0.5 * ((L_qk(hd) + 3) * U * ms) / (ms + eps) + U_RSQ
    return r, e_r


def qk_fwd(x, w, cs, sn, eps):
    """RMSNorm (w: [HD] or None: no norm) + RoPE of x [..., HD].  Returns (want, e, dlr) (dlr: derivative with respect to log rstd)"""
    hd = x.shape[-1]
    if w is None:
        o, m = rope_pairs(x, cs, sn)
        return o, 3 * U * m, torch.zeros_like(o)
    r, e_r = rms_stats(x, eps, hd)
    y = x * r * w
    o, m = rope_pairs(y, cs, sn)
    return o, m * (e_r + 5 * U), o


def qk_bwd(g, x, w, cs, sn, eps):
    """k_qk_norm_rope_bwd: dy = R^T g; dx = r w dy - x r^3 mean(x w dy) (no norm: dx = dy).  Returns (want, e, dy, e_dy, r, e_r)"""
    hd = x.shape[-1]
    dy, m_dy = rope_pairs_t(g, cs, sn)
    e_dy = 2 * U * m_dy
    if w is None:
        return dy, e_dy + U * dy.abs(), dy, e_dy, None, None
    r, e_r = rms_stats(x, eps, hd)
    t = x * w * dy
    m = t.mean(-1, keepdim=True)
    e_m = ((L_qk(hd) + 3) * U * t.abs().sum(-1, keepdim=True) + (x * w).abs().mul(e_dy).sum(-1, keepdim=True)) / hd
    a1, a2 = r * w * dy, x * r ** 3 * m
    want = a1 - a2
    e = r * w.abs() * e_dy + a1.abs() * (e_r + 3 * U) + x.abs() * r ** 3 * e_m + a2.abs() * (3 * e_r + 4 * U) + U * want.abs()
    return want, e, dy, e_dy, r, e_r


def qk_rope_norm_bwd(g, z, rr, w, cs, sn):
    """k_qk_rope_norm_bwd_z: y = R^T z, dy = R^T g, dx = r (w dy - y / w mean(dy y)) from the stored roped z and 1 / rms r (chained).  (want, e)"""
    hd = z.shape[-1]
    dy, m_dy = rope_pairs_t(g, cs, sn)
    y, m_y = rope_pairs_t(z, cs, sn)
    if w is None:
        return dy, 2 * U * m_dy + U * dy.abs()
    e_dy, e_y = 2 * U * m_dy, 2 * U * m_y
    t = dy * y
    m = t.mean(-1, keepdim=True)
    e_m = ((L_qk(hd) + 3) * U * t.abs().sum(-1, keepdim=True) + (dy.abs() * e_y + y.abs() * e_dy).sum(-1, keepdim=True)) / hd
    a1, a2 = w * dy, y / w * m
    want = rr * (a1 - a2)
    e = rr * (w.abs() * e_dy + (e_y / w.abs()) * m.abs() + (y / w).abs() * e_m + 4 * U * (a1.abs() + a2.abs())) + U * want.abs()
    return want, e


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------------------
def check(name, out, want, e, blocks=True, verbose=True):
    """a bf16 output: per element tol = 1/2 ulp(|want| + e) + e, and the 64 x 64 block RMS <= 0.5 ulp (gemm_bounds.check).  blocks=False: no block limit —
    for outputs whose elements share their roundings (a GroupNorm group at mean / std = 256 has a handful of distinct input values; fit_rows, which counts
    each distinct value once, holds those) and for short vectors of independent sums (the q / k norm-weight gradient)"""
    o = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    rep = GB.check(name, o, want.reshape(o.shape).to(F64), e.reshape(o.shape).to(F64), verbose=blocks and verbose)
    if not blocks:
        rep.block_rms = 0.0
        if verbose:
            print(f"[bound] {name}: worst err/tol={rep.worst:.3f} at {rep.worst_at}; {rep.n} outputs")
    return rep


@dataclass
class SumReport:
    name: str
    worst: float
    worst_at: tuple
    block_rms: float
    n: int

    @property
    def ok(self):
        return self.worst <= 1.0 and self.block_rms <= SUM_RMS_LIMIT

    def line(self):
        return (f"[bound] {self.name}: worst err/tol={self.worst:.3f} at {self.worst_at}; worst 64-column block RMS(err/e)={self.block_rms:.3f} "
                f"(limit {SUM_RMS_LIMIT}); {self.n} outputs")


def check_f32(name, out, want, e, verbose=True):
    """an fp32 sum [N] or [nb, N]: |out - want| <= e + u |want| element-wise, and RMS(min(err / e, 4)) <= 0.5 over blocks of 64 columns x 64 rows"""
    o = out.to(F64).reshape(-1, out.shape[-1])
    w, ee = want.to(F64).reshape(o.shape), e.to(F64).reshape(o.shape)
    err = (o - w).abs()
    tol = ee + U * w.abs() + 1e-300
    ratio = torch.where(torch.isfinite(o), err / tol, torch.full_like(err, math.inf))
    flat = int(torch.argmax(ratio))
    worst = float(ratio.view(-1)[flat])
    R, Cn = o.shape
    q = (err / tol).clamp(max=4.0).nan_to_num(4.0)
    rb, cb = cdiv(R, 64), cdiv(Cn, 64)
    up = torch.zeros(rb * 64, cb * 64, dtype=F64, device=o.device)
    cnt = torch.zeros_like(up)
    up[:R, :Cn] = q * q
    cnt[:R, :Cn] = 1
    ms = up.view(rb, 64, cb, 64).sum((1, 3)) / cnt.view(rb, 64, cb, 64).sum((1, 3)).clamp_min(1)
    rep = SumReport(name, worst, divmod(flat, Cn), math.sqrt(float(ms.max())), R * Cn)
    if verbose:
        print(rep.line())
    return rep


@dataclass
class FitReport:
    name: str
    offset: float          # worst (|offset coefficient| - its fp32 allowance) / standard error over the rows
    offset_at: int
    slope: float           # the same for the log-rstd coefficient
    slope_at: int
    rows: int

    @property
    def ok(self):
        return self.offset <= Z_LIMIT and self.slope <= Z_LIMIT

    def line(self):
        return (f"[fit] {self.name}: worst row offset {self.offset:.2f} SE at row {self.offset_at}, slope {self.slope:.2f} SE at row {self.slope_at} "
                f"(limit {Z_LIMIT}); {self.rows} rows")


def fit_rows(name, out, want, e, dmu, dlr, e_mu, e_r, verbose=True):
    """out / want / e / dmu / dlr: [G, n] (one normalised row or GroupNorm (image, group) per row, fp64-able); e_mu / e_r: [G] the fp32 statistics bounds.
    Weighted least squares of (out - want) onto [dmu, dlr] with per-element noise sigma = ulp(|want| + e) / sqrt(12) + e_elem, where e_elem is e minus the
    statistics' share (kept in sigma so a near-zero output's fp32 error is noise, not signal)."""
    o, w = out.to(F64), want.to(F64)
    d = torch.where(torch.isfinite(o), o - w, torch.full_like(w, 1e30))
    sig = ulp_bf16(w.abs() + e) / math.sqrt(12.0) + (e - dmu.abs() * e_mu[:, None] - dlr.abs() * e_r[:, None]).clamp_min(0)
    # elements with the same exact output (a heavily quantised input: bf16 values at mean / std = 64 take a dozen values) share ONE rounding error: each
    # distinct value of a row counts once, or their common error would pass for coherent
    srt, idx = torch.sort(w, dim=1)
    first = torch.ones_like(srt, dtype=torch.bool)
    first[:, 1:] = srt[:, 1:] != srt[:, :-1]
    once = torch.zeros_like(first).scatter_(1, idx, first)
    wt = once.to(F64) / (sig * sig)
    X1, X2 = dmu.to(F64), dlr.to(F64)
    a11, a12, a22 = (wt * X1 * X1).sum(1), (wt * X1 * X2).sum(1), (wt * X2 * X2).sum(1)
    b1, b2 = (wt * X1 * d).sum(1), (wt * X2 * d).sum(1)
    det = a11 * a22 - a12 * a12
    live1, live2 = a11 > 0, a22 > 0
    both = live1 & live2 & (det > 1e-12 * a11 * a22)
    c1 = torch.where(both, (a22 * b1 - a12 * b2) / det.clamp_min(1e-300), b1 / a11.clamp_min(1e-300))
    c2 = torch.where(both, (a11 * b2 - a12 * b1) / det.clamp_min(1e-300), b2 / a22.clamp_min(1e-300))
    se1 = torch.where(both, torch.sqrt(a22 / det.clamp_min(1e-300)), 1.0 / torch.sqrt(a11.clamp_min(1e-300)))
    se2 = torch.where(both, torch.sqrt(a11 / det.clamp_min(1e-300)), 1.0 / torch.sqrt(a22.clamp_min(1e-300)))
    z1 = torch.where(live1, ((c1.abs() - e_mu) / se1).clamp_min(0), torch.zeros_like(c1))
    z2 = torch.where(live2, ((c2.abs() - e_r) / se2).clamp_min(0), torch.zeros_like(c2))
    z1, z2 = z1.nan_to_num(math.inf), z2.nan_to_num(math.inf)
    i1, i2 = int(torch.argmax(z1)), int(torch.argmax(z2))
    rep = FitReport(name, float(z1[i1]), i1, float(z2[i2]), i2, o.shape[0])
    if verbose:
        print(rep.line())
    return rep

"""Element-wise error bounds for the attention kernels (simpletuner_amd/csrc/attention.hip, attention_bwd.hip, csrc/gen/*.inc) against an fp64 reference of the SAME
bf16 q, k, v, dO (and the same fp32 key bias).  Counterpart of tests/gemm_bounds.py; every constant below is read off the kernels' arithmetic, none is fitted.

Rounding points (u = 2^-24, the fp32 unit roundoff; bf16 keeps 8 significant bits):
  scores      s = fp32 sum of exact bf16 products over d <= 128 (MFMA chains, -ffp-contract=fast), times scale2 = fp32(scale log2e), + fp32(bias log2e); the
              exponent argument a = s scale2 + bias log2e - m is formed with at most four more fp32 roundings.  Its absolute error (log2 units) is
                  ea <= u ((d + 2) scale2 sum_c |q_c k_c| + 4 (|s scale2| + |bias log2e|) + 2 |m|)
              (m = the row max in the forward, lse2 in the backward).  k_attn_bwd_dkv4 starts every score chain from lse2 / scale2 (the prep kernel writes it
              pre-divided, tools/kgen/dkv.py), so its chains also carry (d + 3) u |lse2|, and its dP chains start from +delta, (d + 3) u |delta|: `lse_in_chain`.
              K and V are only negated there (exact).  The generator's first version pre-scaled K by scale2 and re-rounded it to bf16, a relative 2^-9 error of
              every score term; no current route has it, so this model does not admit it (the CPU checker test shows it failing).
  exponential fast_exp2 = v_exp_f32, relative error <= 2^-22: P32 = P (1 + eps), eps <= ln2 ea + 2^-22.
  P / dS      packed to bf16 by RNE (pack8 / v_cvt_pk_bf16_f32) before the PV, dV, dK and dQ MFMAs; l sums the fp32 values, so the weights applied to V do
              not sum exactly to 1.  One RNE moves x by at most 2^-8 |x|.
  outputs     O = fp32(acc / l) rounded once; O_res = bf16(acc / l - O); lse2 = m + log2 l.  dV, dK (x scale) and dQ (x scale) are one RNE of the fp32 sum.
              k_attn_fwd64 takes exponentials against a reference max that may lag by up to 2^8: P reaches 2^8 instead of 1, the same relative precision.
  prep        delta = fp32 sum of bf16 O dO (+ O_res dO on the residual route): error <= u (d + 4) sum|O dO| (+ |O_res dO|).
  backward P  recomputed from the STORED lse2; dS = P32 (dP - delta), dP an fp32 sum of bf16 dO v products.
  dQ tail     dq64 + tail: the 64-row kernel stores a bf16 partial dQ over the full key tiles; the tail launch adds the last tile to it and rounds again.
  fp32 sums over the long axis (keys for O / dQ, queries for dK / dV): u (n + 8) sum of |terms| (+ 8: the per-tile rescales and the final multiply).

Per-element worst case: each output is checked as err <= tol = 1/2 ulp_bf16(|ref| + e) + e (one extra 1/2 ulp of the partial for the dQ tail route), e the sum of
|coefficient| x (the worst relative error of each rounded intermediate) over its terms, e.g. e_O = sum_j p_j |v_j| (2^-8 + eps_j) + |O| eps_l + u (Sk + 8) sum_j p_j |v_j|.

Chaining: the backward is bounded against an fp64 backward from the same bf16 q, k, v, dO and the kernel's OWN stored O (+ O_res) and lse2, so a one-ulp
difference in the forward cannot leak into the backward bound.  The unchained fp64 check (rel-L2 against the fully fp64 backward) keeps the suite's constants.

Localisation: over each (b, h, 64-row tile, head dim) block (rows = queries for O / dQ, keys for dK / dV) the mean of min((err / sigma)^2, 64) must stay
<= 1 + 8 / sqrt(n), n the rows of the block (2 for a full tile; a ragged last tile of n < 64 rows gets the same 5.6 standard deviations of its own mean).
sigma^2 is the model VARIANCE of the rounding errors: an RNE rounding of x with spacing ulp(x) is uniform in +-ulp / 2, variance ulp^2 / 12; the bf16
roundings of P and dS inside the sums are taken as roundings of values whose mantissa t in [1, 2) is log-uniformly distributed (exponentials of continuously
distributed scores), E[(ulp / x)^2] = 2^-14 E[1 / t^2] = 2^-14 (3 / (8 ln 2)), so Var = KAPPA x^2 with KAPPA = 2^-14 * 0.541 / 12.  Under the model every element
has E[(err / sigma)^2] <= 1 (values that round exactly, such as P = 1, contribute less).  The errors of different rows are independent, so a block of 64 rows is
a mean of at least 64 independent terms even when the errors of one row are fully correlated across its channels; for a chi-square(1) term (variance 2) that
mean has standard deviation <= sqrt(2 / n) (0.18 at n = 64), and the limit 1 + 8 / sqrt(n) sits 5.6 of those above the model's expectation.  The cap of 64 keeps one near-zero output
(whose ulp is tiny next to the fp32 summation error) from failing a block alone: it adds at most 64 / (64 d) to the block mean.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

F64 = torch.float64
U24 = 2.0 ** -24
LOG2E = 1.0 / math.log(2.0)
EXP_REL = 2.0 ** -22            # v_exp_f32
BF16_REL = 2.0 ** -8            # one RNE to bf16: |x - bf16(x)| <= 2^-8 |x|
KAPPA = 2.0 ** -14 * (3.0 / (8.0 * math.log(2.0))) / 12.0
BLOCK = 64
STAT_SIGMAS = 8.0          # block limit 1 + STAT_SIGMAS / sqrt(rows): 5.6 standard deviations of a mean of `rows` chi-square(1) terms
STAT_CAP = 64.0


def ulp_bf16(x):
    """the bf16 ulp at |x| (fp64 tensor): 2^(floor(log2 |x|) - 7); |x| below the smallest normal uses the subnormal spacing"""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def _chunks(n, step):
    for i in range(0, n, step):
        yield i, min(n, i + step)


@dataclass
class Fwd:
    O: torch.Tensor         # [B, H, Sq, d] fp64
    e_O: torch.Tensor       # worst-case error of the fp32 value before the output rounding
    var_O: torch.Tensor     # model variance of the P roundings' effect on O (the output rounding is added by check())
    lse2: torch.Tensor      # [B, H, Sq]
    e_lse2: torch.Tensor


def _scores(q, k, bias_b, scale):
    """fp64 natural-log scores and the log2-unit argument error ingredients of one chunk: s2 = scores in log2 units, mag2 = scale2 sum |q k|"""
    s = (q @ k.transpose(-1, -2)) * scale
    mag2 = (q.abs() @ k.abs().transpose(-1, -2)) * (scale * LOG2E)
    b2 = None
    if bias_b is not None:
        s = s + bias_b
        b2 = (bias_b * LOG2E).abs()
    return s, mag2, b2


def _arg_err(d, mag2, s2, b2, m):
    """ea (log2 units): fp32 score sum, scale multiply, bias add and the subtraction of m (the forward's row max / the backward's lse2)"""
    ea = U24 * ((d + 2) * mag2 + 4 * s2.abs() + 2 * m.abs())
    if b2 is not None:
        ea = ea + 4 * U24 * b2
    return ea


def attn_fwd_model(q, k, v, scale, bias=None, chunk=1024):
    """q [B, H, Sq, d], k / v [B, H, Sk, d] (bf16 or exact values), bias [B, Sk] natural-log units or None -> Fwd (fp64, on q's device)"""
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    nt = (Sk + 63) // 64
    O = torch.empty(B, H, Sq, d, dtype=F64, device=q.device)
    e_O, var_O = torch.empty_like(O), torch.empty_like(O)
    lse2 = torch.empty(B, H, Sq, dtype=F64, device=q.device)
    e_l = torch.empty_like(lse2)
    for b in range(B):
        bb = bias[b].to(F64) if bias is not None else None
        for h in range(H):
            kk, vv = k[b, h].to(F64), v[b, h].to(F64)
            va = vv.abs()
            for i0, i1 in _chunks(Sq, chunk):
                qq = q[b, h, i0:i1].to(F64)
                s, mag2, b2 = _scores(qq, kk, bb, scale)
                lse = torch.logsumexp(s, -1, keepdim=True)
                p = torch.exp(s - lse)
                s2 = s * LOG2E
                m = s2.max(-1, keepdim=True).values
                ea = _arg_err(d, mag2, s2, b2, m)
                eps = math.log(2.0) * ea + EXP_REL
                o = p @ vv
                pv = p @ va
                eps_l = eps.max(-1, keepdim=True).values + U24 * (Sk + 2 * nt)
                e = (p * (BF16_REL + eps)) @ va + o.abs() * eps_l + U24 * (Sk + 2 * nt + 8) * pv
                O[b, h, i0:i1] = o
                e_O[b, h, i0:i1] = e
                var_O[b, h, i0:i1] = KAPPA * ((p * p) @ (vv * vv))
                lse2[b, h, i0:i1] = (lse * LOG2E)[:, 0]
                e_l[b, h, i0:i1] = (ea.max(-1).values + LOG2E * (eps_l[:, 0] + U24 * 4) + U24 * 4 * (lse[:, 0].abs() * LOG2E + 1))
    return Fwd(O, e_O, var_O, lse2, e_l)


@dataclass
class Bwd:
    dQ: torch.Tensor
    e_dQ: torch.Tensor
    var_dQ: torch.Tensor
    dK: torch.Tensor
    e_dK: torch.Tensor
    var_dK: torch.Tensor
    dV: torch.Tensor
    e_dV: torch.Tensor
    var_dV: torch.Tensor
    dQ_part: torch.Tensor | None = None     # dq64 + tail: the fp64 dQ over the full key tiles (what the 64-row kernel stores, before the tail adds the rest)


def attn_bwd_model(q, k, v, dO, O, lse2, scale, bias=None, O_res=None, lse_in_chain=False, tail_from=None, chunk=1024):
    """fp64 backward of the same bf16 q, k, v, dO from the given O (+ O_res) and lse2 (the kernel's own: chained; or the fp64 forward's: unchained).
    All [B, H, S, d] (lse2 [B, H, Sq]).  lse_in_chain: the dkv4 route's dK / dV (score chains start from lse2 / scale2).  tail_from: the first key of the dQ tail
    (dq64 + tail: the partial dQ over keys [0, tail_from) is rounded to bf16 once more).  Returns Bwd with worst-case pre-rounding errors and model variances."""
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    f = lambda x: x.to(F64)
    out = {n: torch.zeros(B, H, S_, d, dtype=F64, device=q.device) for n, S_ in
           (("dQ", Sq), ("e_dQ", Sq), ("var_dQ", Sq), ("dK", Sk), ("e_dK", Sk), ("var_dK", Sk), ("dV", Sk), ("e_dV", Sk), ("var_dV", Sk))}
    part = torch.zeros(B, H, Sq, d, dtype=F64, device=q.device) if tail_from is not None else None
    for b in range(B):
        bb = bias[b].to(F64) if bias is not None else None
        for h in range(H):
            kk, vv = f(k[b, h]), f(v[b, h])
            for i0, i1 in _chunks(Sq, chunk):
                qq, gg, oo = f(q[b, h, i0:i1]), f(dO[b, h, i0:i1]), f(O[b, h, i0:i1])
                L2 = f(lse2[b, h, i0:i1])[:, None]
                s, mag2, b2 = _scores(qq, kk, bb, scale)
                s2 = s * LOG2E
                p = torch.exp2(s2 - L2)
                ea = _arg_err(d, mag2, s2, b2, L2)
                ea_kv = ea + (U24 * (d + 3) * L2.abs() if lse_in_chain else 0.0)
                delta = (gg * oo).sum(-1, keepdim=True)
                e_delta = U24 * (d + 4) * (gg.abs() * oo.abs()).sum(-1, keepdim=True)
                if O_res is not None:
                    rr = f(O_res[b, h, i0:i1])
                    delta = delta + (gg * rr).sum(-1, keepdim=True)
                    e_delta = e_delta + U24 * (d + 4) * (gg.abs() * rr.abs()).sum(-1, keepdim=True)
                dp = gg @ vv.t()
                e_dp = U24 * (d + 2) * (gg.abs() @ vv.abs().t())
                x = dp - delta
                ds = p * x
                ga, qa, ka = gg.abs(), qq.abs(), kk.abs()
                # dkv4's dP chains start from +delta and accumulate dO . (-v): the chain's roundings also carry (d + 3) u |delta|
                e_dp_kv = e_dp + (U24 * (d + 3) * delta.abs() if lse_in_chain else 0.0)
                for which, eak, edp in (("q", ea, e_dp), ("kv", ea_kv, e_dp_kv)):
                    eps = math.log(2.0) * eak + EXP_REL
                    # dS before its bf16 rounding: P's relative error, the dP / delta sums, the subtraction and the product
                    e_ds = ds.abs() * (eps + 2 * U24) + p * (edp + e_delta + U24 * x.abs())
                    e_dsr = e_ds + BF16_REL * (ds.abs() + e_ds)          # ... and after it
                    v_ds = KAPPA * ds * ds + (p * (edp + e_delta)) ** 2 / 3
                    if which == "q":
                        dq = scale * (ds @ kk)
                        out["dQ"][b, h, i0:i1] = dq
                        out["e_dQ"][b, h, i0:i1] = scale * (e_dsr @ ka) + U24 * (Sk + 8) * scale * (ds.abs() @ ka)
                        out["var_dQ"][b, h, i0:i1] = scale * scale * (v_ds @ (kk * kk))
                        if part is not None:
                            part[b, h, i0:i1] = scale * (ds[:, :tail_from] @ kk[:tail_from])
                    else:
                        out["dK"][b, h] += scale * (ds.t() @ qq)
                        out["e_dK"][b, h] += scale * (e_dsr.t() @ qa) + U24 * (Sq + 8) * scale * (ds.abs().t() @ qa)
                        out["var_dK"][b, h] += scale * scale * (v_ds.t() @ (qq * qq))
                        out["dV"][b, h] += p.t() @ gg
                        out["e_dV"][b, h] += (p * (eps + BF16_REL)).t() @ ga + U24 * (Sq + 8) * (p.t() @ ga)
                        out["var_dV"][b, h] += KAPPA * ((p * p).t() @ (gg * gg))
    return Bwd(dQ_part=part, **out)


def rope_norm_bwd_model(g, tol_g, var_g, z, rrms, w, cos, sin):
    """The fused RoPE + RMSNorm backward epilogue (attention_bwd.hip rope_bwd_finish) carried in fp64: out = r (w dy - (y / w) mean(dy y)), dy = R^T g,
    y = R^T z.  It is linear in g with Jacobian J = r (diag(w) R^T - (1/128) diag(y / w) z^T) (mean(dy y) = (g . z) / 128: R is orthogonal), so
        want = J g,  e = |J| tol_g + e_fp32,  var = sum_j J_ij^2 var_g_j
    g: the fp64 reference gradient w.r.t. the roped head-major activation [B, H, S, 128]; tol_g / var_g: the error bound / variance of the kernel's bf16 g (the
    stored dQ / dK bound, its output rounding included).  z: the roped activation (bf16 Q or K) [B, H, S, 128]; rrms [B, H, S] fp32; w [B, H, S, 128] (per
    token: w_lo / w_hi by position); cos / sin [S, 64] fp32.  e_fp32: the epilogue's fp32 arithmetic (two-term rotations, the 128-term sum, v_rcp_f32 of w,
    the products): u (8 r |w dy| + 8 r |y / w| |m| + 130 r |y / w| sum|dy y| / 128), far below one bf16 ulp."""
    f = lambda x: x.to(F64)
    g, z, r, w = f(g), f(z), f(rrms)[..., None], f(w)
    c = f(cos)[None, None].repeat_interleave(2, -1)
    sn = f(sin)[None, None].repeat_interleave(2, -1)

    def rt(v):          # R^T v per pair: (v0 c + v1 s, v1 c - v0 s)
        v0, v1 = v[..., 0::2], v[..., 1::2]
        out = torch.empty_like(v)
        out[..., 0::2] = v0 * c[..., 0::2] + v1 * sn[..., 0::2]
        out[..., 1::2] = v1 * c[..., 0::2] - v0 * sn[..., 0::2]
        return out

    def rt_abs(v):      # |R^T| v
        v0, v1 = v[..., 0::2], v[..., 1::2]
        out = torch.empty_like(v)
        ca, sa = c[..., 0::2].abs(), sn[..., 0::2].abs()
        out[..., 0::2] = v0 * ca + v1 * sa
        out[..., 1::2] = v1 * ca + v0 * sa
        return out

    def rt_sq(v):       # (R^T)^2 v (element-wise squares)
        v0, v1 = v[..., 0::2], v[..., 1::2]
        out = torch.empty_like(v)
        c2, s2 = c[..., 0::2] ** 2, sn[..., 0::2] ** 2
        out[..., 0::2] = v0 * c2 + v1 * s2
        out[..., 1::2] = v1 * c2 + v0 * s2
        return out

    dy, y = rt(g), rt(z)
    m = (g * z).sum(-1, keepdim=True) / 128
    a = y / (128 * w)
    want = r * (w * dy - (y / w) * m)
    e = r * (w.abs() * rt_abs(tol_g) + (y / w).abs() * (z.abs() * tol_g).sum(-1, keepdim=True) / 128)
    e = e + U24 * r * (8 * (w * dy).abs() + 8 * (y / w).abs() * m.abs() + 130 * (y / w).abs() * (dy * y).abs().sum(-1, keepdim=True) / 128)
    # sum_j J_ij^2 var_j with J_ij = r (w_i Rt_ij - a_i z_j)
    var = r * r * (w * w * rt_sq(var_g) - 2 * w * a * rt(z * var_g) + a * a * (z * z * var_g).sum(-1, keepdim=True))
    return want, e, var.clamp_min(0)


def stored_tol_var(want, e, var):
    """the error bound and variance of a stored bf16 output (one RNE of the modelled fp32 value), as rope_norm_bwd_model takes them for its input"""
    return 0.5 * ulp_bf16(want.abs() + e) + e, var + ulp_bf16(want) ** 2 / 12


# ---- the check ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    name: str
    worst: float            # max err / tol
    worst_at: tuple         # (b, h, row, channel)
    block_stat: float       # mean(min((err / sigma)^2, 64)) of the (b, h, 64-row tile) block closest to its limit
    block_at: tuple         # (b, h, row tile)
    n: int
    block_limit: float = 2.0

    @property
    def ok_elem(self):
        return self.worst <= 1.0

    @property
    def ok_block(self):
        return self.block_stat <= self.block_limit

    @property
    def ok(self):
        return self.ok_elem and self.ok_block

    def line(self):
        return (f"[bound] {self.name}: worst err/tol={self.worst:.3f} at {self.worst_at}; worst block mean (err/sigma)^2={self.block_stat:.3f} "
                f"(limit {self.block_limit:.2f}) at (b, h, tile) {self.block_at}; {self.n} outputs")


def check(name, out, want, e, var, extra_round=None, final=None, verbose=True):
    """out: the kernel's output as [B, H, S, d] (any float dtype; a view of the stored layout); want / e / var: fp64 [B, H, S, d] from the models above.
    extra_round: [B, H, S, d] values rounded to bf16 once more on this route (the dq64 + tail partial), or None.  final: the value whose bf16 rounding ends
    the computation when that is not the output itself (O + O_res: the residual O_res; default want).  Returns a Report."""
    o = out.to(F64)
    assert o.shape == want.shape, (name, tuple(o.shape), tuple(want.shape))
    err = (o - want).abs()
    fr = want if final is None else final
    tol = 0.5 * ulp_bf16(fr.abs() + e) + e
    sig2 = var + ulp_bf16(fr) ** 2 / 12
    if extra_round is not None:
        tol = tol + 0.5 * ulp_bf16(extra_round.abs() + e)
        sig2 = sig2 + ulp_bf16(extra_round) ** 2 / 12
    fin = torch.isfinite(o)
    ratio = torch.where(fin, err / tol, torch.full_like(err, math.inf))
    flat = int(torch.argmax(ratio))
    worst = float(ratio.reshape(-1)[flat])
    B, H, S, d = o.shape
    z = torch.where(fin, err * err / sig2, torch.full_like(err, STAT_CAP)).clamp(max=STAT_CAP)
    nb = (S + BLOCK - 1) // BLOCK
    zp = torch.zeros(B, H, nb * BLOCK, d, dtype=F64, device=o.device)
    cnt = torch.zeros_like(zp)
    zp[:, :, :S] = z
    cnt[:, :, :S] = 1
    ms = zp.view(B, H, nb, BLOCK * d).sum(-1) / cnt.view(B, H, nb, BLOCK * d).sum(-1)
    rows = torch.full((nb,), float(BLOCK), dtype=F64, device=o.device)
    rows[-1] = S - (nb - 1) * BLOCK
    lim = 1 + STAT_SIGMAS / rows.sqrt()
    bflat = int(torch.argmax((ms - 1) / (lim - 1)))
    bi = _unravel(bflat, (B, H, nb))
    rep = Report(name, worst, tuple(int(x) for x in _unravel(flat, (B, H, S, d))), float(ms.reshape(-1)[bflat]),
                 tuple(int(x) for x in bi), o.numel(), float(lim[bi[2]]))
    if verbose:
        print(rep.line())
    return rep


def check_lse2(name, out, want, e, verbose=True):
    """lse2 [B, H, Sq] fp32: element-wise only (one value per row)"""
    o = out.to(F64)
    err = (o - want).abs()
    tol = e + U24 * want.abs()
    ratio = torch.where(torch.isfinite(o), err / tol, torch.full_like(err, math.inf))
    flat = int(torch.argmax(ratio))
    rep = Report(name, float(ratio.reshape(-1)[flat]), tuple(int(x) for x in _unravel(flat, tuple(o.shape))), 0.0, (), o.numel())
    if verbose:
        print(rep.line())
    return rep


def _unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


def assert_bound(rep: Report):
    assert rep.ok_elem, rep.line()
    assert rep.ok_block, rep.line()


def rel_l2(out, ref):
    """the suite's existing global check"""
    o, r = out.to(F64), ref.to(F64)
    return float((o - r).norm() / r.norm().clamp_min(1e-300))

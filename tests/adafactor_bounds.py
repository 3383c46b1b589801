"""Element-wise error bounds for one fused Adafactor step (simpletuner_amd/csrc/adafactor.hip: k_af_stats, k_af_factors, k_af_coef, k_af_update) against the
fp64 restatement of the SAME stored inputs (tests/adafactor_ref.py:step_tensor), in the spirit of tests/lion_bounds.py / tests/soap_bounds.py.

Where the bounds come from.  The kernels compute in fp32, u = 2^-24 per rounding.  Instead of first-order formulas every quantity is carried as an
INTERVAL [lo, hi] in fp64 that is known to contain what fp32 arithmetic in the kernels' order can produce, whatever the contraction (a fused
multiply-add rounds once where the interval widens twice, never more):
    rnd[lo, hi]        = [lo - u |lo|, hi + u |hi|]                 one rounding to nearest of any value in the interval (rounding is monotone)
    sum of n >= 0 terms = [sum lo (1 - u)^D, sum hi (1 + u)^D]      D = the largest number of additions one term passes through, in ANY order
    x y, x / y, sqrt x, max(x, c), x + y, x - y                     exact interval arithmetic, then rnd (sqrt: rnd twice, i.e. 1 ulp = 2u, should the
                                                                    hardware form not round correctly; the reciprocal square root: 2 ulp = 4u)
The expressions, as the kernels spell them (T = the tensor's tiles, tile = 64 rows x 256 columns, wave = 16 rows, lane = 4 columns):
    g'  = rnd(gs g)                       g2 = rnd(g' g')
    row sum: D = 4 (lane) + 6 (butterfly) + ntc (tiles);  column sum: D = 16 (lane) + 3 (waves) + ntr (tiles);  small matrices: D = C, D = R
    mean = rnd(sum / n);  lerp: w < 0.5: rnd(a + rnd(w rnd(b - a))), else rnd(b - rnd(rnd(b - a) (1 - w)))      (1 - w exact for w in [0.5, 1])
    rm  = max(rnd(sum row_var / R), eps1),  D = ceil(R / 256) + 9  (small: R)
    v   = rnd(rnd(rv / rm) cv);  r = rsq(max(v, eps1^2)) within 2 ulp = 4u (v_rsq_f32 is specified to 1 ulp);  uu = rnd(g' r)
    sum p^2, sum uu^2: the squares rounded, D = elements per thread (64, vec 4, small R C) + 9 (block) + ceil(T / 256) + 9
    rn  = rnd rnd(sqrt(numel));  alpha = rnd(max(eps2, rnd(rnd rnd(sqrt(sum p^2)) / rn)) rho)
    denom = max(1, rnd(rnd rnd(sqrt(sum uu^2)) / rnd(rn d)));  coef = rnd(alpha / denom)
    p'  = rnd(rnd(p decay) - rnd(coef uu)), then ONE rounding into the arena dtype (bf16: u = 2^-8, nearest even)
The rule has clamps and two max: all are 1-Lipschitz and monotone, so an interval passes through them as it is; nothing is discontinuous, and EVERY
element of p, row_var, col_var and variance is compared.  The scalars are the fp32 values the launcher forms (consts()).  No number here is fitted
to a kernel's output.  The same intervals bound the fp32 stand-in of tests/adafactor_ref.py (torch's reductions are some order of at most as many
additions per term), which is how the CPU tests use them."""
from __future__ import annotations

import numpy as np
import torch

from tests import adafactor_ref as AR

U = 2.0 ** -24
UB = 2.0 ** -8          # bf16: 8 significand bits, round to nearest: half an ulp is at most 2^-8 of the value
F64 = torch.float64
TR, TC, VEC_ITEM, SMALL_MAX = 64, 256, 1024, 64


def f32(x):
    return float(np.float32(x))


def consts(step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale):
    """every scalar as the fp32 value the kernels use (st355_adafactor_step takes doubles and rounds each once; eps1^2 and 1 - lr weight_decay are formed
    in double first)"""
    return AR.scalars_f32(step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale)


class Iv:
    """a closed interval of fp64 tensors"""

    def __init__(self, lo, hi=None):
        lo = torch.as_tensor(lo, dtype=F64)
        self.lo, self.hi = lo, lo if hi is None else torch.as_tensor(hi, dtype=F64)

    def rnd(self, k=1):
        lo, hi = self.lo, self.hi
        for _ in range(k):
            lo, hi = lo - U * lo.abs(), hi + U * hi.abs()
        return Iv(lo, hi)

    def __add__(self, o):
        o = _iv(o)
        return Iv(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        o = _iv(o)
        return Iv(self.lo - o.hi, self.hi - o.lo)

    def __mul__(self, o):
        o = _iv(o)
        a, b, c, d = self.lo * o.lo, self.lo * o.hi, self.hi * o.lo, self.hi * o.hi
        return Iv(torch.minimum(torch.minimum(a, b), torch.minimum(c, d)), torch.maximum(torch.maximum(a, b), torch.maximum(c, d)))

    def div_pos(self, o):
        """by an interval of positive numbers"""
        o = _iv(o)
        assert bool((o.lo > 0).all())
        return self * Iv(1.0 / o.hi, 1.0 / o.lo)

    def sqrt(self):
        return Iv(self.lo.clamp(min=0).sqrt(), self.hi.clamp(min=0).sqrt())

    def max(self, c):
        return Iv(self.lo.clamp(min=c), self.hi.clamp(min=c))

    def nonneg(self):
        return Iv(self.lo.clamp(min=0), self.hi.clamp(min=0))

    def sum_pos(self, dim, depth, keepdim=True):
        """a sum of non-negative terms along dim in any order with at most `depth` additions per term; dim=None: all of them"""
        if dim is None:
            return Iv(self.lo.sum() * (1 - U) ** depth, self.hi.sum() * (1 + U) ** depth)
        return Iv(self.lo.sum(dim, keepdim=keepdim) * (1 - U) ** depth, self.hi.sum(dim, keepdim=keepdim) * (1 + U) ** depth)


def _iv(x):
    return x if isinstance(x, Iv) else Iv(x)


def lerp(a, b, w):
    """a: the stored fp32 state (exact), b: an interval, w: the fp32 weight"""
    diff = (b - a).rnd()
    if w < 0.5:
        return ((diff * w).rnd() + a).rnd().nonneg()
    return (b - (diff * (1.0 - w)).rnd()).rnd().nonneg()


def kind_of(shape):
    batch, R, C = AR.factor_shape(shape)
    return "vec" if R == 0 else ("small" if batch > 1 and R * C <= SMALL_MAX else "mat")


def step_intervals(shape, p, g, state, c, arena_dtype, any_order=False):
    """p, g: the tensor's stored values; state: its stored fp32 state (row_var [batch, R, 1], col_var [batch, 1, C] or variance [C]) BEFORE the step;
    c: consts().  Returns {"p", "row_var", "col_var" | "variance"}: the intervals of what the kernels may store.  any_order: every sum with D = its
    number of terms, which holds for ANY summation order (the fp32 stand-in's reductions are torch's, whose order is not the kernels')"""
    batch, R, C = AR.factor_shape(shape)
    kind = kind_of(shape)
    numel = batch * max(R, 1) * C
    p, g = AR.as3(p.to(F64), shape), AR.as3(g.to(F64), shape)
    g1 = (Iv(g) * c["gs"]).rnd()
    g2 = (g1 * g1).rnd().nonneg()
    out = {}
    if kind == "vec":
        tiles, per_thread = -(-C // VEC_ITEM), VEC_ITEM // 256
        v = out["variance"] = lerp(state["variance"].to(F64), g2, c["omb2"])
    else:
        if kind == "mat":
            ntr, ntc = -(-R // TR), -(-C // TC)
            tiles, per_thread = batch * ntr * ntc, 64
            d_row, d_col, d_rm = 4 + 6 + ntc, 16 + 3 + ntr, -(-R // 256) + 9
        else:
            tiles, per_thread = -(-batch // 256), R * C
            d_row, d_col, d_rm = C, R, R
        if any_order:
            d_row, d_col, d_rm = C, R, R
        row_mean = g2.sum_pos(-1, d_row).div_pos(float(C)).rnd()
        col_mean = g2.sum_pos(-2, d_col).div_pos(float(R)).rnd()
        rv = out["row_var"] = lerp(state["row_var"].to(F64), row_mean, c["omb2"])
        cv = out["col_var"] = lerp(state["col_var"].to(F64), col_mean, c["omb2"])
        rm = rv.sum_pos(-2, d_rm).div_pos(float(R)).rnd().max(c["eps1"])
        v = (rv.div_pos(rm).rnd() * cv).rnd()
    r = Iv(1.0).div_pos(v.max(c["eps1sq"]).sqrt()).rnd(4)
    uu = (g1 * r).rnd()
    depth = per_thread + 9 + -(-tiles // 256) + 9
    if any_order:
        depth = numel
    sp = (Iv(p) * Iv(p)).rnd().nonneg().sum_pos(None, depth)
    su = (uu * uu).rnd().nonneg().sum_pos(None, depth)
    rn = Iv(float(numel)).rnd().sqrt().rnd(2)          # (float)numel rounds only from 2^24 elements on
    alpha = (sp.sqrt().rnd(2).div_pos(rn).rnd().max(c["eps2"]) * c["rho"]).rnd()
    denom = su.sqrt().rnd(2).div_pos((rn * c["d"]).rnd()).rnd().max(1.0)
    coef = alpha.div_pos(denom).rnd()
    new = ((Iv(p) * c["decay"]).rnd() - (uu * coef).rnd()).rnd()
    if arena_dtype == torch.bfloat16:
        new = Iv(new.lo - UB * new.lo.abs(), new.hi + UB * new.hi.abs())
    out["p"] = new
    return out


def check(name, got, iv, want, worst):
    """every element of `got` inside the interval (+ the fp32 flush-to-zero floor), and the restatement `want` inside it too (the interval is a bound
    AROUND the fp64 result, not beside it); returns the largest |got - want| / (half the interval's width) seen so far"""
    got, want = got.to(F64).reshape(iv.lo.shape), want.to(F64).reshape(iv.lo.shape)
    floor = 1e-37
    assert bool((iv.lo - floor <= want).all() and (want <= iv.hi + floor).all()), f"{name}: the fp64 restatement lies outside its own interval"
    below, above = iv.lo - floor - got, got - iv.hi - floor
    bad = (below > 0) | (above > 0)
    bound = torch.maximum(iv.hi - want, want - iv.lo) + floor
    ratio = float(((got - want).abs() / bound).max())
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |err| / bound = {ratio:.3f} "
                                 f"(max |err| {float((got - want).abs().max()):.3e})")
    return max(worst, ratio)


def check_step(tag, shapes, p_before, g, states_before, p_after, states_after, c, arena_dtype, worst=0.0, any_order=False):
    """all tensors of one arena step: p_before / g / p_after are lists of tensors, states_* lists of dicts (fp32, torch's layout); the fp64 restatement runs
    from the same stored inputs.  Returns (worst ratio, the restatement's intermediates per tensor)"""
    inter = []
    for i, s in enumerate(shapes):
        iv = step_intervals(s, p_before[i], g[i], states_before[i], c, arena_dtype, any_order)
        st64 = {k: AR.as3(v.to(F64), s).clone() if k == "variance" else v.to(F64).reshape(AR.new_state(s)[k].shape).clone() for k, v in states_before[i].items()}
        want_p, x = AR.step_tensor(AR.as3(p_before[i].to(F64), s), AR.as3(g[i].to(F64), s), st64, c)
        inter.append(x)
        worst = check(f"{tag} tensor {i} {s} p", p_after[i], iv["p"], want_p, worst)
        for k in st64:
            worst = check(f"{tag} tensor {i} {s} {k}", states_after[i][k], iv[k], st64[k], worst)
    return worst, inter


__all__ = ["U", "UB", "Iv", "consts", "step_intervals", "check", "check_step", "kind_of", "f32", "AR"]

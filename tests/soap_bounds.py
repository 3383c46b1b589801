"""Element-wise error bounds for one fused SOAP step (simpletuner_amd/csrc/soap.hip: k_soap_step + k_soap_fold) against the fp64 restatement of the
SAME stored inputs (tests/soap_ref.py:one_step_fp64), written like tests/lion_bounds.py.

Where the bounds come from.  The kernel computes in fp32, u = 2^-24 per rounding, in the order below (r x L orientation, Q the kernel's own r x r
basis, R = r rounded up to 32).  A fused multiply-add rounds once where the bound counts two roundings, never more.  A v_mfma_f32_32x32x2_f32 chain
over K terms is a k-ordered fp32 fma chain: |error| <= gamma_K sum |a b|, gamma_K = K u / (1 - K u); the zero padding adds exact zeros.  The
scalars are the fp32 values that cross the ABI (consts()); 1 - beta is formed in double by the launcher and rounded once.  |.| products are fp64.
No number below is fitted to a kernel's output.
    g' = s g                               e_g  = u |g'|
    m' = fma(1-b1, g', b1 m)               e_m  = (1-b1) e_g + u |b1 m| + u |m'|                                  (checked: exp_avg)
    gp = Q^T g'                            e_gp = |Q|^T e_g + gamma_R |Q|^T |g'|
    v' = fma(1-b2, gp gp, b2 v)            e_v  = (1-b2) (2 |gp| e_gp + e_gp^2 + u (|gp| + e_gp)^2) + u |b2 v| + u |v'|   (checked: exp_avg_sq)
    mp = Q^T m'                            e_mp = |Q|^T e_m + gamma_R |Q|^T |m'|
    d  = sqrt(v') + eps                    e_d  = min(e_v / sqrt(v'), sqrt(e_v)) + 2u sqrt(v') + u d              (|sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt|a - b|)
    w  = mp / d                            e_w  = (e_mp + |w| e_d) / (d - e_d) + u (|w| + the same)               (the quotient, correctly rounded; d - e_d > 0)
    uu = Q w                               e_u  = |Q| e_w + gamma_R |Q| |w|
    p1 = fma(-step, uu, p)                 e_p1 = step e_u + u |p1|
    p2 = fma(-lr wd, p1, p1)               e_p2 = (1 + lr wd) e_p1 + u |p2|                                       (checked: the parameter)
    S  = g' g'^T  (four waves' chains, 3 adds, the chunks in order)      e_S = |g'| e_g^T + e_g |g'|^T + e_g e_g^T + gamma_(L + nch + 4) |g'| |g'|^T
    GG'= fma(w, S - GG, GG)                e_GG = w (e_S + u |S - GG|) + u |GG'|                                   (checked: GG; w >= 0.5: S - (S - GG)(1 - w),
                                                                                                                   e_GG = e_S + (1 - w)(e_S + 2 u |S - GG|) + u |GG'|)
Where d - e_d <= 0 (a projected gradient below its own error while v is still zero) the kernel's denominator is only known to be >= eps (1 - u):
e_w = |w| + (|mp| + e_mp) / (eps (1 - 4u)) there, which loosens that column of p; the share of such elements (`loose`) must stay below 1e-3.  Every element of p, exp_avg, exp_avg_sq and GG is compared; none is skipped.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import soap_ref as SR

U = 2.0 ** -24
F64 = torch.float64


def f32(x):
    return float(np.float32(x))


def gamma(k):
    return k * U / (1 - k * U)


def consts(grad_scale, beta1, beta2, eps, step_size, lr_weight_decay, gg_weight):
    """every scalar as the fp32 value the kernel uses (st355_soap_step forms 1 - beta in double and rounds once)"""
    return dict(gs=f32(grad_scale), b1=f32(beta1), omb1=f32(1.0 - beta1), b2=f32(beta2), omb2=f32(1.0 - beta2), eps=f32(eps), step=f32(step_size),
                lrwd=f32(lr_weight_decay), w=f32(gg_weight))


def step_size(lr, betas, t, correct_bias=True):
    """the host double St355Soap passes (:187-191)"""
    s = lr
    if correct_bias:
        s = s * ((1.0 - betas[1] ** t) ** 0.5) / (1.0 - betas[0] ** t)
    return s


def step_bounds(x, c, L):
    """x = SR.one_step_fp64(...); returns the bounds (m, v, p, GG) in the r x L orientation"""
    r = x["Q"].shape[0]
    R = (r + 31) // 32 * 32
    nch = (L + 511) // 512
    aQ = x["Q"].abs()
    g1, m1, gp, v1, mp, d, w, p1, p2 = (x[k] for k in ("g1", "m1", "gp", "v1", "mp", "d", "w", "p1", "p2"))
    e_g = U * g1.abs()
    e_m = c["omb1"] * e_g + U * (c["b1"] * x["m"]).abs() + U * m1.abs()
    e_gp = aQ.T @ e_g + gamma(R) * (aQ.T @ g1.abs())
    e_v = c["omb2"] * (2 * gp.abs() * e_gp + e_gp ** 2 + U * (gp.abs() + e_gp) ** 2) + U * (c["b2"] * x["v"]).abs() + U * v1.abs()
    e_mp = aQ.T @ e_m + gamma(R) * (aQ.T @ m1.abs())
    sq = v1.sqrt()
    e_sq = torch.minimum(e_v / sq.clamp(min=1e-300), e_v.sqrt())
    e_d = e_sq + 2 * U * sq + U * d                      # v_sqrt_f32 is accurate to 1 ulp = 2u, not correctly rounded
    safe = d - e_d > 0
    # where the denominator's bound reaches zero (|gp| below its own error on a first step) only d^ >= eps (1 - u) is known: |w^| <= (|mp| + e_mp) / that
    e_w = torch.where(safe, (e_mp + w.abs() * e_d) / (d - e_d).clamp(min=1e-300), w.abs() + (mp.abs() + e_mp) / (c["eps"] * (1 - 4 * U)))
    e_w = e_w + U * (w.abs() + e_w)
    e_u = aQ @ e_w + gamma(R) * (aQ @ w.abs())
    e_p1 = c["step"] * e_u + U * p1.abs()
    e_p = (1 + c["lrwd"]) * e_p1 + U * p2.abs() if c["lrwd"] > 0 else e_p1
    ag = g1.abs()
    e_S = ag @ e_g.T + e_g @ ag.T + e_g @ e_g.T + gamma(L + nch + 4) * (ag @ ag.T)
    dif = (x["S"] - x["GG"]).abs()
    if c["w"] < 0.5:
        e_GG = c["w"] * (e_S + U * dif) + U * x["GG1"].abs()
    else:
        e_GG = e_S + (1 - c["w"]) * (e_S + 2 * U * dif) + U * x["GG1"].abs()
    return dict(m=e_m, v=e_v, p=e_p, GG=e_GG, loose=float((~safe).to(F64).mean()))


def check(name, got, want, bound, worst):
    """every element of `got` within `bound` of `want` (+ the fp32 denormal floor); returns the largest |err| / bound seen so far"""
    err = (got.to(F64) - want).abs()
    lim = bound * (1 + 1e-6) + 1e-45                     # 1e-6: the second-order terms (u times a bound) the first-order formulas leave out
    ratio = float((err / lim).max())
    assert bool((err <= lim).all()), f"{name}: |err| / bound = {ratio:.3f} (max |err| {float(err.max()):.3e})"
    return max(worst, ratio)


def orient(t, wide):
    return t if wide else t.T


__all__ = ["U", "consts", "step_size", "step_bounds", "check", "gamma", "f32", "orient", "SR"]

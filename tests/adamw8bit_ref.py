"""fp64 restatement of 8-bit block-wise AdamW (simpletuner_amd/csrc/adamw8bit.hip: st355_adamw8bit_step) and its element bounds, written like tests/step_bounds.py
(whose U, U_DIV, U_SQRT and f32 are used).  Nothing here reads the product's codebooks: they are rebuilt from the published recipe (Dettmers et al. 2022).

Where the bounds come from.  The kernel computes in fp32, u = 2^-24 per rounding, sqrtf and a division 4 u each (step_bounds), in the order below; a fused
multiply-add rounds once where two roundings are counted, never more.  The scalars are the fp32 values that cross the ABI; lr wd, 1 - beta are formed in fp32
by the launcher and are among the roundings counted; step_size and bc2_sqrt are rounded from double as st355_adamw_ema_step's.  No number is fitted to the kernel.
    m0 = codebook[code] s  (quantised) | stored fp32  e_m0 = u |m0| | 0            (v0 the same)
    g' = g grad_scale                                 e_g = u |g'|
    p1 = p - (lr wd) p                                e_p1 = 2 u |lr wd p| + u |p1|                        (lr wd, its product with p; the subtraction)
    m' = m0 + (1 - b1)(g' - m0)                       e_m = e_m0 + (1 - b1)(e_g + e_m0) + 3 u (1 - b1) |g' - m0| + u |m'|
    v' = v0 + (1 - b2)(g' g' - v0)                    e_gg = 2 |g'| e_g + u g'^2;  e_v = e_v0 + (1 - b2)(e_gg + e_v0) + 3 u (1 - b2) |g'^2 - v0| + u |v'|
    sq = sqrtf(v')                                    e_sq = e_v / (sqrt(v'-) + sqrt(v' + e_v)) + 4 u sq,  v'- = max(v' - e_v, 0)  (at most sqrt(e_v) at v' = 0)
    den = sq / bc2_sqrt + eps                         e_den = e_sq / bc2_sqrt + 4 u sq / bc2_sqrt + u den
    p' = p1 - step_size (m' / den)                    e_p = e_p1 + step_size ((e_m + |m' / den| e_den) / (den - e_den) + 4 u |m' / den|) + u |upd| + u |p'|
p' is stored in fp32 (tol = e_p, whose last term is the store's rounding) or after one RNE to bf16 (tol = 1/2 ulp_bf16(|p'| + e_p) + e_p); plain m', v' are
fp32 outputs with tol = e_m, e_v.  Every bound carries ABS = 2^-126 on top: below it fp32 is denormal and a rounding is absolute, not relative.
Block scale s' = max(max |x'|, 1e-12): max is 1-Lipschitz in the sup norm, so |s'_kernel - s'_ref| <= e_s = max over the block of e_x, i.e. e_s / ulp(s') ulps.
Code: x = x' / s' is formed with e_x' and e_s and one division, delta = (e_x + |x_ref| e_s) / (s' - e_s) + 4 u |x_ref|; the nearest value to a point within delta
of x_ref is within h + delta of x_ref, h = half the gap of the bracket of x_ref (below the lowest signed value -0.993: the distance to it).  Since |codebook| <= 1:
|codebook[code] s'_kernel - x'_ref| <= h s' + (e_s + s' delta).  Holds at ties, whichever side the kernel takes.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import gemm_bounds as GB
from tests.step_bounds import U, U_DIV, U_SQRT, f32

F64 = torch.float64
BLOCK, MIN_NUMEL, FLOOR, ABS = 256, 4096, f32(1e-12), 2.0 ** -126


def codebooks():
    """(signed, unsigned) as fp64 tensors holding the fp32-rounded values, ascending"""
    def decades(extra):
        out = []
        for i in range(7):
            k = 2 ** (i + extra)
            edges = np.linspace(0.1, 1.0, k + 1)
            out += [float((edges[j] + edges[j + 1]) / 2 * 10.0 ** (i - 6)) for j in range(k)]
        return out
    pos = decades(0)
    signed = sorted([-x for x in pos] + [0.0] + pos + [1.0])
    unsigned = sorted([0.0] + decades(1) + [1.0])
    return tuple(torch.tensor(np.array(c, dtype=np.float64).astype(np.float32).astype(np.float64)) for c in (signed, unsigned))


def eligible(numel):
    return numel >= MIN_NUMEL and numel % BLOCK == 0


def dequantise(cb, codes, scales):
    """codes [n] uint8, scales [n / 256] fp32 -> fp64 [n]"""
    return cb[codes.long()] * scales.to(F64).repeat_interleave(BLOCK)


def quantise(cb, x):
    """x fp64 [n] -> (codes uint8, scales fp64): the nearest codebook value to x / s, the lower index at a tie"""
    s = x.view(-1, BLOCK).abs().amax(1).clamp_min(FLOOR)
    xn = x / s.repeat_interleave(BLOCK)
    hi = torch.searchsorted(cb, xn).clamp(0, 255)
    lo = (hi - 1).clamp_min(0)
    return torch.where((xn - cb[lo]).abs() <= (cb[hi] - xn).abs(), lo, hi).to(torch.uint8), s


def consts(lr, beta1, beta2, eps, wd, step, grad_scale):
    lr, b1, b2 = f32(lr), f32(beta1), f32(beta2)
    return dict(lrwd=lr * f32(wd), omb1=1.0 - b1, omb2=1.0 - b2, eps=f32(eps), gs=f32(grad_scale), step_size=f32(lr / (1.0 - b1 ** step)),
                bc2_sqrt=f32(np.sqrt(1.0 - b2 ** step)))


def step(p, g, m0, v0, c, dequantised):
    """one step from the stored state (fp64-able, flat).  Returns dict name -> (want, e) for m, v, p (e_p without the bf16 store)"""
    p, g, m0, v0 = p.to(F64), g.to(F64), m0.to(F64), v0.to(F64)
    e_m0, e_v0 = (U * m0.abs(), U * v0.abs()) if dequantised else (0.0 * m0, 0.0 * v0)
    g1 = g * c["gs"]
    e_g = U * g1.abs()
    dec = c["lrwd"] * p
    p1 = p - dec
    e_p1 = 2 * U * dec.abs() + U * p1.abs()
    dm = g1 - m0
    m1 = m0 + c["omb1"] * dm
    e_m = e_m0 + c["omb1"] * (e_g + e_m0) + 3 * U * c["omb1"] * dm.abs() + U * m1.abs() + ABS
    gg = g1 * g1
    dv = gg - v0
    v1 = v0 + c["omb2"] * dv
    e_v = e_v0 + c["omb2"] * (2 * g1.abs() * e_g + U * gg + e_v0) + 3 * U * c["omb2"] * dv.abs() + U * v1.abs() + ABS
    sq = torch.sqrt(v1)
    e_sq = e_v / (torch.sqrt((v1 - e_v).clamp_min(0)) + torch.sqrt(v1 + e_v)) + U_SQRT * sq
    q = sq / c["bc2_sqrt"]
    den = q + c["eps"]
    e_den = e_sq / c["bc2_sqrt"] + U_DIV * q + U * den
    ratio = m1 / den
    upd = c["step_size"] * ratio
    p2 = p1 - upd
    e_p = e_p1 + c["step_size"] * ((e_m + ratio.abs() * e_den) / (den - e_den).clamp_min(1e-300) + U_DIV * ratio.abs()) + U * upd.abs() + U * p2.abs() + ABS
    return {"m": (m1, e_m), "v": (v1, e_v), "p": (p2, e_p)}


def p_tol(want, e, bf16_out):
    return 0.5 * GB.ulp_bf16(want.abs() + e) + e if bf16_out else e


def code_bound(cb, x_ref, e_x):
    """(s_ref, e_s per block, tol per element): tolerance of |codebook[code] s_kernel - x_ref| for the block-wise quantisation of x_ref +- e_x"""
    s = x_ref.view(-1, BLOCK).abs().amax(1).clamp_min(FLOOR)
    e_s = e_x.view(-1, BLOCK).amax(1)
    sb, esb = s.repeat_interleave(BLOCK), e_s.repeat_interleave(BLOCK)
    xn = x_ref / sb
    hi = torch.searchsorted(cb, xn).clamp(0, 255)
    lo = (hi - 1).clamp_min(0)
    h = torch.where(xn < cb[0], cb[0] - xn, (cb[hi] - cb[lo]) / 2)
    delta = (e_x + xn.abs() * esb) / (sb - esb).clamp_min(1e-300) + U_DIV * xn.abs()
    return s, e_s, h * sb + esb + sb * delta

"""Element-wise error bounds for the kernels between the model's output and the next step's weights: the noise mix and the losses (elementwise.hip), the
rank-space LoRA gradients (skinny.hip), gradient norm / clip / clamp, AdamW, EMA and the LoRA operand packer (optim.hip), against an fp64 reference of the SAME
stored inputs (bf16 or fp32 values, exact in fp64; fp32 scalars as the host rounds them).

Where the bounds come from.  The kernels compute in fp32, u = 2^-24 per rounding; sqrtf and a division are given 4 u each (as norm_bounds gives rsqrtf).  The
library is built with -ffp-contract=fast: a fused multiply-add rounds once where the bound counts two roundings, never more.  A sum taken along a tree whose longest
chain has L additions is off by at most L u sum|terms|; L is read off the kernel's tree.  A bf16 output gets tol = 1/2 ulp_bf16(|ref| + e) + e (GB.check), an
fp32 output gets e alone, plus its own last rounding u |ref| (NB.check_f32 adds it); fp32 SUMS also keep NB.check_f32's block statistic RMS(min(err / e, 4)) <= 0.5.
No number below is fitted to a kernel's output.

skinny (k_skinny_tn_mfma<32 | 64 | 128>, k_skinny_reduce[_multi]).  Products of bf16 values are exact in fp32.  One workgroup accumulates the mc rows of its chunk
in order: one addition per row (the MFMA takes 16 rows per instruction and its internal order is unspecified; any order of 16 is within 16 of the chain).  The
reduce sums cdiv(nchunks, 4) partials per lane, then 2 shuffle adds, then one multiply by alpha and, when accumulating, one add onto the prior:
    e = (mc + cdiv(nchunks, 4) + 4) u |alpha| (|L|^T |R|) + u |prior|
mc and nchunks are the launcher's own (ops.skinny_plan -> st355_skinny_plan).  alpha is the fp32 value the ABI receives.

loss per sample (k_mse, k_cond_loss<1 | 2>, k_mse_finalize).  A thread adds 8 elements per 16-byte vector and cdiv(vecs, 1024) vectors, then wave_sum (6), then the
16 wave partials in order:  L = 8 cdiv(vecs, 1024) + 22.  The sum is multiplied by w and by the fp32 1 / per_sample (one division, two products: 6 u).  The batch
mean adds the B per-sample values in order and divides: (B + 4) u.
  d = pred - target is ONE fp32 rounding, e_d = u |d| (it is exact only when the exponents lie within 16 of each other; the rounding is carried, not assumed away).
  l2 term d^2 m: 2 e_d |d| m + 2 u |term| = 4 u |term|.
  huber / smooth_l1 term k (r - c) m, r = sqrt(d^2 + c^2), k = 2c | 2: c^2, d, d^2 and the add put at most 4 u (relative) on the radicand, the root halves it and
  sqrtf adds 4 u: r is off by 6 u r.  The subtraction r - c cancels, so the term's error is ABSOLUTE in r:  |k m| 6 u r + 4 u |term| (r - c, k, the two products).
  It is bounded as the expression is written, not relative to the term.  What that allows: at |d| << c the term is k d^2 / (2 c) while its bound is 6 u k c, a
  relative error of 12 u (c / d)^2 — 0.72 (72 %) of the per-sample loss for a sample whose residuals ALL sit at |d| = 1e-3 c, and the loss stops resolving at
  |d| ~ 3.5 u^(1/2) c = 8.5e-4 c.  (d^2 / (r + c) is the cancellation-free form, should the kernel ever miss this bound.)
dpred: a short fp32 product / quotient, rounded once to bf16: e = 8 u |ref|.  The 8 u is the figure the issue behind this module sets for all three losses, kept
  as set, not a count: l2's dscale w d m is e_d and three products, 4 u; huber / smooth_l1's 0.5 dscale w k d / r m counts, by the rules above, e_d, 6 u on r,
  4 u for the division and four rounded products (0.5 dscale and k = 2 c | 2 are exact), 15 u, so there 8 u is TIGHTER than the count.  Either is dwarfed by the
  bf16 half-ulp (2^-9 |ref| = 2^15 u |ref|) that GB.check adds, so e only decides elements within 2^-12 of a bf16 tie.  dscale = grad_scale * 2 / (per_sample * B)
  is formed in fp32 on the host; dscale32() mirrors that and the fp64 reference uses the fp32 value.

noise mix.  x_t = (1 - s) x + s n: 1 - s, two products, one add: e = 3 u (|1 - s| |x| + |s n|); ddpm's a x + s n and a n - s x likewise.  The flow target n - x is one
fp32 rounding, e = u |n - x|.  With generated noise x_t and the target are chained on the kernel's own stored noise_out.

grad_norm (k_grad_norm, k_grad_norm_final).  blocks = min(cdiv(n, 256), 1024); a thread's chain is cdiv(n, 256 blocks), then wave_sum (6), the 4 waves in order, then
cdiv(blocks, 64) partials per lane and wave_sum (6); each square is one more rounding:  e = (L + 1) u sum g^2.  The maximum is exact (bit-compared).
grad_clip_norm: chained on the statistics the kernel stored.  coef = min(1, max_norm / (sqrtf(ss) pre_scale + 1e-6)) in fp64 from the stored fp32 ss: sqrtf 4 u, one
  product, one add, the division 4 u: e_coef = 10 u coef.  Then one product (u) and the output rounding.  coef >= 1 must leave every element's bits alone.

AdamW, one step from a given state (adam_one).  step_size = fp32(lr / (1 - b1^step)) and bc2_sqrt = fp32(sqrt(1 - b2^step)) are rounded as make_adam does; the error is
carried through the expression in order:
    g' = g grad_scale                                  e_g = u |g'|
    p1 = p (1 - lr wd)                                 e_p1 = 3 u |p1|                                     (lr wd, 1 - ., the product)
    m' = m + (g' - m)(1 - b1)                          e_m = (1 - b1) e_g + 3 u (1 - b1) |g' - m| + u |m'|  (the difference, 1 - b1, the product; the add)
    v' = v b2 + (1 - b2) g' g'                         e_v = u |v b2| + (1 - b2)(2 |g'| e_g + 3 u g'^2) + u |v'|
    sq = sqrtf(v')                                     e_sq = e_v / (sqrt(v') + sqrt(v' + e_v)) + 4 u sq   (finite at v' = 0: there e_v = 0 too)
    denom = sq / bc2_sqrt + eps                        e_den = e_sq / bc2_sqrt + 4 u sq / bc2_sqrt + u denom
    p' = p1 - step_size (m' / denom)                   e_p = e_p1 + step_size (e_m / denom + |m'| e_den / denom^2 + 4 u |m' / denom|) + u |upd| + u |p'|
m', v', p' are fp32 outputs (tol = e); the bf16-parameter kernel rounds p' once more (RNE): tol = 1/2 ulp_bf16(|p'| + e_p) + e_p.  p_bf16 is one RNE of the
stored fp32 parameter (bit-compared).  The fp32 EMA  s - omd (s - p')  is chained on the stored new parameter: omd = 1.f - decay as fp32 forms it, the difference,
the product and the subtraction: e = 2 u omd |s - p'| (+ the output rounding).  The bf16 EMA materialises (s - p') in bf16 as the kernel states — bf16(fp32(s - p')),
reproduced exactly — and then e = 2 u (|s| + omd |diff|) under one RNE.  ema_update is the same two expressions.
lora_pack is one RNE of A or of the fp32 product scale * B: bit-compared with GB.to_bf16_rne.  adamw_bf16_sr_step is bit-compared with oracle.train_math.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import gemm_bounds as GB
from tests import norm_bounds as NB

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
U = 2.0 ** -24
U_SQRT = 4 * U
U_DIV = 4 * U
COLS = 1024            # flat arenas are checked as [rows, COLS] matrices (the checkers' blocks are 64 x 64)

cdiv = NB.cdiv


def f32(x):
    """the fp32 value a float argument takes when it crosses the C ABI"""
    return float(np.float32(x))


# ---- chain lengths ------------------------------------------------------------------------------------------------------------------------------------
def L_skinny(mc, nchunks):
    return mc + cdiv(nchunks, 4) + 4


def L_loss(per_sample):
    return 8 * cdiv(per_sample // 8, 1024) + 22


def grad_norm_blocks(n):
    return min(cdiv(n, 256), 1024)


def L_grad_norm(n):
    b = grad_norm_blocks(n)
    return cdiv(n, b * 256) + 6 + 4 + cdiv(b, 64) + 6


# ---- flat views ---------------------------------------------------------------------------------------------------------------------------------------
def as2d(t, cols=COLS):
    """a flat tensor as [rows, cols], zero-padded (out = want = e = 0 on the padding: err / tol = 0)"""
    f = t.reshape(-1)
    pad = (-f.numel()) % cols
    if pad:
        f = torch.cat([f, torch.zeros(pad, dtype=f.dtype, device=f.device)])
    return f.view(-1, cols)


def check_bf16(name, out, want, e, flat=False, verbose=True):
    """a bf16 output under GB.check (element bound and 64 x 64 block RMS)"""
    if flat:
        out, want, e = as2d(out), as2d(want.to(F64)), as2d(e.to(F64))
    return GB.check(name, out, want.to(F64), e.to(F64), verbose=verbose)


def check_sum(name, out, want, e, verbose=True):
    """an fp32 SUM: element bound and block statistic (NB.check_f32)"""
    return NB.check_f32(name, out, want, e, verbose=verbose)


def check_f32(name, out, want, e, flat=True, verbose=True):
    """an fp32 output that is not a sum: |out - want| <= e + u |want| element-wise (NB.check_f32 without its block statistic)"""
    if flat:
        out, want, e = as2d(out), as2d(want.to(F64)), as2d(e.to(F64))
    rep = NB.check_f32(name, out, want, e, verbose=False)
    rep.block_rms = 0.0
    if verbose:
        print(f"[bound] {name}: worst err/tol={rep.worst:.3f} at {rep.worst_at}; {rep.n} outputs")
    return rep


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ---- skinny -------------------------------------------------------------------------------------------------------------------------------------------
def skinny(Lm, R, alpha, mc, nchunks, prior=None):
    """Lm [M, P], R [M, r] (the logical rows, gathered; only the r_used columns): want [P, r], e"""
    l, r = Lm.to(F64), R.to(F64)
    a = f32(alpha)
    want = a * (l.t() @ r)
    e = L_skinny(mc, nchunks) * U * abs(a) * (l.abs().t() @ r.abs())
    if prior is not None:
        want = want + prior.to(F64)
        e = e + U * prior.to(F64).abs()
    return want, e


# ---- losses -------------------------------------------------------------------------------------------------------------------------------------------
def dscale32(grad_scale, per_sample, B):
    """grad_scale * 2.0f / ((float)per_sample * (float)batch), every operation in fp32 as the launcher forms it"""
    return float(np.float32(grad_scale) * np.float32(2.0) / (np.float32(per_sample) * np.float32(B)))


def loss(pred, target, loss_type, huber_c=None, weight=None, emask=None, grad_scale=1.0):
    """pred / target [B, per_sample] (bf16 values); huber_c / weight [B] fp32 or None; emask [B, period] fp32 or None (repeats over per_sample / period channels).
    Returns dict: per_sample (want, e), loss (want, e), dpred (want, e)."""
    p, t = pred.to(F64), target.to(F64)
    B, n = p.shape
    w = torch.ones(B, dtype=F64, device=p.device) if weight is None else weight.to(F64)
    if emask is None:
        m = torch.ones_like(p)
    else:
        m = emask.to(F64).reshape(B, 1, -1).expand(B, n // emask.shape[-1], emask.shape[-1]).reshape(B, n)
    d = p - t
    L = L_loss(n)
    ds = dscale32(grad_scale, n, B)
    if loss_type == "l2":
        term = d * d * m
        e_term = 4 * U * term.abs()
        dp = ds * w[:, None] * d * m
    else:
        c = huber_c.to(F64)[:, None]
        k = 2.0 * c if loss_type == "huber" else torch.full_like(c, 2.0)
        r = torch.sqrt(d * d + c * c)
        term = k * (r - c) * m
        e_term = (k * m).abs() * 6 * U * r + 4 * U * term.abs()
        dp = 0.5 * ds * w[:, None] * k * d / r * m
    s = term.sum(1)
    ps = w * s / n
    e_ps = w.abs() / n * (L * U * term.abs().sum(1) + e_term.sum(1)) + 6 * U * ps.abs()
    lo = ps.mean()
    e_lo = (e_ps + U * ps.abs()).mean() + (B + 4) * U * ps.abs().mean()
    return {"per_sample": (ps, e_ps), "loss": (lo.reshape(1), e_lo.reshape(1)), "dpred": (dp, 8 * U * dp.abs())}


# ---- noise mix ----------------------------------------------------------------------------------------------------------------------------------------
def flow_mix(x, noise, sigma):
    """x / noise [B, per_sample]; sigma [B] fp32.  Returns (x_t want, e), (target want, e)"""
    xd, nd, s = x.to(F64), noise.to(F64), sigma.to(F64)[:, None]
    a, b = (1 - s) * xd, s * nd
    tg = nd - xd
    return (a + b, 3 * U * (a.abs() + b.abs())), (tg, U * tg.abs())


def ddpm_mix(x, noise, sa, ss):
    xd, nd, a, s = x.to(F64), noise.to(F64), sa.to(F64)[:, None], ss.to(F64)[:, None]
    return (a * xd + s * nd, 3 * U * ((a * xd).abs() + (s * nd).abs())), (a * nd - s * xd, 3 * U * ((a * nd).abs() + (s * xd).abs()))


# ---- gradient norm / clip ---------------------------------------------------------------------------------------------------------------------------------
def grad_norm(g):
    gd = g.to(F64).reshape(-1)
    ss = (gd * gd).sum()
    return ss.reshape(1, 1), ((L_grad_norm(gd.numel()) + 1) * U * ss).reshape(1, 1), gd.abs().max()


def clip_coef(ss_stored, max_norm, pre_scale):
    """coef (python float) in fp64 from the STORED fp32 sum of squares; the fp32 scalars as the ABI receives them"""
    norm = math.sqrt(float(ss_stored)) * f32(pre_scale)
    return min(f32(max_norm) / (norm + f32(1e-6)), 1.0)


def grad_clip(g, coef):
    want = g.to(F64) * coef
    return want, (10 * U + U) * want.abs()


# ---- AdamW / EMA ------------------------------------------------------------------------------------------------------------------------------------------
def adam_consts(lr, beta1, beta2, eps, wd, step, grad_scale, ema_decay):
    """make_adam: every scalar as fp32, step_size and bc2_sqrt from double arithmetic on those fp32 values, rounded to fp32"""
    lr, b1, b2, eps, wd, gs = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd), f32(grad_scale)
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, gs=gs, step_size=f32(lr / bc1), bc2_sqrt=f32(math.sqrt(bc2)),
                omd=float(np.float32(1.0) - np.float32(ema_decay)))


def adamw(p, g, m, v, c):
    """one adam_one from (p, g, m, v) (fp64-able, flat); c = adam_consts(...).  Returns dict name -> (want, e) for m, v, p"""
    p, g, m, v = p.to(F64), g.to(F64), m.to(F64), v.to(F64)
    omb1, omb2 = 1.0 - c["b1"], 1.0 - c["b2"]
    g1 = g * c["gs"]
    e_g = U * g1.abs()
    p1 = p * (1.0 - c["lr"] * c["wd"])
    e_p1 = 3 * U * p1.abs()
    m1 = m + (g1 - m) * omb1
    e_m = omb1 * e_g + 3 * U * omb1 * (g1 - m).abs() + U * m1.abs()
    v1 = v * c["b2"] + omb2 * g1 * g1
    e_v = U * (v * c["b2"]).abs() + omb2 * (2 * g1.abs() * e_g + 3 * U * g1 * g1) + U * v1.abs()
    sq = torch.sqrt(v1)
    e_sq = e_v / (sq + torch.sqrt(v1 + e_v)).clamp_min(1e-300) + U_SQRT * sq
    q = sq / c["bc2_sqrt"]
    denom = q + c["eps"]
    e_den = e_sq / c["bc2_sqrt"] + U_DIV * q + U * denom
    ratio = m1 / denom
    upd = c["step_size"] * ratio
    p2 = p1 - upd
    e_p = e_p1 + c["step_size"] * (e_m / denom + m1.abs() * e_den / (denom * denom) + U_DIV * ratio.abs()) + U * upd.abs() + U * p2.abs()
    return {"m": (m1, e_m), "v": (v1, e_v), "p": (p2, e_p)}


def ema_f32(s, p_stored, omd):
    s, p = s.to(F64), p_stored.to(F64)
    d = s - p
    return s - omd * d, 2 * U * omd * d.abs()


def ema_bf16(s, p_stored, omd):
    """(s - p) materialised in bf16: bf16(fp32(s - p)), which GB.to_bf16_rne reproduces bit for bit"""
    s, p = s.to(F64), p_stored.to(F64)
    d = GB.to_bf16_rne(s - p).to(F64)
    return s - omd * d, 2 * U * (s.abs() + omd * d.abs())

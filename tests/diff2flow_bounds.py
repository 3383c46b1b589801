"""Element-wise error bounds of the Diff2Flow loss kernel (csrc/diff2flow.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernel's arithmetic, never from what it returns.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u): the
relative error of an fp32 sum of n terms in ANY order.  The bf16 inputs (p, x, tau) are exact in fp32; the table entries (c0, c1), the mask m and the row weight w
are fp32 numbers, so reading them costs no rounding.  The counts hold with or without fused multiply-adds (a fused pair rounds once instead of twice);
SLACK = 1 + 2^-10 covers the second-order terms.  The timestep is clamped to [0, T - 1] on both sides.

per element, the kernel's expression:
    A = c0 x, Bp = c1 p: one rounding each;  z = A - Bp:                    e_z = u (|A| + |Bp|) + u |z|
    epsilon:  f = p - z:                                                    e_f = e_z + u |f|
    v:        C = c0 p, D = c1 x, e = C + D:  e_e = u (|C| + |D|) + u |e|;  f = e - z:  e_f = e_e + e_z + u |f|
    d = f - tau:                                                            e_d = e_f + u |d|
    (the cancellations — z against p, e against z, f against tau — are counted absolutely: every e_* carries the magnitudes of the terms that cancel)
    the summand s = (d d) m:                                                e_s = (2 |d| e_d + e_d^2) m + 2 u d^2 m
the two-stage sum: each of the n terms takes part in at most n + 64 additions (the lane's run, 6 butterfly steps, 4 wave partials, the stage-2 partials):
    |S - S64| <= sum e_s + gamma(n + 64) sum |s|
per_sample = (S w) (1 / n): 1 / n one rounding, two products: 3 u.   loss = (sum_b per_sample) / B in sample order: gamma(B + 1).
dpred = gcoef d m,  gcoef = ((2 grad_scale / (n B)) w) k:  n B and the division on the host: 2 u;  k = 1 + c1 or c0 + c1: u;  the two products: 2 u;  then d and m:
    2 u  ->  e32 = |gcoef m| e_d + GRAD_ROUNDINGS u |dpred|, GRAD_ROUNDINGS = 8 (7 counted, 1 spare);  then ONE bf16 rounding:  tol = e32 + ub (|dpred64| + e32)

`rounds` widens the gradient count for a reference whose gradient comes from another fp32 chain of operations (torch autograd through the bridge's expression:
mse backward 2 (a - b) g: 3 u; the mask: u; the two mean backwards: 2 u; the product with c1 (and c0): 2 u; the accumulation of the two paths: u; the subtraction
nodes pass the gradient on unrounded: 9, taken as 12), and out_bf16=False leaves the bf16 rounding out for a gradient kept in fp32.
"""
import torch

from tests import diff2flow_ref as DR

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10
GRAD_ROUNDINGS = 8
AUTOGRAD_ROUNDINGS = 12


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def loss_ref(pred, noisy, tau, timesteps, table, mode, emask=None, weight=None, grad_scale=1.0, rounds=GRAD_ROUNDINGS, out_bf16=True):
    """fp64 on the given operands: {name: (reference, bound)} for loss, per_sample, dpred"""
    r = DR.closed64(pred, noisy, tau, timesteps, table, mode, emask, weight, grad_scale)
    B = pred.shape[0]
    p, x = DR._flat(pred, B), DR._flat(noisy, B)
    N = p.shape[1]
    c0, c1, d, m, w, k = r["c0"], r["c1"], r["d"], r["m"], r["w"], r["k"]
    A, Bp = (c0 * x).abs(), (c1 * p).abs()
    z = c0 * x - c1 * p
    e_z = U * (A + Bp) + U * z.abs()
    if mode == "epsilon":
        f = p - z
        e_f = e_z + U * f.abs()
    else:
        C, D = (c0 * p).abs(), (c1 * x).abs()
        e = c0 * p + c1 * x
        f = e - z
        e_f = U * (C + D) + U * e.abs() + e_z + U * f.abs()
    e_d = SLACK * (e_f + U * d.abs())
    s = d * d * m
    e_s = (2 * d.abs() * e_d + e_d * e_d) * m.abs() + 2 * U * s.abs()
    e_sum = e_s.sum(1) + gamma(N + 64) * s.abs().sum(1)
    per = r["per_sample"]
    e_per = SLACK * (e_sum * w[:, 0].abs() / N + 3 * U * per.abs())
    e_loss = SLACK * (e_per.sum() / B + gamma(B + 1) * per.abs().sum() / B)
    g = r["dpred"].reshape(B, N)
    gcoef = (2.0 * grad_scale / (N * B)) * w * k
    e32 = SLACK * ((gcoef * m).abs() * e_d + rounds * U * g.abs())
    tol = e32 + UB * (g.abs() + e32) if out_bf16 else e32
    return {"loss": (r["loss"], e_loss + TINY), "per_sample": (per, e_per + TINY), "dpred": (r["dpred"], (tol + TINY).reshape(pred.shape))}


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

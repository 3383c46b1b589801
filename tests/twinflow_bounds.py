"""Element-wise error bounds of the TwinFlow kernels (csrc/twinflow.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u): the
relative error of an fp32 sum of n terms in ANY order.  A bf16 number is exact in fp32; sqrtf is correctly rounded.  The counts hold with or without fused
multiply-adds (a fused pair rounds once instead of twice); SLACK = 1 + 2^-10 covers the second-order terms.  The scalar parameters the tests pass (ratio, clamp,
grad_scale, s_cur, s_next, rho) are fp32 numbers, so passing them costs no rounding.  clamp() is 1-Lipschitz, so an element whose r sits next to +-clamp moves by
no more than r's own error whichever branch a rounding puts it in: no assertion about inputs near the kink is needed.

st355_twinflow_rcgm_step   h = t_next - t_prev: u;  h f: u  ->  e_hf = 2 u |h f|
    x' = bf16(x + h f):     e32 = e_hf + u (|y| + e_hf),  tol = e32 + ub (|y| + e32)                       y = x + h f in fp64
    acc' = acc + (-h) f:    tol = e_hf + u (|a| + e_hf)   (first: acc is taken as 0 and the sum is exact: tol = e_hf)     a = acc - h f in fp64

st355_twinflow_loss        t' = t + ratio (c - uu):  c - uu: u;  the product: u;  the sum: u  ->  e_t = 2 u |ratio (c - uu)| + u |t'|     (no pair: t' = t, e_t = 0)
    d = p - t': e_d = e_t + u |d|;   r = d - acc: e_r = e_d + u |r|;   rc = clamp(r): e_rc = e_r
    summands rc^2: 2 |rc| e_rc + e_rc^2 + u rc^2;   d^2: 2 |d| e_d + e_d^2 + u d^2
    each summand takes part in at most n_add = per_sample + 10 + max(2048, B) additions (the lane's run, 6 butterfly steps, 4 wave partials, and in stage 2 a run of
    ceil(B * parts / 256) partials plus the 256 run sums: at most max(2048, B), as B * parts <= max(2048, B)): + gamma(n_add) sum |summand|;   the mean (1 / n rounded: u, the product: u): 2 u
    dpred = gscale (rc + d):  the sum: e_rc + e_d + u |rc + d|;  gscale = fp32(grad_scale 2 / n): u;  the product: u;  then ONE bf16 rounding

st355_twinflow_ucgm_step   x_hat = x - s_cur f: e_xh = u |s_cur f| + u |x_hat|;   g_cur = 1 - s_cur: u;   z_hat = x + g_cur f: e_zh = 2 u |g_cur f| + u |z_hat|
    q_keep = sqrtf(1 - rho): 2 u;  q_noise = sqrtf(rho): u
    z = z_hat q_keep + noise q_noise: e_z = q_keep e_zh + 3 u |z_hat q_keep| + 2 u |noise q_noise| + u |z|
    g_next = 1 - s_next: u;   y = g_next x_hat + s_next z: e32 = g_next e_xh + 2 u |g_next x_hat| + s_next e_z + u |s_next z| + u |y|;  then bf16
"""
import torch

from tests import twinflow_ref as TR

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def _c(t):
    return t.detach().to(F64).cpu()


def rcgm_step_ref(x, acc, fc, t_prev, t_next, first):
    """{x: (reference, bound), acc: (reference, bound)} of ONE step on the given operands (taken before the in-place call)"""
    xs, f = _c(x), _c(fc)
    h = (_c(t_next) - _c(t_prev)).reshape(-1, *([1] * (x.dim() - 1)))
    hf = (h * f).abs()
    e_hf = 2 * U * hf
    y = xs + h * f
    e32 = SLACK * (e_hf + U * (y.abs() + e_hf))
    a = -h * f if first else _c(acc) - h * f
    e_a = SLACK * (e_hf if first else e_hf + U * (a.abs() + e_hf))
    return {"x": (y, e32 + UB * (y.abs() + e32) + TINY), "acc": (a, e_a + TINY)}


def loss_ref(pred, target, acc, cond=None, uncond=None, ratio=0.0, clamp=1.0, grad_scale=1.0):
    """{losses: (reference [2], bound [2]), dpred: (reference, bound), clamped: fraction of elements the fp64 reference clamps}"""
    ref = TR.twinflow64(pred, target, acc, cond, uncond, ratio, clamp, grad_scale)
    p, t, a = _c(pred), _c(target), _c(acc)
    B = p.shape[0]
    n, per = p.numel(), p.numel() // B
    if cond is not None:
        k = float(ratio) * (_c(cond) - _c(uncond))
        t = t + k
        e_t = 2 * U * k.abs() + U * t.abs()
    else:
        e_t = torch.zeros_like(p)
    d = p - t
    e_d = e_t + U * d.abs()
    r = d - a
    e_r = e_d + U * r.abs()
    rc = r.clamp(min=-float(clamp), max=float(clamp))
    n_add = per + 10 + max(2048, B)
    out = []
    for v, e in ((rc, e_r), (d, e_d)):
        sq = v * v
        e_sum = (2 * v.abs() * e + e * e + U * sq).sum() + gamma(n_add) * sq.sum()
        out.append(SLACK * (e_sum / n + 2 * U * sq.sum() / n))
    g = float(grad_scale) * 2.0 / n
    e32 = SLACK * (abs(g) * (e_r + e_d + U * (rc + d).abs()) + 2 * U * ref["dpred"].abs())
    return {"losses": (ref["losses"], torch.stack(out) + TINY), "dpred": (ref["dpred"], e32 + UB * (ref["dpred"].abs() + e32) + TINY), "clamped": ref["clamped"]}


def ucgm_step_ref(x, v, s_cur, s_next, rho, noise=None):
    """(reference, bound) on the given operands (taken before the in-place call); the scalars are fp32 numbers"""
    xs, f = _c(x), _c(v)
    has_n = noise is not None and rho != 0.0
    nz = _c(noise) if has_n else torch.zeros_like(xs)
    g_cur, g_next, qk, qn = 1 - s_cur, 1 - s_next, (1 - rho) ** 0.5, rho ** 0.5
    x_hat, z_hat = xs - s_cur * f, xs + g_cur * f
    e_xh = U * (s_cur * f).abs() + U * x_hat.abs()
    e_zh = 2 * U * (g_cur * f).abs() + U * z_hat.abs()
    z = z_hat * qk + nz * qn
    e_z = qk * e_zh + 3 * U * (z_hat * qk).abs() + 2 * U * (nz * qn).abs() + U * z.abs()
    y = g_next * x_hat + s_next * z
    e32 = SLACK * (abs(g_next) * e_xh + 2 * U * (g_next * x_hat).abs() + abs(s_next) * e_z + U * (s_next * z).abs() + U * y.abs())
    return y, e32 + UB * (y.abs() + e32) + TINY


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

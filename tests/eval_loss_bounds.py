"""Element-wise error bounds of the evaluation-loss kernels (csrc/eval_loss.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u): the
relative error of an fp32 sum of n terms in ANY order.  A bf16 number is exact in fp32; sqrtf is correctly rounded.  The counts hold with or without fused
multiply-adds (a fused pair rounds once instead of twice); SLACK = 1 + 2^-10 covers the second-order terms.

st355_eval_flow_views      g = 1 - s: u;  g x: u  ->  2 u |g x|;   s n: u |s n|;   the sum: u |y|            y = (1 - s) x + s n in fp64
    e32 = 2 u |g x| + u |s n| + u |y|,   out = bf16(...):  tol = e32 + ub (|y| + e32)

st355_eval_loss            d = p - t: two bf16 numbers whose exponents may differ by more than 16, so the fp32 difference rounds: e_d = u |d|
    l2         summand d^2:  e = 2 |d| e_d + e_d^2 + u d^2
    huber /    c2 = c c: u c^2;   q = d d + c2:  e_q = (2 |d| e_d + e_d^2 + u d^2) + u c^2 + u q
    smooth_l1  r = sqrtf(q): |sqrt(q') - sqrt(q)| <= e_q / (2 sqrt(max(q - e_q, tiny))), then u r:  e_r;   r - c: e_rc = e_r + u |r - c|   (the cancellation for |d| << c
               is carried by the ABSOLUTE terms u c^2 / (2 c) and u r: no relative claim is made about r - c)
               scale = 2 c (exact: a power-of-two multiple) or 2;   summand scale (r - c):  e = scale e_rc + u |summand|
    each summand takes part in at most n_add = per_sample + 10 + 2048 additions (the lane's run, 6 butterfly steps, 4 wave partials, at most 2048 partials of the
    sample in stage 2): + gamma(n_add) sum |summand|;   per_sample = sum * fp32(1 / n): 2 u
    loss[k] = (sum_b per_sample[k, b]) / B:  B - 1 additions and one division: gamma(B) sum_b |per_sample| + sum_b e_per
"""
import torch

from tests import eval_loss_ref as ER

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def _c(t):
    return t.detach().to(F64).cpu()


def views_ref(latents, noise, sigma):
    """(reference [K, B, ...], bound) on the given operands"""
    x, n = _c(latents)[None], _c(noise)[None]
    s = _c(sigma).reshape(-1, *([1] * (x.dim() - 1)))
    y = ER.views64(latents, noise, sigma)
    e32 = SLACK * (2 * U * ((1.0 - s) * x).abs() + U * (s * n).abs() + U * y.abs())
    return y, e32 + UB * (y.abs() + e32) + TINY


def loss_ref(pred, target, loss_type="l2", huber_c=None):
    """{loss: (reference [K], bound [K]), per_sample: (reference [K, B], bound [K, B])}"""
    ref_loss, ref_per = ER.loss64(pred, target, loss_type, huber_c)
    p, t = _c(pred), _c(target)
    K, B = p.shape[0], t.shape[0]
    per = t.numel() // B
    d = p - t[None]
    e_d = U * d.abs()
    e_sq = 2 * d.abs() * e_d + e_d * e_d + U * d * d
    if loss_type == "l2":
        summand, e = d * d, e_sq
    else:
        c = (_c(huber_c) if torch.is_tensor(huber_c) else torch.full((K * B,), float(torch.tensor(float(huber_c), dtype=torch.float32)), dtype=F64))
        c = c.reshape(K, B, *([1] * (t.dim() - 1)))
        q = d * d + c * c
        e_q = e_sq + U * c * c + U * q
        r = torch.sqrt(q)
        e_r = e_q / (2.0 * torch.sqrt((q - e_q).clamp_min(TINY))) + U * r
        e_rc = e_r + U * (r - c).abs()
        scale = 2.0 * c if loss_type == "huber" else torch.full_like(c, 2.0)
        summand = scale * (r - c)
        e = scale * e_rc + U * summand.abs()
    n_add = per + 10 + 2048
    s_abs = summand.abs().reshape(K, B, -1).sum(dim=2)
    e_sum = e.reshape(K, B, -1).sum(dim=2) + gamma(n_add) * s_abs
    e_per = SLACK * (e_sum / per + 2 * U * s_abs / per)
    e_loss = SLACK * ((e_per.sum(dim=1) + gamma(B) * ref_per.abs().sum(dim=1)) / B)
    return {"loss": (ref_loss, e_loss + TINY), "per_sample": (ref_per, e_per + TINY)}


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

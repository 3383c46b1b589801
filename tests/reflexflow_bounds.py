"""Element-wise error bounds of the ReflexFlow kernels (csrc/reflexflow.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u): the
relative error of an fp32 sum of n terms in ANY order.  A product of two bf16 numbers is exact in fp32.  sqrtf and the fp32 division are correctly rounded.  The
counts below hold with or without fused multiply-adds (a fused pair rounds once instead of twice); SLACK = 1 + 2^-10 covers the second-order terms.  The scalar
parameters of the tests (alpha, beta1, beta2, grad_scale, huber_c) are fp32 numbers, so passing them costs no rounding; the clamp constant is 1e-6f in the kernel
and 1e-6 in fp64 (relative distance < u: counted in the 3 u of the reciprocals).

st355_flow_euler_step   y = x + h v:  h v one rounding (or none, fused), the sum one, then bf16:
    |x' - y| <= e32 + ub (|y| + e32),  e32 = u |h v| + u (|y| + u |h v|)

st355_reflexflow_stats  terms |c - b| (1 rounding), p p (exact), tau tau (tau: 1, product: 1 -> 3 u), p tau (2 u); each of the N terms takes part in at most
    N + 64 additions (the lane's run, 6 butterfly steps, 4 wave partials, the stage-2 partials):
    |S_k - S_k64| <= [c_k u + gamma(N + 64) (1 + c_k u)] sum |term_k|,  c = (1, 0, 3, 2)

st355_reflexflow_loss   against fp64 ON THE GIVEN fp32 STATS.  Per sample, from the stats:
    e_scale = alpha / max(S_e, 1e-6): u;  pn, tn: sqrt u, clamp;  1 / pn, 1 / tn: 3 u each;
    udot = pp / pn^2 - pt / (pn tn) =: A - Bt:  each product chain 7 u, the difference u:  |udot - udot64| <= 8 u (|A| + |Bt|) =: e_udot
    gcoef = (grad_scale 2 beta1 / B) / pn: 7 u;  dscale = grad_scale / (N B): 2 u
  per element (d = p - t: u):
    l2:     l = d d: 3 u |l|;  g = 2 d: u |g|
    huber:  s = d d + c c: 4 u;  r = sqrt s: 3 u;  l = k (r - c): |l - l64| <= k 3 u r + 3 u |l|  (the cancellation in r - c is counted absolutely);  g = k d / r: 6 u |g|
    w = (beta2 m) (1 + e_scale e):  x = 1 + e_scale e with |x - x64| <= 3 u |e_scale e| + u |x| =: e_x;  |w - w64| <= |beta2 m| e_x + 2 u |w64| =: e_w
    the summand l w: |.| <= e_l |w| + |l| e_w + u |l w|;  the sum over N: + gamma(N + 64) sum |l w|;  the mean: 2 u
    ADR: uu = p / pn: 3 u;  th = tau / tn: 4 u;  q = uu - th: e_q = 3 u |uu| + 4 u |th| + u |q|;  q q: 2 |q| e_q + u q^2;  sum: gamma(N + 64);  beta1: u;  the add: u
    dpred = dscale g w + gcoef (q - uu udot):
        main: |dscale g| e_w + 10 u |main|;   v = q - uu udot: e_v = e_q + |uu| e_udot + 4 u |uu udot| + u |v|;   gcoef v: |gcoef| e_v + 8 u |gcoef v|;   the add: u
        then ONE bf16 rounding:  tol = e32 + ub (|dpred64| + e32)
    loss = mean_b per_sample in sample order: gamma(B + 1)

No assertion about |d| near a kink: the smooth_l1 built here is the reference's 2 (sqrt(d^2 + c^2) - c) (common.py:6158-6159), smooth everywhere, so no input sits at a
point where a rounding of d switches branches; what the form does have, the cancellation in r - c for |d| << c, is counted absolutely in e_l above.  check_inputs
therefore asserts only the clamp condition: every |p|, |tau| and sum |e| is exactly 0 or at least 1e-2.
"""
import torch

from tests import reflexflow_ref as RR

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def euler_ref(x, v, dt):
    y = RR.euler64(x, v, dt).cpu()
    B = x.shape[0]
    hv = (dt.detach().to(F64).reshape(B, *([1] * (x.dim() - 1))) * v.detach().to(F64)).abs().cpu()
    e32 = SLACK * (U * hv + U * (y.abs() + U * hv))
    return y, e32 + UB * (y.abs() + e32) + TINY


def stats_ref(pred, noisy, latents, clean=None, biased=None):
    """(reference [B, 4], bound [B, 4])"""
    p, tau = RR._flat(pred).cpu(), (RR._flat(noisy) - RR._flat(latents)).cpu()
    N = p.shape[1]
    e = (RR._flat(clean) - RR._flat(biased)).abs().cpu() if clean is not None else torch.zeros_like(p)
    mags = torch.stack([e.sum(1), (p * p).sum(1), (tau * tau).sum(1), (p * tau).abs().sum(1)], dim=1)
    ref = RR.stats64(pred, noisy, latents, clean, biased).cpu()
    c = torch.tensor([1.0, 0.0, 3.0, 2.0], dtype=F64)
    return ref, SLACK * (c * U + gamma(N + 64) * (1 + c * U)) * mags + TINY


def loss_ref(pred, target, noisy, latents, stats, clean=None, biased=None, loss_type="l2", huber_c=0.1, emask=None, alpha=1.0, beta1=10.0, beta2=1.0, grad_scale=1.0):
    """fp64 on the given operands and the given fp32 stats: {name: (reference, bound)} for loss, per_sample, adr, dpred"""
    cpu = lambda t: None if t is None else t.detach().cpu()
    pred, target, noisy, latents, stats, clean, biased, emask = map(cpu, (pred, target, noisy, latents, stats, clean, biased, emask))
    huber_c = cpu(huber_c) if torch.is_tensor(huber_c) else huber_c
    ref = RR.reflexflow64(pred, target, noisy, latents, clean, biased, loss_type, huber_c, emask, alpha, beta1, beta2, grad_scale, stats=stats)
    p, t = RR._flat(pred), RR._flat(target)
    B, N = p.shape
    st = stats.to(F64)
    d = p - t
    if loss_type == "l2":
        l, g = d * d, 2 * d
        e_l, e_g = 3 * U * l.abs(), U * g.abs()
    else:
        c = RR._huber(huber_c, B)
        r = torch.sqrt(d * d + c * c)
        k = 2 * c if loss_type == "huber" else torch.full_like(c, 2.0)
        l, g = k * (r - c), k * d / r
        e_l, e_g = k * 3 * U * r + 3 * U * l.abs(), 6 * U * g.abs()
    m = RR._mask_full(emask, B, N)
    w0 = torch.full_like(p, float(beta2)) * (m if m is not None else 1.0)
    has_e = clean is not None and alpha != 0.0
    if has_e:
        ese = alpha * (RR._flat(clean) - RR._flat(biased)) / st[:, 0:1].clamp_min(RR.EPS)
        x = 1.0 + ese
        e_x = 3 * U * ese.abs() + U * x.abs()
    else:
        x, e_x = torch.ones_like(p), torch.zeros_like(p)
    w = w0 * x
    e_w = w0.abs() * e_x + 2 * U * w.abs()
    lw = l * w
    e_sum = (e_l * w.abs() + l.abs() * e_w + U * lw.abs()).sum(1) + gamma(N + 64) * lw.abs().sum(1)
    e_mean = SLACK * (e_sum / N + 2 * U * lw.sum(1).abs() / N)
    dscale = grad_scale / (N * B)
    main = dscale * g * w
    e_grad = (dscale * g).abs() * e_w + abs(dscale) * e_g * w.abs() + 10 * U * main.abs()
    adr, e_adr = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
    if beta1 != 0.0:
        tau = RR._flat(noisy) - RR._flat(latents)
        pnorm, tnorm = st[:, 1:2].sqrt(), st[:, 2:3].sqrt()
        pn, tn = pnorm.clamp_min(RR.EPS), tnorm.clamp_min(RR.EPS)
        uu, th = p / pn, tau / tn
        q = uu - th
        e_q = 3 * U * uu.abs() + 4 * U * th.abs() + U * q.abs()
        A, Bt = st[:, 1:2] / (pn * pn), st[:, 3:4] / (pn * tn)
        live = pnorm > RR.EPS
        udot = torch.where(live, A - Bt, torch.zeros_like(A))
        e_udot = torch.where(live, 8 * U * (A.abs() + Bt.abs()), torch.zeros_like(A))
        qq = (q * q).sum(1)
        adr = beta1 * qq
        e_adr = SLACK * abs(beta1) * ((2 * q.abs() * e_q + U * q * q).sum(1) + gamma(N + 64) * qq + U * qq)
        gcoef = grad_scale * 2.0 * beta1 / (B * pn)
        v = q - uu * udot
        e_v = e_q + uu.abs() * e_udot + 4 * U * (uu * udot).abs() + U * v.abs()
        e_grad = e_grad + gcoef.abs() * e_v + 8 * U * (gcoef * v).abs()
    e_grad = SLACK * (e_grad + U * ref["dpred"].reshape(B, N).abs())
    e_per = e_mean + e_adr + U * ref["per_sample"].abs()
    e_loss = SLACK * (e_per.sum() / B + gamma(B + 1) * ref["per_sample"].abs().sum() / B)
    return {"loss": (ref["loss"], e_loss + TINY), "per_sample": (ref["per_sample"], e_per + TINY), "adr": (ref["adr"], e_adr + U * adr.abs() + TINY),
            "dpred": (ref["dpred"], (e_grad + UB * (ref["dpred"].reshape(B, N).abs() + e_grad) + TINY).reshape(pred.shape))}


def check_inputs(pred, noisy, latents, clean=None, biased=None):
    """what the bounds assume about the test's own inputs: every |p|, |tau|, sum |e| is exactly 0 or at least 1e-2 (never near the 1e-6 clamps)"""
    st = RR.stats64(pred, noisy, latents, clean, biased)
    vals = torch.stack([st[:, 0], st[:, 1].sqrt(), st[:, 2].sqrt()], dim=1)
    return bool(((vals == 0) | (vals >= 1e-2)).all())


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

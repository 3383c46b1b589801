"""Element-wise error bounds of the LCM kernels (csrc/lcm.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u).  The bf16
inputs are exact in fp32; the table entries (a, s), (ap, sp), the guidance scale w and the fp32 x_prev / target are fp32 numbers: reading them costs no rounding.  The
counts hold with or without fused multiply-adds (a fused pair rounds once instead of twice).  A division or a square root is counted as 2 u (one ulp: what the device
guarantees whether or not the correctly rounded expansions are selected).  SLACK = 1 + 2^-10 covers the second-order terms.  Indices are clamped on both sides.

the CFG combine:   dif = pc - pu: u |dif|;  w dif: |w| u |dif| + u |w dif|;  p = pu + w dif:              e_p = u (2 |w dif| + |p|)
x0 / eps at (x, p; a, s), e_p the error already in p (0 for a bf16 prediction):
    epsilon:  sp = s p: s e_p + u |s p|;  num = x - sp: + u |num|;  x0 = num / a:                          e_x0 = (s e_p + u |s p| + u |num|) / a + 2 u |x0|
              — the 1 / a amplification: at the last solver timestep a = 0.068, every absolute error of the numerator (which cancels from |x| + |s p| down to a |x0|) grows 15x
              eps = p:                                                                                     e_eps = e_p
    v:        x0 = a x - s p:                                                                              e_x0 = u |a x| + s e_p + u |s p| + u |x0|
              eps = a p + s x:                                                                             e_eps = a e_p + u |a p| + u |s x| + u |eps|
solver:   x_prev = ap x0 + sp eps:   e = ap e_x0 + u |ap x0| + sp e_eps + u |sp eps| + u |x_prev|;   the bf16 copy: e + ub (|x_prev| + e)
scalings:  S = scaling t (t < 2^24 exact): u;  S^2: 3 u;  q = S^2 + 0.25: 4 u;  c_skip = 0.25 / q: 6 u;  sqrt q: 4 u;  c_out = S / sqrt q: 7 u   ->  COEF = 8 (relative);
           t = 0: S = 0, q = 0.25, c_skip = 1, c_out = 0 exactly
target / m:  c_skip x + c_out x0:   e = (COEF + 1) u |c_skip x| + c_out e_x0 + (COEF + 1) u |c_out x0| + u |result|
loss:  d = m - target: e_d = e_m + u |d|
       l2:     l = d^2:  e_l = 2 |d| e_d + e_d^2 + u l;                   g = 2 d:  e_g = 2 e_d
       huber:  q = d^2 + c^2:  e_q = 2 |d| e_d + e_d^2 + u d^2 + u c^2 + u q;  r = sqrt q:  e_r = e_q / (2 r) + 2 u r;  l = r - c:  e_l = e_r + u |l|
               g = d / r:  e_g = e_d / r + |d| e_r / r^2 + 2 u |g|
       the two-stage sum: every term takes part in at most n + 64 additions:  |S - S64| <= sum e_l + gamma(n + 64) sum |l|;  per_sample = S (1 / n): 3 u;  loss: gamma(B + 1)
       dpred = gcoef g,  gcoef = ((grad_scale / (n B)) c_out) dx0:  the host quotient 2 u, c_out COEF u, the product u, dx0 = -(s / a): 2 u (v: exact), the product u,
               the last product u  ->  GRAD = 16 (15 counted);  e32 = |gcoef| e_g + GRAD u |dpred|;  then ONE bf16 rounding:  tol = e32 + ub (|dpred| + e32)
sampler:  denoised as m;  out = an denoised + sn noise:  e = an e_den + u |an den| + u |sn noise| + u |out|;  bf16: e + ub (|out| + e)
"""
import torch

from tests import lcm_ref as LR

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10
COEF = 8
GRAD = 16
AUTOGRAD = 24          # a gradient from another fp32 chain (torch autograd through the reference's expression): the same operands, at most this many roundings


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def _x0_eps_err(x, p, a, s, e_p, mode):
    if mode == "epsilon":
        sp = s * p
        num = x - sp
        x0 = num / a
        return (s * e_p + U * sp.abs() + U * num.abs()) / a + 2 * U * x0.abs(), e_p
    x0 = a * x - s * p
    eps = a * p + s * x
    return U * (a * x).abs() + s * e_p + U * (s * p).abs() + U * x0.abs(), a * e_p + U * (a * p).abs() + U * (s * x).abs() + U * eps.abs()


def solver_ref(x_s, pair, w, index, start, sched, prev, mode):
    """{name: (reference, bound)} for x_prev32, x_prev16"""
    r = LR.solver64(x_s, pair, w, index, start, sched, prev, mode)
    wd = r["w"] * (r["pc"] - r["pu"])
    e_p = U * (2 * wd.abs() + r["p"].abs())
    e_x0, e_eps = _x0_eps_err(r["x"], r["p"], r["a"], r["s"], e_p, mode)
    xp = r["x_prev"]
    e = SLACK * (r["ap"] * e_x0 + U * (r["ap"] * r["x0"]).abs() + r["sp"] * e_eps + U * (r["sp"] * r["eps"]).abs() + U * xp.abs())
    shape = x_s.shape
    return {"x_prev32": (xp.reshape(shape), (e + TINY).reshape(shape)), "x_prev16": (xp.reshape(shape), (e + UB * (xp.abs() + e) + TINY).reshape(shape))}


def _affine_err(cs, co, x, x0, e_x0):
    """the error of c_skip x + c_out x0 with kernel-computed scalings (exact where t = 0)"""
    res = cs * x + co * x0
    k = torch.where(co == 0, torch.zeros_like(co), torch.full_like(co, float(COEF + 1)))          # t = 0: c_skip = 1, c_out = 0 exactly: result = x
    return k * U * (cs * x).abs() + co * e_x0 + k * U * (co * x0).abs() + torch.where(co == 0, torch.zeros_like(co), torch.full_like(co, U)) * res.abs()


def target_ref(x_prev32, p_t, t, sched, mode, scaling=10.0):
    r = LR.target64(x_prev32, p_t, t, sched, mode, scaling)
    e_x0, _ = _x0_eps_err(r["xp"], r["p"], r["a"], r["s"], torch.zeros_like(r["p"]), mode)
    e = SLACK * _affine_err(r["c_skip"], r["c_out"], r["xp"], r["x0"], e_x0)
    shape = x_prev32.shape
    return {"target": (r["target"].reshape(shape), (e + torch.where(r["c_out"] == 0, 0.0, TINY)).expand_as(r["target"]).reshape(shape))}


def loss_ref(pred, x_s, target, start, sched, mode, scaling=10.0, loss_type="l2", huber_c=0.001, grad_scale=1.0, rounds=GRAD, out_bf16=True):
    """{name: (reference, bound)} for loss, per_sample, dpred"""
    r = LR.closed64(pred, x_s, target, start, sched, mode, scaling, loss_type, huber_c, grad_scale)
    B = pred.shape[0]
    n = r["p"].shape[1]
    e_x0, _ = _x0_eps_err(r["x"], r["p"], r["a"], r["s"], torch.zeros_like(r["p"]), mode)
    e_m = _affine_err(r["c_skip"], r["c_out"], r["x"], r["x0"], e_x0)
    d = r["d"]
    e_d = SLACK * (e_m + U * d.abs())
    c = float(huber_c)
    if loss_type == "l2":
        e_l = 2 * d.abs() * e_d + e_d * e_d + U * r["l"].abs()
        e_g = 2 * e_d
    else:
        q = d * d + c * c
        rt = q.sqrt()
        e_q = 2 * d.abs() * e_d + e_d * e_d + U * d * d + U * c * c + U * q
        e_r = SLACK * e_q / (2 * rt) + 2 * U * rt
        e_l = e_r + U * r["l"].abs()
        e_g = e_d / rt + d.abs() * e_r / q + 2 * U * r["g"].abs()
    e_sum = SLACK * e_l.sum(1) + gamma(n + 64) * r["l"].abs().sum(1)
    per = r["per_sample"]
    e_per = SLACK * (e_sum / n + 3 * U * per.abs())
    e_loss = SLACK * (e_per.sum() / B + gamma(B + 1) * per.abs().sum() / B)
    gcoef = (grad_scale / (n * B)) * r["c_out"] * r["dx0"]
    g = r["dpred"].reshape(B, n)
    e32 = SLACK * (gcoef.abs() * e_g + rounds * U * g.abs())
    tol = e32 + UB * (g.abs() + e32) if out_bf16 else e32
    return {"loss": (r["loss"], e_loss + TINY), "per_sample": (per, e_per + TINY), "dpred": (r["dpred"], (tol + TINY).reshape(pred.shape))}


def sample_ref(x, pred, noise, sched, t, t_next, mode, scaling=10.0):
    r = LR.sample_step64(x, pred, noise, sched, t, t_next, mode, scaling)
    e_x0, _ = _x0_eps_err(r["x"], r["p"], r["a"], r["s"], torch.zeros_like(r["p"]), mode)
    e_den = SLACK * _affine_err(r["c_skip"], r["c_out"], r["x"], r["x0"], e_x0)
    if r["last"]:
        e = e_den
    else:
        e = SLACK * (r["an"] * e_den + U * (r["an"] * r["denoised"]).abs() + U * (r["sn"] * r["noise"]).abs() + U * r["out"].abs())
    out = r["out"]
    return {"out": (out.reshape(x.shape), (e + UB * (out.abs() + e) + TINY).reshape(x.shape))}


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol); an element whose bound is 0 must be exact"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    ok = bool((err <= tol).all())
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ok, float(ratio.max())

"""Element-wise error bounds for the Internal Guidance kernels (simpletuner_amd/csrc/internal_guidance.hip) against the fp64 restatement
(tests/internal_guidance_ref.py) — derived, not fitted, in the style of tests/layersync_bounds.py and tests/gemm_bounds.py.  u = 2^-24 (fp32 unit roundoff),
v = 2^-8 (one round-to-nearest-even to bf16, relative), D = row length, N = 64, M = B * rows.  "Recursive summation" is the standard bound: an fp32 sum of K
terms, in any order, is off by at most K u sum|terms| (products of two bf16 values are exact in fp32; + 8 absorbs the adds of fixed-order partials and a bias).

Stored intermediates are chained, as in gemm_bounds.py: xhat / rstd are bounded against fp64 of the SAME bf16 input rows; everything computed FROM stored values
(y from xhat, Wf, c; dx from xhat, rstd, WfT, dy; the parameter gradients from xhat, dy) is bounded against the fp64 value of the kernel's own stored operands, so a
one-ulp tie in an intermediate cannot leak into the next stage.  The unchained end-to-end agreement with the executed reference is the fixture's and the engine
tests' business.

fold.  Wf = bf16(fl(gamma W)): |Wf - gamma W| <= (v + u (1 + v)) |gamma W|.  c = bf16(fl(sum_d W beta) + b): a D-term fmaf chain in thread-strided partials, a
butterfly, four wave sums and b — recursive summation over D + 8 terms, then one bf16 rounding:
    |c - c64| <= v |c64| + (1 + v) (D + 8) u (sum_d |W beta| + |b|)

forward, per row with A = max_j |x_j|, s = sqrt(var64 + 1e-6) = 1 / rstd64, d_j = x_j - mean:
  mean   = fl(sum x) * fl(1 / D): recursive summation of D bf16 values plus the two roundings of the scale: e_mean = (D + 2) u A;
  d_j    one subtraction of the perturbed mean: |d_j - d64_j| <= e_mean + u |d64_j| =: e_d;
  var    = fl(sum d_j^2) / D: each square moves by <= 2 |d_j| e_d + e_d^2, the sum by recursive summation; with sum |d_j| <= D sqrt(var64) <= D s the relative
         error of var + eps is delta_v <= 2 e_mean / s + (e_mean / s)^2 + (D + 8) u  (centred: no cancellation between E[x^2] and mean^2; the u |d_j| part of e_d
         is inside the + 8);
  rstd   = 1 / sqrt(.): |(1 + t)^(-1/2) - 1| <= |t| / 2 * (1 - |t|)^(-3/2) <= 0.77 |t| for |t| <= 1/4 (the function refuses rows beyond that); the square root, the
         division and the eps add cost three more roundings: delta_r = 0.77 delta_v + 8 u;
  xhat   = bf16(d_j * rstd): |xhat - xhat64| <= v |xhat64| + (1 + v) (e_d / s + |xhat64| (delta_r + 2 u)).
A constant row has var64 = 0, s = 1e-3: the bound is e_mean / s in absolute terms (xhat64 = 0), which is what a mean off by its roundings gives.

tokens.  y = bf16(acc), acc = sum_d xhat Wf + c on the thin GEMM route: gemm_bounds' form, tol = 1/2 ulp_bf16(|ref| + e) + e with e = (D + 8) u (|xhat| |Wf|^T + |c|).

backward.  g_d = sum_k dy_k WfT[d, k] on the MFMA (K = 64): e_g = (64 + 8) u sum_k |dy_k Wf_kd|.  m1 = fl(sum_d g) / D and m2 = fl(sum_d g xhat) / D (16 lane-local
terms per chunk, then two butterfly steps — a fixed order, D + 8 terms at most):
    e_m1 = mean_d e_g + (D + 8) u mean_d |g|,      e_m2 = mean_d (e_g |xhat|) + (D + 8) u mean_d |g xhat|
dh = rstd * ((g - m1) - xhat * m2): four roundings on top of the operands' errors:
    e_dh = rstd (e_g + e_m1 + |xhat| e_m2) + 4 u rstd (|g| + |m1| + |xhat m2|)
out = bf16(dx + dh): tol = 1/2 ulp_bf16(|ref| + e) + e with e = e_dh + u |ref|.

parameter gradients.  P = dy^T xhat and db = sum_m dy in split-M partials, fixed order: e_P = (M + 8) u |dy|^T |xhat|, e_db = (M + 8) u sum_m |dy|.  Then per element
    dW     = fmaf(P, gamma, fl(db beta)):      e = e_P |gamma| + e_db |beta| + 3 u (|P gamma| + |db beta|)
    dgamma = sum_n W P (8 chains of 8 + 8):    e = sum_n |W| e_P + (N + 8) u sum_n |W P|
    dbeta  = sum_n W db:                       e = sum_n |W| e_db + (N + 8) u sum_n |W db|
    db     itself:                             e = e_db
and for the bf16 gradient arena of a full fine-tune one more rounding: tol = 1/2 ulp_bf16(|ref| + e) + e.
"""
import torch

from tests.gemm_bounds import ulp_bf16

F64 = torch.float64
U = 2.0 ** -24
V = 2.0 ** -8
EPS = 1e-6
N = 64


def _rounded(ref, e):
    """one RNE to bf16 of an fp32 value within e of ref"""
    return 0.5 * ulp_bf16(ref.abs() + e) + e


def fold_bounds(gamma, beta, W, b):
    """-> (Wf64, tol_Wf, c64, tol_c); WfT has the same values transposed"""
    ga, be, Wd, bd = (t.to(F64) for t in (gamma, beta, W, b))
    D = Wd.shape[1]
    Wf = Wd * ga[None, :]
    c = Wd @ be + bd
    return Wf, (V + U * (1 + V)) * Wf.abs(), c, V * c.abs() + (1 + V) * (D + 8) * U * ((Wd * be[None, :]).abs().sum(dim=1) + bd.abs())


def fwd_bounds(h):
    """h [M, D] (the exact bf16 input values) -> (xhat64, tol_xhat [M, D], rstd64, tol_rstd [M])"""
    x = h.to(F64)
    D = x.shape[1]
    mean = x.mean(dim=1, keepdim=True)
    d = x - mean
    var = (d * d).mean(dim=1, keepdim=True)
    s = torch.sqrt(var + EPS)
    xhat = d / s
    e_mean = (D + 2) * U * x.abs().amax(dim=1, keepdim=True)
    delta_v = 2 * e_mean / s + (e_mean / s) ** 2 + (D + 8) * U
    assert float(delta_v.max()) <= 0.25, "fwd_bounds: a row outside the regime of the derivation (delta_v > 1/4)"
    delta_r = 0.77 * delta_v + 8 * U
    e_d = e_mean + U * d.abs()
    tol_x = V * xhat.abs() + (1 + V) * (e_d / s + xhat.abs() * (delta_r + 2 * U))
    return xhat, tol_x, (1.0 / s)[:, 0], (delta_r / s)[:, 0]


def tokens_bounds(xhat, Wf, c):
    """the kernel's own stored xhat [M, D], Wf [N, D], c [N] -> (y64, tol_y)"""
    x, w, cc = xhat.to(F64), Wf.to(F64), c.to(F64)
    ref = x @ w.t() + cc
    e = (x.shape[1] + 8) * U * (x.abs() @ w.abs().t() + cc.abs())
    return ref, _rounded(ref, e)


def bwd_bounds(xhat, rstd, dy, WfT, dx_in):
    """the kernel's own stored operands (xhat [M, D], rstd [M], WfT [D, N]), dy [M, N], dx_in [M, D] -> (out64, tol) of dx_in + dh"""
    x, r, g_, w, d0 = xhat.to(F64), rstd.to(F64)[:, None], dy.to(F64), WfT.to(F64), dx_in.to(F64)
    D = x.shape[1]
    g = g_ @ w.t()
    e_g = (N + 8) * U * (g_.abs() @ w.abs().t())
    m1, m2 = g.mean(dim=1, keepdim=True), (g * x).mean(dim=1, keepdim=True)
    e_m1 = e_g.mean(dim=1, keepdim=True) + (D + 8) * U * g.abs().mean(dim=1, keepdim=True)
    e_m2 = (e_g * x.abs()).mean(dim=1, keepdim=True) + (D + 8) * U * (g * x).abs().mean(dim=1, keepdim=True)
    dh = r * (g - m1 - x * m2)
    e_dh = r * (e_g + e_m1 + x.abs() * e_m2) + 4 * U * r * (g.abs() + m1.abs() + (x * m2).abs())
    ref = d0 + dh
    return ref, _rounded(ref, e_dh + U * ref.abs())


def wgrad_bounds(xhat, dy, gamma, beta, W, bf16_out: bool):
    """the kernel's own stored xhat [M, D], dy [M, N], the parameters -> {name: (ref64, tol)} for g_gamma, g_beta, g_W, g_b"""
    x, g_, ga, be, Wd = xhat.to(F64), dy.to(F64), gamma.to(F64), beta.to(F64), W.to(F64)
    M = x.shape[0]
    P, db = g_.t() @ x, g_.sum(dim=0)
    e_P, e_db = (M + 8) * U * (g_.abs().t() @ x.abs()), (M + 8) * U * g_.abs().sum(dim=0)
    out = {
        "g_W": (P * ga[None, :] + db[:, None] * be[None, :], e_P * ga.abs()[None, :] + e_db[:, None] * be.abs()[None, :] + 3 * U * ((P * ga[None, :]).abs() + (db[:, None] * be[None, :]).abs())),
        "g_gamma": ((Wd * P).sum(dim=0), (Wd.abs() * e_P).sum(dim=0) + (N + 8) * U * (Wd * P).abs().sum(dim=0)),
        "g_beta": ((Wd * db[:, None]).sum(dim=0), (Wd.abs() * e_db[:, None]).sum(dim=0) + (N + 8) * U * (Wd * db[:, None]).abs().sum(dim=0)),
        "g_b": (db, e_db),
    }
    if bf16_out:
        out = {k: (ref, _rounded(ref, e)) for k, (ref, e) in out.items()}
    return out

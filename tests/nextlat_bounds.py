"""Element-wise error bounds for the NextLat kernels (simpletuner_amd/csrc/nextlat.hip) against the fp64 restatement (tests/nextlat_ref.py) — derived, not fitted,
in the manner of tests/internal_guidance_bounds.py.  u = 2^-24 (fp32 unit roundoff); one round-to-nearest-even to bf16 costs half a bf16 ulp, at most 2^-9
relative: `_rounded(ref, e)` = 1/2 ulp_bf16(|ref| + e) + e for a stored bf16 value whose fp32 pre-image is within e of ref.  An fp32 sum of K terms, in any fixed
order, is off by at most K u sum|terms| (recursive summation; products of two bf16 values are exact in fp32, + 8 absorbs the adds of fixed-order partials).

Stored intermediates are chained: U, A, pred, psi, dA, dU, g, P1 and P2 each cost their one bf16 rounding where they are stored, and every kernel is bounded
against the fp64 value of ITS OWN stored operands, so a one-ulp tie in an intermediate cannot leak into the next stage.  The GEMM steps between the kernels are
tests/gemm_bounds.py's; the row pass (xhat, rstd) is internal_guidance_bounds.fwd_bounds.  The unchained end-to-end agreement with the executed reference is the
fixture's and the engine tests' business.

fold.  W1f = bf16(fl(gamma W_up)): e = u |gamma W_up|.  c1 = bf16(fl(sum_d W_up beta) + b_up): a D-term fmaf chain in lane-strided partials and a butterfly:
e = (D + 8) u (sum_d |W_up beta| + |b_up|).  Wd = bf16(W_down), bd = bf16(b_down): e = 0 (exact copies for bf16 parameters).  The transposes hold the same values.

gelu_erf.  ew_bounds' account of gelu_erf_parts (Abramowitz & Stegun 7.1.26, 0.75e-7 absolute on Phi, v_rcp_f32, v_exp_f32) at value = 1:
    A  = bf16(U phi):            e = |U| e_phi + 2 u |ref| + A20(ref, 1)
    dU = bf16(dA grad):          e = |dA| e_grad + 2 u |ref| + A20(ref, |dA|),   e_grad = e_phi + |U| 0.3989 gauss (3.5 u U^2 + 3 u) + u |grad|
gelu_erf' is Lipschitz with constant at most 1.13 and clamp with constant 1: a perturbed operand moves the result by no more than that multiple, so no
decided / undecided split around the kinks is needed — and, chained on stored operands, none arises.

loss.  d = fl(pred - t): u |d|.  psi = bf16(clamp(d, -1, 1)) or bf16(2 d): e = u |d| (the clamp is 1-Lipschitz) or 2 u |d|.  The per-element loss (0.5 d d,
|d| - 0.5, or d d) carries 3 u of its own roundings on top of |d loss / d d| u |d| <= 2 u loss + ...: e_elem = 6 u elem + u.  The mean: a lane's chain is
rows_per_wave * 8 ceil(D / 512) terms, then 6 butterfly steps, 3 wave adds, ceil(blocks / 256) partials per thread of the last pass, 6 + 3 more and the scale:
    |loss - loss64| <= (6 u + (L + 2) u) mean(elem) + u,      L = rows_per_wave 8 ceil(D / 512) + ceil(blocks / 256) + 18

ln_bwd_add.  m1 = fl(sum_d g) / D, m2 = fl(sum_d g xhat) / D over stored bf16 g and xhat (8 ceil(D / 512) lane-local terms, then the butterfly: D + 8 at most):
    e_m1 = (D + 8) u mean_d |g|,      e_m2 = (D + 8) u mean_d |g xhat|
f = fl(s rstd); dh = f ((g - m1) - xhat m2): five roundings on top of the operands' errors:
    e_dh = |s| rstd (e_m1 + |xhat| e_m2) + 5 u |s| rstd (|g| + |m1| + |xhat m2|)
out = bf16(dx + dh): tol = _rounded(ref, e_dh + u |ref|).

wgrad_up, from the stored P1 (bf16) and db1 (fp32):
    dW     = s fma(P1, gamma, fl(db1 beta)):              e = 4 u |s| (|P1 gamma| + |db1 beta|)
    db_up  = s db1:                                       e = u |s db1|
    dgamma = s sum_n W P1 (32-row chains, 32 row lanes, ceil(N / 256) chunks: N + 8 terms at most):    e = (N + 10) u |s| sum_n |W P1|
    dbeta  = s sum_n W db1:                               e = (N + 10) u |s| sum_n |W db1|
wgrad_down:  dW = s P2, db = s db2:  e = u |ref|.
For the bf16 gradient arena of a full fine-tune one more rounding: tol = _rounded(ref, e).  accumulate adds one fp32 (or bf16) addition to what is there.
"""
import math

import torch

from tests import ew_bounds as EW
from tests.gemm_bounds import ulp_bf16

F64 = torch.float64
U = 2.0 ** -24


def _rounded(ref, e):
    """one RNE to bf16 of an fp32 value within e of ref"""
    return 0.5 * ulp_bf16(ref.abs() + e) + e


def fold_bounds(gamma, beta, W_up, b_up, W_down, b_down):
    """-> {name: (ref64, tol)} for W1f, c1, Wd, bd (W1fT / WdT: the same values transposed)"""
    ga, be, Wu, bu, Wd, bd = (t.to(F64) for t in (gamma, beta, W_up, b_up, W_down, b_down))
    D = Wu.shape[1]
    W1f = Wu * ga[None, :]
    c1 = Wu @ be + bu
    e_c = (D + 8) * U * ((Wu * be[None, :]).abs().sum(dim=1) + bu.abs())
    z = torch.zeros((), dtype=F64)
    return {"W1f": (W1f, _rounded(W1f, U * W1f.abs())), "c1": (c1, _rounded(c1, e_c)), "Wd": (Wd, _rounded(Wd, z)), "bd": (bd, _rounded(bd, z))}


def gelu_fwd_bounds(U_):
    g = U_.to(F64)
    phi, _, e_phi = EW._phi_parts(g)
    ref = g * phi
    return ref, _rounded(ref, g.abs() * e_phi + 2 * U * ref.abs() + EW.A20(ref, 1.0))


def gelu_bwd_bounds(U_, dA):
    g, d = U_.to(F64), dA.to(F64)
    phi, gauss, e_phi = EW._phi_parts(g)
    k = 1.0 / math.sqrt(2.0 * math.pi)
    grad = phi + g * k * gauss
    e_grad = e_phi + g.abs() * k * gauss * (3.5 * U * g * g + 3 * U) + U * grad.abs()
    ref = d * grad
    return ref, _rounded(ref, d.abs() * e_grad + 2 * U * ref.abs() + EW.A20(ref, d.abs()))


def loss_chain(M: int, D: int) -> int:
    """the longest fp32 addition chain of st355_nextlat_loss (module docstring)"""
    blocks = min((M + 3) // 4, 1024)
    rows_per_wave = ((M + 3) // 4 + blocks - 1) // blocks
    return rows_per_wave * 8 * ((D + 511) // 512) + (blocks + 255) // 256 + 18


def loss_bounds(pred, target, mode: str):
    """pred, target [M, D] (the stored bf16 values) -> (loss64, tol_loss, psi64, tol_psi)"""
    p, t = pred.to(F64), target.to(F64)
    d = p - t
    if mode == "mse":
        elem, psi, e_psi = d * d, 2.0 * d, 2 * U * d.abs()
    else:
        a = d.abs()
        elem, psi, e_psi = torch.where(a < 1.0, 0.5 * d * d, a - 0.5), d.clamp(-1.0, 1.0), U * d.abs()
    M, D = p.shape
    loss = elem.mean()
    return loss, (6 * U + (loss_chain(M, D) + 2) * U) * loss + U, psi, _rounded(psi, e_psi)


def ln_bwd_add_bounds(g, xhat, rstd, scale: float, dx_in):
    """the stored operands g, xhat [M, D], rstd [M], the scale, dx_in [M, D] -> (out64, tol) of dx_in + dh"""
    gg, x, r, d0 = g.to(F64), xhat.to(F64), rstd.to(F64)[:, None], dx_in.to(F64)
    D = x.shape[1]
    s = abs(float(scale))
    m1, m2 = gg.mean(dim=1, keepdim=True), (gg * x).mean(dim=1, keepdim=True)
    e_m1 = (D + 8) * U * gg.abs().mean(dim=1, keepdim=True)
    e_m2 = (D + 8) * U * (gg * x).abs().mean(dim=1, keepdim=True)
    dh = float(scale) * r * (gg - m1 - x * m2)
    e_dh = s * r * (e_m1 + x.abs() * e_m2) + 5 * U * s * r * (gg.abs() + m1.abs() + (x * m2).abs())
    ref = d0 + dh
    return ref, _rounded(ref, e_dh + U * ref.abs())


def wgrad_up_bounds(P1, db1, gamma, beta, W_up, scale: float, bf16_out: bool):
    """-> {name: (ref64, tol)} for g_gamma, g_beta, g_W, g_b"""
    P, db, ga, be, W = P1.to(F64), db1.to(F64).reshape(-1), gamma.to(F64), beta.to(F64), W_up.to(F64)
    N = W.shape[0]
    s, a = float(scale), abs(float(scale))
    out = {
        "g_W": (s * (P * ga[None, :] + db[:, None] * be[None, :]), 4 * U * a * ((P * ga[None, :]).abs() + (db[:, None] * be[None, :]).abs())),
        "g_b": (s * db, U * a * db.abs()),
        "g_gamma": (s * (W * P).sum(dim=0), (N + 10) * U * a * (W * P).abs().sum(dim=0)),
        "g_beta": (s * (W * db[:, None]).sum(dim=0), (N + 10) * U * a * (W * db[:, None]).abs().sum(dim=0)),
    }
    if bf16_out:
        out = {k: (ref, _rounded(ref, e)) for k, (ref, e) in out.items()}
    return out


def wgrad_down_bounds(P2, db2, scale: float, bf16_out: bool):
    s = float(scale)
    out = {"g_W": (s * P2.to(F64), U * abs(s) * P2.to(F64).abs()), "g_b": (s * db2.to(F64).reshape(-1), U * abs(s) * db2.to(F64).reshape(-1).abs())}
    if bf16_out:
        out = {k: (ref, _rounded(ref, e)) for k, (ref, e) in out.items()}
    return out

"""Element-wise error bounds of the LoKr kernels (csrc/lokr.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16: 8 significant bits, round to
nearest even: the unit roundoff of a store), gamma(n) = n u / (1 - n u): the relative error of an fp32 sum of n terms in ANY order.

st355_lokr_fold, per element of a target (rows outside every target: copied, bound 0):
  1. a = fl(s w1[i, j])                                   |a - s w1| <= u |s w1|
  2. v = fma(a, w2[k, l], W) (one rounding)               |v - V64| <= u |s w1 w2| + u (|V64| + u |s w1 w2|),  V64 = W + s w1 w2
  3. Wf = bf16(v)                                         |Wf - V64| <= e_v + ub (|V64| + e_v)
     s = 0: a = 0, v = W exactly, Wf = W bit for bit.  WfT holds the same bits.  w2b = bf16(w2): |w2b - w2| <= ub |w2|.
st355_lokr_mix: fp32 w1 times bf16 dy by an ol-term fma chain (each fma rounds once: the chain is a sum of ol terms whose products are taken exactly), one bf16 store:
     |dP - dP64| <= gamma(ol) sum_i |w1 dy| + ub (|dP64| + gamma(ol) sum_i |w1 dy|)
st355_lokr_dw2: products of two bf16 are exact in fp32; a slice's tile is an fp32 sum of its rows on the MFMA, the slices are added in order, then one multiply by
     alpha and, when accumulating, one add.  At most R = M im rows + S <= R slices take part in the additions of one element:
     |out - out64| <= gamma(2 R) |alpha| sum |L R| (1 + 2 u) + 2 u |out64| (+ u |prev|)
st355_lokr_dw1: likewise over the M ok products of one element, the four waves of a workgroup and the <= 1024 workgroup partials:
     |out - out64| <= gamma(M ok + 1024 + 64) |alpha| sum |dy P| (1 + 2 u) + 2 u |out64| (+ u |prev|)      (+ 64: the MFMA pads ok to a multiple of 32 with zeros, four wave sums)
P (the GEMM route: x.view(M im, in) w2b^T, fp32 accumulation over in terms, one bf16 store):
     |P - P64| <= gamma(in) sum |x w2b| + ub (|P64| + gamma(in) sum |x w2b|)
"""
import torch

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def fold_ref(W, targets, s: float):
    """targets: [(n_off, N, w1, w2)].  (reference [N_total, K] fp64, bound)"""
    ref = W.to(F64).cpu().clone()
    tol = torch.zeros_like(ref)
    for (n_off, N, w1, w2) in targets:
        d = s * torch.kron(w1.to(F64).cpu(), w2.to(F64).cpu())
        V = ref[n_off:n_off + N] + d
        e_v = U * d.abs() + U * (V.abs() + U * d.abs())
        ref[n_off:n_off + N] = V
        tol[n_off:n_off + N] = e_v + UB * (V.abs() + e_v) + (TINY if s != 0.0 else 0.0)
    return ref, tol


def w2b_ref(w2):
    r = w2.to(F64).cpu()
    return r, UB * r.abs() + TINY


def mix_ref(dy, n_off: int, w1, ok: int):
    """dy [M, C] (the logical rows).  (reference [M, im ok], bound)"""
    ol, im = w1.shape
    d = dy.to(F64).cpu()[:, n_off:n_off + ol * ok].reshape(-1, ol, ok)
    w = w1.to(F64).cpu()
    ref = torch.einsum("ij,mik->mjk", w, d).reshape(d.shape[0], im * ok)
    mag = torch.einsum("ij,mik->mjk", w.abs(), d.abs()).reshape(d.shape[0], im * ok)
    e = gamma(ol) * mag
    return ref, e + UB * (ref.abs() + e) + TINY


def dw2_ref(dP, x, im: int, ok: int, alpha: float, prev=None):
    """dP [M, im ok], x [M, im in] (the logical rows).  (reference [ok, in], bound)"""
    M = x.shape[0]
    Lm, Rm = dP.to(F64).cpu().reshape(M * im, ok), x.to(F64).cpu().reshape(M * im, -1)
    v = alpha * (Lm.t() @ Rm)
    ref = v if prev is None else prev.to(F64).cpu() + v
    tol = gamma(2 * M * im) * abs(alpha) * (Lm.abs().t() @ Rm.abs()) * (1 + 2 * U) + 2 * U * ref.abs() + TINY
    if prev is not None:
        tol = tol + U * prev.to(F64).cpu().abs()
    return ref, tol


def dw1_ref(dy, n_off: int, P, ol: int, im: int, ok: int, alpha: float, prev=None):
    M = P.shape[0]
    d = dy.to(F64).cpu()[:, n_off:n_off + ol * ok].reshape(M, ol, ok)
    p = P.to(F64).cpu().reshape(M, im, ok)
    v = alpha * torch.einsum("mik,mjk->ij", d, p)
    ref = v if prev is None else prev.to(F64).cpu() + v
    tol = gamma(M * ok + 1024 + 64) * abs(alpha) * torch.einsum("mik,mjk->ij", d.abs(), p.abs()) * (1 + 2 * U) + 2 * U * ref.abs() + TINY
    if prev is not None:
        tol = tol + U * prev.to(F64).cpu().abs()
    return ref, tol


def p_ref(x, w2b, im: int):
    """x [M, im in] bf16, w2b [ok, in] bf16.  (reference [M, im ok], bound)"""
    M = x.shape[0]
    ok, in_ = w2b.shape
    xv, w = x.to(F64).cpu().reshape(M * im, in_), w2b.to(F64).cpu()
    ref = (xv @ w.t()).reshape(M, im * ok)
    e = gamma(in_) * (xv.abs() @ w.abs().t()).reshape(M, im * ok)
    return ref, e + UB * (ref.abs() + e) + TINY


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.to(F64).cpu() - ref).abs()
    return bool((err <= tol).all()), float((err / tol.clamp_min(TINY)).max())

"""Element-wise error bounds of the DoRA kernels (csrc/dora.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16: 8 significant bits, round to nearest even),
gamma(n) = n u / (1 - n u): the relative error of an fp32 sum of n terms in ANY order (each term takes part in at most n additions).

st355_dora_fold, per output row n of a target (slab of r_pad K-extension columns, K input columns):
  1. t[k] = sum_r B[n, r] A[r, k] on the MFMA: products of two bf16 are exact in fp32, the r_pad-term accumulation is not:  |t - t64| <= gamma(r_pad) sum_r |B||A| =: e_t
  2. v[k] = fl(t + W[n, k]):                                                                   |v - V64| <= e_t (1 + u) + u (|V64| + e_t) =: e_v
  3. S = sum_k fl(v^2) by fma in a fixed order over K terms (+ 5 butterfly steps + 3 wave sums):  |S - S64| <= sum_k (2 |V64| e_v + e_v^2) + gamma(K + 16) S_up =: e_S
     with S_up = S64 + sum_k (2 |V64| e_v + e_v^2)
  4. norm = sqrtf(S), correctly rounded:  |norm - norm64| <= e_S / norm64 + u (norm64 + e_S / norm64) =: e_n      (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b))
  5. inv_norm = fl(1 / norm):             |inv - 1 / norm64| <= e_n / (norm64 (norm64 - e_n)) + u / (norm64 - e_n)
     g = fl(m / norm):                    |g - m / norm64|  <= |m| e_n / (norm64 (norm64 - e_n)) + u |m| / (norm64 - e_n) =: e_g
  6. W' = bf16(fl(g W)):                  |W' - g64 W| <= e_g |W| + (|g64| + e_g) |W| (ub + 2 u) + tiny;  B_blk' likewise.  The transposes hold the same bits.
st355_dora_dmag: products of two bf16 exact, M-term fma sums per chunk then <= 64 k chunk sums, one multiply by inv_norm, one add when accumulating:
     |dm - dm64| <= gamma(M + 64) |inv| sum |dy y0| (1 + 2 u) + 2 u |dm64| (+ u |prev| through dm64 = prev + ...)
st355_dora_db_finish: fl(prev + fl(g P)) (or one fma):  |gB - gB64| <= u |g P| + u (1 + u) |gB64|
"""
import torch

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def fold_ref(W, A_cat_T, B_blk, m, targets, r_pad: int):
    """fp64 on the bf16 operands: {name: (reference, bound)} for inv_norm, g, Wf, Bf over all N rows (rows outside every target: reference None there is not needed —
    the targets of the tests tile N)"""
    W64, At, Bb, m64 = W.to(F64).cpu(), A_cat_T.to(F64).cpu(), B_blk.to(F64).cpu(), m.to(F64).cpu()
    N, K = W64.shape
    norm = torch.zeros(N, dtype=F64); e_n = torch.zeros(N, dtype=F64)
    for i, (n_off, n) in enumerate(targets):
        rows, slab = slice(n_off, n_off + n), slice(i * r_pad, (i + 1) * r_pad)
        t = Bb[rows, slab] @ At[:, slab].t()
        e_t = gamma(r_pad) * (Bb[rows, slab].abs() @ At[:, slab].abs().t())
        V = W64[rows] + t
        e_v = e_t * (1 + U) + U * (V.abs() + e_t)
        pert = (2 * V.abs() * e_v + e_v * e_v).sum(1)
        S = (V * V).sum(1)
        e_S = pert + gamma(K + 16) * (S + pert)
        nr = S.sqrt()
        norm[rows] = nr
        e_n[rows] = e_S / nr + U * (nr + e_S / nr)
    assert bool((e_n < 1e-3 * norm).all())
    lo = norm - e_n
    inv = 1.0 / norm
    e_inv = e_n / (norm * lo) + U / lo
    g = m64 / norm
    e_g = m64.abs() * e_n / (norm * lo) + U * m64.abs() / lo
    out = {"norm": (norm, e_n), "inv_norm": (inv, e_inv), "g": (g, e_g)}
    for name, src in (("Wf", W64), ("Bf", Bb)):
        out[name] = (g[:, None] * src, e_g[:, None] * src.abs() + (g.abs() + e_g)[:, None] * src.abs() * (UB + 2 * U) + TINY)
    return out


def dmag_ref(dy, y0, inv_norm, prev=None):
    """dy [M, N] (the logical rows), y0 [M, N] bf16, inv_norm fp32 as given: (reference, bound)"""
    d, y, inv = dy.to(F64).cpu(), y0.to(F64).cpu(), inv_norm.to(F64).cpu()
    M = d.shape[0]
    ref = inv * (d * y).sum(0)
    if prev is not None:
        ref = prev.to(F64).cpu() + ref
    tol = gamma(M + 64) * inv.abs() * (d * y).abs().sum(0) * (1 + 2 * U) + 2 * U * ref.abs() + TINY
    if prev is not None:
        tol = tol + U * prev.to(F64).cpu().abs()
    return ref, tol


def db_finish_ref(P, g, prev=None):
    v = g.to(F64).cpu()[:, None] * P.to(F64).cpu()
    ref = v if prev is None else prev.to(F64).cpu() + v
    return ref, U * v.abs() + U * (1 + U) * ref.abs() + TINY


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.to(F64).cpu() - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

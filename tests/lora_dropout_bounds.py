"""Element-wise bounds of the LoRA-dropout kernels (csrc/lora_dropout.hip) against fp64, every rounding counted — TEST INFRASTRUCTURE ONLY.

The operands are bf16 values in memory (exact in fp64), the mask is exact (integer arithmetic; dropped elements are exact zeros), every product of two bf16 numbers
is exact in fp32.  What rounds:
  * the fp32 accumulation of n products, in whatever order the MFMA and the split-M reduction take them: |err| <= gamma(n) * sum |terms|, gamma(n) = n u / (1 - n u),
    u = 2^-24 (Higham, Accuracy and Stability, Lemma 3.1 — holds for any summation order);
  * the multiplication by the fp32 scale 1 / (1 - p'), itself one rounding away from the exact quotient: two more factors (1 + u);
  * a bf16 store: round-to-nearest-even, |err| <= 2^-8 |value| (8 significand bits: half an ulp), plus the bf16 subnormal step 2^-134 near zero.
`T`:  one fp32 sum over K products, the scale, ONE bf16 rounding.
`dA`: fp32 sums over M products (MFMA inside a chunk, then the fixed-order reduce over chunks: n = M + chunks terms in the worst case), alpha * scale, an fp32 add into
      the previous value when accumulating.
`dx`: the adapter term is an fp32 sum over G * r_pad products per target, masked, summed over the targets, scaled, added in fp32 to the bf16 value the dx GEMM left and
      rounded to bf16 — so the input gradient carries TWO bf16 roundings (the GEMM's own store, then this one) where the unmasked K-extension has one; `dx` bounds the
      kernel's step (the second rounding), `dx_after_gemm` adds the first for a comparison that starts from the fp64 GEMM.
"""
import torch

F64 = torch.float64
U32 = 2.0 ** -24
UBF = 2.0 ** -8
TINY = 2.0 ** -133


def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def _keep64(keep):
    return keep.to(F64)


def down(x, A_g, keep, scale: float):
    """(fp64 reference, bound) of T_g = bf16(scale sum_k keep x A_g): x [M, K], A_g [r, K], keep [M, K]"""
    x, A = x.to(F64), A_g.to(F64)
    xm = x * _keep64(keep)
    ref = scale * (xm @ A.t())
    mag = scale * (xm.abs() @ A.abs().t())
    acc = gamma(x.shape[1] + 2) * mag
    return ref, UBF * (ref.abs() + acc) + acc + TINY


def dA(x, U_g, keep, scale: float, alpha: float = 1.0, prev=None, chunks: int = 1):
    """(fp64 reference, bound) of dA_g[r, k] (+)= alpha scale sum_m U_g[m, r] keep[m, k] x[m, k]: x [M, K], U_g [M, r] -> [r, K]"""
    x, U = x.to(F64), U_g.to(F64)
    xm = x * _keep64(keep)
    val = alpha * scale * (U.t() @ xm)
    mag = alpha * scale * (U.abs().t() @ xm.abs())
    bound = gamma(x.shape[0] + chunks + 3) * mag + 1e-37
    if prev is not None:
        val = prev.to(F64) + val
        bound = bound + U32 * val.abs()
    return val, bound


def dx(dx_old, U, A_cat, keeps, r_pad: int, scale: float):
    """(fp64 reference, bound) of dx = bf16(dx_old + scale sum_g keep_g . (U_g A_g)): dx_old [M, K] bf16, U [M, K2], A_cat [K2, K], keeps a list of [M, K] masks"""
    U, A = U.to(F64), A_cat.to(F64)
    add = torch.zeros(dx_old.shape, dtype=F64)
    mag = torch.zeros(dx_old.shape, dtype=F64)
    for g, keep in enumerate(keeps):
        c = slice(g * r_pad, (g + 1) * r_pad)
        add += (U[:, c] @ A[c]) * _keep64(keep)
        mag += (U[:, c].abs() @ A[c].abs()) * _keep64(keep)
    ref = dx_old.to(F64) + scale * add
    acc = gamma(len(keeps) * r_pad + len(keeps) + 3) * scale * mag + U32 * ref.abs()
    return ref, UBF * (ref.abs() + acc) + acc + TINY


def dx_after_gemm(base64, base_mag, K_base: int, U, A_cat, keeps, r_pad: int, scale: float):
    """the two roundings of dx from the fp64 base product on: base64 = dy W in fp64, base_mag = |dy| |W|; the dx GEMM stores bf16(base) (first rounding), the
    masked kernel adds the adapter term and stores again (second rounding).  (fp64 reference, bound)"""
    first = UBF * (base64.abs() + gamma(K_base) * base_mag) + gamma(K_base) * base_mag + TINY
    ref, second = dx(base64, U, A_cat, keeps, r_pad, scale)
    return ref, second + (1.0 + UBF) * first

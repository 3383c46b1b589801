"""Element-wise error bounds for the LayerSync kernels (simpletuner_amd/csrc/layersync.hip) against the fp64 restatement (tests/layersync_ref.py) of the SAME bf16
inputs — derived, not fitted, in the style of tests/gemm_bounds.py.  u = 2^-24 (fp32 unit roundoff), D = row length, n = B * rows.

cosine per row.  The kernel accumulates <s, t>, |s|^2 and |t|^2 in fp32 (products of bf16 values are exact in fp32; a lane chain of 8 * passes terms, then a
6-level butterfly) and forms c = <s, t> / (|s| |t|).  Recursive-summation bound: each sum is off by at most D u sum|a b|; by Cauchy-Schwarz sum|s t| <= |s| |t|, so the
dot product contributes D u to c, the two norms (square roots halve their relative error) D u / 2 each at |c| <= 1, the two divisions and the square roots a few u:

    |c - c64| <= 2 D u

mean.  One fixed-order fp32 sum of n values of magnitude <= 1 (error <= n u on the mean's numerator, i.e. <= n u / n per unit — bounded by n u outright), on top of
the rows' own error:

    |sim - sim64| <= 2 D u + n u

gradient.  G = (t^ - c s^) / max(|s|, 1e-12) / n is evaluated in fp32 and stored with ONE round-to-nearest-even to bf16: half a bf16 ulp, at most 2^-8
relative (8 significand bits).  The fp32 expression itself: |t^_j|, |s^_j| <= 1 carry the norms' relative error D u / 2 each, c carries 2 D u — together <= 4 D u in absolute terms
before the common factor 1 / (n |s|):

    |G - G64| <= 2^-8 |G64| + 4 D u / (n max(|s|, 1e-12))
"""
import torch

U = 2.0 ** -24
EPS = 1e-12


def cos_bound(D: int) -> float:
    return 2.0 * D * U


def sim_bound(D: int, n: int) -> float:
    return 2.0 * D * U + n * U


def grad_bound(G64: torch.Tensor, s_norm: torch.Tensor, D: int) -> torch.Tensor:
    """G64 [n, D] fp64, s_norm [n] = |s| per row (fp64) -> the per-element bound [n, D]"""
    n = G64.shape[0]
    return 2.0 ** -8 * G64.abs() + (4.0 * D * U / (n * s_norm.clamp_min(EPS)))[:, None]

"""Muon restated in fp64 (the arithmetic MuonClip intends) and a CPU stand-in for the Muon wrappers of `simpletuner_amd.ops`.

TEST INFRASTRUCTURE ONLY.  `ns_fp64` / `muon_step_fp64` are the yardstick the golden fixture (tests/golden/muon_vectors.pt, the reference's own
MuonClip executed) and the HIP kernels are held to.  `install(monkeypatch)` replaces ops.MuonPlan / ops.muon_step / ops.muon_orthogonalize with
plain-torch fp32 functions honouring the same contracts (one fp32 arena, matrices at element offsets), so St355Muon's host logic and the trainer
run with `-m "not gpu"`; the GPU tests are the proof for the kernels.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64
NS_DEFAULT = (3.4445, -4.7750, 2.0315)


def ns_fp64(x: torch.Tensor, coeffs, normalize: bool = True, eps: float = 1e-7) -> torch.Tensor:
    """the orthogonalisation of one matrix, in its own orientation: X = x (or x^T if tall), X /= max(||X||_F, eps), then per (a, b, c):
    A = X X^T, X = a X + (b A + c A A) X"""
    X = x.to(F64)
    tall = X.shape[0] > X.shape[1]
    if tall:
        X = X.T
    if normalize:
        X = X / X.norm().clamp(min=eps)
    for a, b, c in coeffs:
        A = X @ X.T
        X = a * X + (b * A + c * (A @ A)) @ X
    return X.T if tall else X


def coefficients(ns_steps=5, ns_coefficients=NS_DEFAULT, use_cans=False, cans_a_bound=1e-4):
    from simpletuner_amd.training.optimizer import muon_cans_coefficients
    return muon_cans_coefficients(ns_steps, cans_a_bound) if use_cans else [tuple(ns_coefficients)] * ns_steps


def muon_step_fp64(ps, grads, ms, lr, momentum=0.95, weight_decay=0.1, eps=1e-7, rms_scale_factor=0.2, coeffs=None, grad_scale=1.0,
                   store=None):
    """one Muon step over lists of matrices; returns (new params, new momenta) in fp64.  `store` (e.g. torch.bfloat16) rounds at the points
    where the reference materialises a tensor of the parameter dtype (momentum, orthogonalised update, scaled update, decayed and updated
    parameter) — how its bf16 / stochastic_rounding=False path is restated"""
    rnd = (lambda t: t.to(store).to(F64)) if store is not None else (lambda t: t)
    coeffs = coefficients() if coeffs is None else coeffs
    out_p, out_m = [], []
    for p, g, m in zip(ps, grads, ms):
        p, g, m = p.to(F64), g.to(F64), m.to(F64)
        m = rnd(m + (1.0 - momentum) * (grad_scale * g - m))
        O = rnd(ns_fp64(m, coeffs, True, eps))
        O = rnd(O * (math.sqrt(max(p.shape)) * rms_scale_factor))
        if weight_decay > 0:
            p = rnd(p + (-lr * weight_decay) * p)
        p = rnd(p + (-lr) * O)
        out_p.append(p)
        out_m.append(m)
    return out_p, out_m


# ---- CPU stand-in for the st355_muon_* wrappers ----------------------------------------------------------------------------------
class MuonPlanCPU:
    def __init__(self, offsets, shapes, device):
        for s in shapes:
            if min(s) > 128:
                raise RuntimeError("muon_plan: short side above 128")
        self.n = len(shapes)
        self.mats = [(int(o), int(s[0]), int(s[1])) for o, s in zip(offsets, shapes)]

    def launches(self, ns_steps):
        return 2 + 3 * ns_steps * len({(min(r, c) + 31) // 32 for _, r, c in self.mats})


def _ns_fp32(X, coeffs, normalize, eps):
    tall = X.shape[0] > X.shape[1]
    X = X.T.contiguous() if tall else X.clone()
    if normalize:
        X = X / X.norm().clamp(min=eps)
    for a, b, c in coeffs:
        A = X @ X.T
        X = a * X + (b * A + c * (A @ A)) @ X
    return X.T if tall else X


def muon_step_cpu(plan, p, g, m, coeffs, lr, momentum=0.95, weight_decay=0.1, eps=1e-7, rms_scale_factor=0.2, grad_scale=1.0):
    for off, r, c in plan.mats:
        n = r * c
        pv, gv, mv = p[off:off + n].view(r, c), g[off:off + n].view(r, c), m[off:off + n].view(r, c)
        mv.copy_(mv + (1.0 - momentum) * (gv * grad_scale - mv))
        O = _ns_fp32(mv, coeffs, True, eps) * float(math.sqrt(max(r, c)) * rms_scale_factor)
        pv.add_(pv, alpha=-lr * weight_decay)
        pv.add_(O, alpha=-lr)


def muon_orthogonalize_cpu(plan, x, coeffs, normalize=True, eps=1e-7, out=None):
    out = torch.zeros_like(x) if out is None else out
    for off, r, c in plan.mats:
        out[off:off + r * c].view(r, c).copy_(_ns_fp32(x[off:off + r * c].view(r, c), coeffs, normalize, eps))
    return out


def install(monkeypatch):
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "MuonPlan", MuonPlanCPU)
    monkeypatch.setattr(ops, "muon_step", muon_step_cpu)
    monkeypatch.setattr(ops, "muon_orthogonalize", muon_orthogonalize_cpu)

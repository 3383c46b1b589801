"""Element-wise error bounds for the Lion step (simpletuner_amd/csrc/lion.hip: st355_lion_step, st355_lion_step_bf16) against an fp64 restatement of the SAME stored
inputs, written like tests/step_bounds.py (whose U, f32, check_f32, check_bf16, ema_f32, ema_bf16 and bits are used here), plus a CPU stand-in for ops.lion_step.

What the step is pinned to.  optimi is not installed anywhere this project is built or tested and the reference does not vendor it, so nothing here executes
optimi's code.  The restatement is the published rule (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", Algorithm 1) with decoupled weight decay
scaled by the learning rate (optimi's decouple_lr=False) and, for bf16 parameters, a Kahan-compensated parameter update; the registry's default settings are read
from the reference's optimizer_param.py with ast (tools/gen_lion_golden.py -> tests/golden/lion_vectors.pt).

Where the bounds come from.  The kernel computes in fp32, u = 2^-24 per rounding, in the order below; the library is built with -ffp-contract=fast-honor-pragmas:
a fused multiply-add rounds once where the bound counts two roundings, never more.  The scalars are the fp32 values that cross the ABI (SB.f32); 1 - beta and
lr wd are formed in fp32 by the launcher, and those roundings are among the ones counted.  No number below is fitted to a kernel's output.
    g' = g grad_scale                         e_g = u |g'|
    c  = m + (g' - m)(1 - b1)                 e_c = (1 - b1) e_g + 3 u (1 - b1) |g' - m| + u |c|       (the difference, 1 - b1, the product; the add)
    s  = sign(c) in {-1, 0, +1}
    m' = m + (g' - m)(1 - b2)                 e_m the same form with b2; an fp32 output (SB.check_f32 adds its last rounding u |m'|), on the bf16 arena one RNE
                                              to bf16 on top: tol = 1/2 ulp_bf16(|m'| + e_m) + e_m (SB.check_bf16)
    d  = -lr s - (lr wd) p                    e_d = 2 u |lr wd p| + u |d|                             (lr wd, its product with p; lr s is exact; the subtraction)
    fp32 arena:          p' = p + d           tol = e_d + u |p'|                                       (SB.check_f32)
    bf16 arena, no comp: p' = bf16(p + d)     t = d, e_t = e_d below
    bf16 arena, Kahan:   t = comp + d         e_t = e_d + u |t|
                         p' = bf16(p + t)     e = e_t + u |p + t|;  tol = 1/2 ulp_bf16(|p + t| + e) + e
                         comp' = bf16(t - (p' - p))   chained on the STORED p': wanted t - (p'_stored - p).  The difference of two bf16 numbers is carried with
                                              u |p' - p| (it is exact only when their exponents lie within 16 of each other), the outer subtraction with
                                              u |comp'|:  e = e_t + u |p' - p| + u |comp'|, then one RNE (SB.check_bf16)
The EMA and p_bf16 are those of AdamW (SB.ema_f32 / SB.ema_bf16 chained on the stored p'; p_bf16 bit-equal to one RNE of the stored p').

sign() is discontinuous, so the check splits the elements.  An element is DECIDED when |c| > e_c in the restatement (the kernel's c then has the same sign), or when
c == 0 and e_c == 0 (g' = m = 0: every intermediate is an exact zero); its p' is held to the bound around p + t(s) with the restatement's s.  Every other element
is UNDECIDED: its p' must lie within the bound around p + t(s) for SOME s in {-1, 0, +1} (the one that fits best is taken, and comp' is chained on that same s).
Nothing is left unchecked.  The share of undecided elements must be at most 1e-3 of the arena; check_step asserts that on the restatement's side before it looks
at the kernel's output.  make_inputs() adds 64 elements built to cancel, g = -(m b1 / (1 - b1)) / grad_scale rounded to the storage dtype, so that the undecided
branch runs: in fp32 storage that rounding leaves |c| ~ u |m| against e_c ~ 4 u |m|.  In bf16 storage the rounding of g leaves |c| ~ 0.9 x 2^-9 |m|, far above
e_c, so on the bf16 arena the same 64 elements come out decided (with a |c| 2^15 times smaller than their neighbours'): no bf16 g cancels a bf16 m at b1 = 0.9.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests.step_bounds import U, bits, check_bf16, check_f32, ema_bf16, ema_f32, f32  # noqa: F401  (re-exported for the tests)

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
MAX_UNDECIDED = 1e-3
GOLDEN = Path(__file__).resolve().parent / "golden" / "lion_vectors.pt"


def golden():
    return torch.load(GOLDEN)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(n, dtype, seed, grad_scale=0.5, beta1=0.9, device="cpu"):
    """the seeded inputs every Lion test shares (the seeds live in tests/golden/lion_vectors.pt): g ~ N(0, 1), m ~ 0.5 N(0, 1), p ~ 0.05 N(0, 1), all in the storage
    dtype; a compensation buffer below half a bf16 ulp of p; an EMA shadow near p.  A leading block of exact zeros in g and m (1024 elements, 256 when n < 8192),
    the first 8 of them with p = -0.0; then, when n >= 64 000 (so that they stay under MAX_UNDECIDED), 64 elements built to cancel."""
    gen = torch.Generator().manual_seed(int(seed))
    g = torch.randn(n, generator=gen)
    m = 0.5 * torch.randn(n, generator=gen)
    p = 0.05 * torch.randn(n, generator=gen)
    comp = 5e-5 * torch.randn(n, generator=gen)
    ema = p + 1e-3 * torch.randn(n, generator=gen)
    zeros = 1024 if n >= 8192 else 256
    cancel = 64 if n >= 64000 else 0
    g[:zeros] = 0
    m[:zeros] = 0
    comp[:zeros] = 0
    p[:8] = -0.0
    g, m, p, ema = g.to(dtype), m.to(dtype), p.to(dtype), ema.to(dtype)
    if cancel:
        b1 = f32(beta1)
        mc = m[zeros:zeros + cancel].to(F64)
        g[zeros:zeros + cancel] = (-(mc * b1 / (1.0 - b1)) / f32(grad_scale)).to(dtype)
    out = dict(p=p, g=g, m=m, comp=comp.to(BF16), ema=ema, zeros=zeros, cancel=cancel)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in out.items()}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
def lion_consts(lr, beta1, beta2, wd, grad_scale, ema_decay=0.0):
    """every scalar as the fp32 value the ABI receives; omd = 1.f - decay as fp32 forms it (SB.adam_consts)"""
    return dict(lr=f32(lr), b1=f32(beta1), b2=f32(beta2), wd=f32(wd), gs=f32(grad_scale), omd=float(np.float32(1.0) - np.float32(ema_decay)))


class Ref:
    """one Lion step from (p, g, m[, comp]) in fp64: c, e_c, s, the decided mask, (m', e_m), and update(s) -> (p + t, e_t, t) for a sign tensor s"""

    def __init__(self, p, g, m, c, comp=None):
        self.p, g, m = p.to(F64), g.to(F64), m.to(F64)
        self.comp = None if comp is None else comp.to(F64)
        self.k = c
        omb1, omb2 = 1.0 - c["b1"], 1.0 - c["b2"]
        g1 = g * c["gs"]
        e_g = U * g1.abs()
        diff = g1 - m
        self.c = m + diff * omb1
        self.e_c = omb1 * e_g + 3 * U * omb1 * diff.abs() + U * self.c.abs()
        self.s = torch.sign(self.c)
        self.decided = (self.c.abs() > self.e_c) | ((self.c == 0) & (self.e_c == 0))
        m1 = m + diff * omb2
        self.m = (m1, omb2 * e_g + 3 * U * omb2 * diff.abs() + U * m1.abs())

    def undecided_share(self):
        return float((~self.decided).to(F64).mean())

    def update(self, s):
        dec = self.k["lr"] * self.k["wd"] * self.p
        d = -self.k["lr"] * s - dec
        e_d = 2 * U * dec.abs() + U * d.abs()
        if self.comp is None:
            t, e_t = d, e_d
        else:
            t = self.comp + d
            e_t = e_d + U * t.abs()
        return self.p + t, e_t, t


def _tol(want, e, bf16_out):
    return 0.5 * GB.ulp_bf16(want.abs() + e) + e if bf16_out else e + U * want.abs() + 1e-300


def check_step(name, c, p0, g, m0, p_out, m_out, comp0=None, comp_out=None, verbose=True):
    """One stored step against the restatement.  p0 / g / m0 (/ comp0): the stored inputs; p_out / m_out (/ comp_out): what the implementation stored.  The arena is
    p0's dtype.  Returns (reports, info): reports = [m, p(, comp)] (SB.check_f32 / SB.check_bf16 reports, see assert_reports), info = dict(undecided, share,
    flipped) with `flipped` the number of undecided elements whose best-fitting sign is not the restatement's."""
    bf = p0.dtype == BF16
    ref = Ref(p0, g, m0, c, comp0)
    share = ref.undecided_share()
    assert share <= MAX_UNDECIDED, f"{name}: {share:.2e} of the arena is undecided in the restatement (limit {MAX_UNDECIDED}): the inputs do not test the sign"
    chk = check_bf16 if bf else check_f32
    reports = [chk(f"{name} m", m_out, *ref.m, flat=True, verbose=verbose)]
    got = p_out.to(F64)
    want, e_t, t = ref.update(ref.s)
    e_p = e_t + U * want.abs() if bf else e_t
    s_used = ref.s.clone()
    und = ~ref.decided
    if bool(und.any()):
        best = ((got - want).abs() / _tol(want, e_p, bf))
        for sv in (-1.0, 0.0, 1.0):
            w2, et2, t2 = ref.update(torch.full_like(ref.s, sv))
            e2 = et2 + U * w2.abs() if bf else et2
            r2 = (got - w2).abs() / _tol(w2, e2, bf)
            take = und & (r2 < best)
            best = torch.where(take, r2, best)
            want, e_p, t, e_t = torch.where(take, w2, want), torch.where(take, e2, e_p), torch.where(take, t2, t), torch.where(take, et2, e_t)
            s_used = torch.where(take, torch.full_like(s_used, sv), s_used)
    reports.append(chk(f"{name} p", p_out, want, e_p, flat=True, verbose=verbose))
    if comp_out is not None:
        moved = got - ref.p                                  # chained on the stored p'
        cw = t - moved
        reports.append(check_bf16(f"{name} comp", comp_out, cw, e_t + U * moved.abs() + U * cw.abs(), flat=True, verbose=verbose))
    info = dict(undecided=int(und.sum()), share=share, flipped=int((s_used != ref.s).sum()))
    if verbose:
        print(f"[bound] {name}: {info['undecided']} undecided of {got.numel()} ({info['flipped']} took another sign than the restatement's)")
    return reports, info


def reports_ok(reports):
    return all(r.ok for r in reports)


def assert_reports(reports):
    for r in reports:
        if isinstance(r, NB.SumReport):
            assert r.ok, r.line()
        else:
            GB.assert_bound(r)


# ---- CPU stand-in for ops.lion_step ----------------------------------------------------------------------------------------------------------------------
def lion_step_cpu(p, g, m, lr, beta1=0.9, beta2=0.99, weight_decay=0.0, grad_scale=1.0, comp=None, ema=None, ema_decay=0.0, p_bf16=None, plant=None):
    """ops.lion_step's contract in fp32 torch ops on host tensors, every operation rounded separately, in the kernel's order.  `plant` swaps in one of three
    deliberate errors the checker must reject: "sign_of_m" (sign taken from m' instead of c), "betas_swapped", "decay_after" (decay applied to p' after the update)."""
    assert p.dim() == 1 and p.is_contiguous() and g.is_contiguous() and p.dtype in (F32, BF16) and g.dtype == p.dtype and m.dtype == p.dtype, "lion_step: flat arenas of one dtype"
    assert p.dtype == F32 or p.numel() % 8 == 0, "lion_step_bf16: n must be a multiple of 8"
    assert comp is None or (p.dtype == BF16 and comp.dtype == BF16), "lion_step: the compensation buffer belongs to the bf16 arena"
    assert p_bf16 is None or p.dtype == F32
    k = lambda x: torch.tensor(x, dtype=F32)
    if plant == "betas_swapped":
        beta1, beta2 = beta2, beta1
    pf, mf = p.float(), m.float()
    gf = g.float() * k(grad_scale)
    diff = gf - mf
    cc = mf + diff * (k(1.0) - k(beta1))
    m_new = mf + diff * (k(1.0) - k(beta2))
    s = torch.sign(m_new if plant == "sign_of_m" else cc)
    lrwd = k(lr) * k(weight_decay)
    if plant == "decay_after":
        d = -k(lr) * s
        d = d - lrwd * (pf + d)
    else:
        d = -k(lr) * s - lrwd * pf
    if comp is None:
        pn = torch.where(d == 0, pf, pf + d).to(p.dtype)                     # a zero update leaves the bits alone, also those of -0 (lion_apply)
    else:
        t = comp.float() + d
        pn = torch.where(t == 0, pf, pf + t).to(BF16)
        comp.copy_((t - (pn.float() - pf)).to(BF16))
    p.copy_(pn)
    m.copy_(m_new.to(m.dtype))
    if ema is not None:
        ef = ema.float()
        ema.copy_((ef - (k(1.0) - k(ema_decay)) * (ef - p.float()).to(ema.dtype).float()).to(ema.dtype))       # (s - p) materialised in the shadow dtype, as k_ema
    if p_bf16 is not None:
        p_bf16.copy_(p.to(BF16))


def install(monkeypatch):
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "lion_step", lion_step_cpu)
    return ops

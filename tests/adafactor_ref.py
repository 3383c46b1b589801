"""Adafactor restated in fp64 (torch/optim/_adafactor.py::_single_tensor_adafactor) and a CPU stand-in for the Adafactor wrappers of
`simpletuner_amd.ops`, plus the one mixed arena the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY.  `step_tensor` is the rule for ONE tensor in whatever dtype it is handed (fp64 for the yardstick): gradient times
grad_scale, alpha from the RMS of p BEFORE the decay, the decay, the factored (last two dims, leading dims a batch) or plain second moment lerped
with 1 - beta2_t = step ** beta2_decay, eps1 on the row-variance mean and eps1 ** 2 on the estimate, the RMS clip of the update, the apply.  It
returns every intermediate the bounds of tests/adafactor_bounds.py need.  `run_fp64` is the trajectory of a list of tensors under it.
`install(monkeypatch)` replaces ops.AdafactorPlan / ops.adafactor_step with plain-torch fp32 functions honouring the same contracts (state fp32,
p rounded once into the arena dtype), so St355Adafactor's host logic and the trainer run with `-m "not gpu"`; the GPU tests are the proof for
the kernels."""
from __future__ import annotations

import itertools

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16


def factor_shape(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 1:
        return 1, 0, shape[0]
    batch = 1
    for s in shape[:-2]:
        batch *= s
    return batch, shape[-2], shape[-1]


def torch_lerp(a, b, w):
    """Tensor.lerp_'s two formulas (ATen lerp: a + w (b - a) below 0.5, b - (b - a)(1 - w) from there on)"""
    diff = b - a
    return a + w * diff if w < 0.5 else b - diff * (1.0 - w)


def scalars(step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale):
    """the host doubles of one step (what crosses the ABI): step counts from 1"""
    return dict(omb2=float(step) ** beta2_decay, rho=min(float(lr), 1.0 / float(step) ** 0.5), eps1=float(eps1), eps1sq=float(eps1) * float(eps1),
                eps2=float(eps2), d=float(d), decay=1.0 - float(lr) * float(weight_decay), gs=float(grad_scale))


def scalars_f32(*a, **kw):
    """the same, each rounded once to fp32: the values st355_adafactor_step hands its kernels"""
    import numpy as np
    return {k: float(np.float32(v)) for k, v in scalars(*a, **kw).items()}


def step_tensor(p, g, state, c):
    """one step of one tensor p [batch, R, C] (or [C] with state = {"variance"}) in p's dtype; state tensors are updated in place
    (row_var [batch, R, 1], col_var [batch, 1, C]).  Returns the new p and the intermediates"""
    numel = p.numel()
    g1 = g * c["gs"]
    rms = p.norm(2) / numel ** 0.5
    alpha = torch.clamp(rms, min=c["eps2"]) * c["rho"]
    pd = p * c["decay"]
    x = dict(g1=g1, p=p, pd=pd)
    if "variance" in state:
        state["variance"].copy_(torch_lerp(state["variance"], g1 * g1, c["omb2"]))
        v = state["variance"].clone()
    else:
        x["row_mean"], x["col_mean"] = (g1 * g1).mean(dim=-1, keepdim=True), (g1 * g1).mean(dim=-2, keepdim=True)
        x["row_old"], x["col_old"] = state["row_var"].clone(), state["col_var"].clone()
        state["row_var"].copy_(torch_lerp(state["row_var"], x["row_mean"], c["omb2"]))
        state["col_var"].copy_(torch_lerp(state["col_var"], x["col_mean"], c["omb2"]))
        x["rm"] = state["row_var"].mean(dim=-2, keepdim=True).clamp(min=c["eps1"])
        v = (state["row_var"] @ state["col_var"]) / x["rm"]
    u = g1 * v.clamp(min=c["eps1sq"]).rsqrt()
    urms = u.norm(2) / (numel ** 0.5 * c["d"])
    denom = torch.clamp(urms, min=1.0)
    x.update(v=v, u=u, alpha=alpha, denom=denom, rms=rms, urms=urms)
    return pd - (alpha / denom) * u, x


def new_state(shape, dtype=F64):
    batch, R, C = factor_shape(shape)
    if R == 0:
        return {"variance": torch.zeros(C, dtype=dtype)}
    return {"row_var": torch.zeros(batch, R, 1, dtype=dtype), "col_var": torch.zeros(batch, 1, C, dtype=dtype)}


def as3(t, shape):
    batch, R, C = factor_shape(shape)
    return t.reshape(C) if R == 0 else t.reshape(batch, R, C)


def run_fp64(p0, grads, lr, beta2_decay=-0.8, eps=(None, 1e-3), d=1.0, weight_decay=0.0, grad_scale=1.0, eps1_dtype=F32, first_step=1, states=None):
    """the trajectory of a list of tensors: grads[k][i] is tensor i's gradient of step first_step + k.  Returns ([per step [per tensor p]], states,
    [per step [per tensor intermediates]]).  eps1=None is the epsilon of eps1_dtype (the parameters' own dtype in torch)"""
    eps1 = torch.finfo(eps1_dtype).eps if eps[0] is None else eps[0]
    shapes = [tuple(p.shape) for p in p0]
    ps = [as3(p.detach().to(F64), s).clone() for p, s in zip(p0, shapes)]
    states = [new_state(s) for s in shapes] if states is None else states
    traj, inter = [], []
    for k, gk in enumerate(grads):
        c = scalars(first_step + k, lr, beta2_decay, eps1, eps[1], d, weight_decay, grad_scale)
        xs = []
        for i, s in enumerate(shapes):
            ps[i], x = step_tensor(ps[i], as3(gk[i].to(F64), s), states[i], c)
            xs.append(x)
        traj.append([p.reshape(s).clone() for p, s in zip(ps, shapes)])
        inter.append(xs)
    return traj, states, inter


# ---- the mixed arena of the CPU and GPU tests ------------------------------------------------------------------------------------------------------
ARENA_SHAPES = [(8, 40), (40, 8), (4, 33), (130, 257), (1, 64), (6, 3, 2, 2), (77,), (5,)]
ZERO_TENSOR = 1            # (40, 8): LoRA's B at its initial value — RMS(p) = 0, the eps2 floor decides alpha
PART_CLAMPED = 2           # (4, 33): one loud row keeps the row mean above eps1 while the quiet rows' estimate falls below eps1^2
ROW_MEAN_CLAMPED = 4       # (1, 64): the row-variance mean lies below eps1
LR = 1e-2
STEPS = 3
# gradient size per step: growing (the update's RMS exceeds d: denom > 1), shrinking (denom = 1)
GROWTH = {0: (1.0, 8.0, 0.5), 1: (1.0, 0.1, 0.05), 3: (1.0, 6.0, 30.0), 5: (1.0, 0.2, 4.0), 6: (1.0, 5.0, 0.3), 7: (1.0, 0.1, 0.1)}
CASES = list(itertools.product((0.0, 0.01), (1.0, 0.5)))          # (weight_decay, grad_scale): all four, on both arena instances


def arena_offsets(shapes, dtype):
    """every tensor starts 16-byte aligned: pad elements follow a tensor whose byte length is no multiple of 16"""
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        n = 1
        for v in s:
            n *= v
        off += (n + per16 - 1) // per16 * per16
    return offs, off


def make_arena(dtype, seed=0):
    """(offsets, length, p0 flat, [gflat per step]) in `dtype`, CPU.  The values are rounded to dtype here, so every consumer sees the same numbers.
    Sizes follow eps1 = finfo(dtype).eps, so that the same clamps act in the fp32 and in the bf16 instance"""
    gen = torch.Generator().manual_seed(seed)
    eps1 = torch.finfo(dtype).eps
    offs, n = arena_offsets(ARENA_SHAPES, dtype)
    p = torch.zeros(n, dtype=F64)
    gs = [torch.zeros(n, dtype=F64) for _ in range(STEPS)]
    for i, (s, o) in enumerate(zip(ARENA_SHAPES, offs)):
        k = 1
        for v in s:
            k *= v
        if i != ZERO_TENSOR:
            p[o:o + k] = 0.05 * torch.randn(k, generator=gen, dtype=F64)
        for step in range(STEPS):
            g = torch.randn(s, generator=gen, dtype=F64)
            if i == PART_CLAMPED:
                g[0] *= 1.0
                g[1:] *= 0.1 * eps1
            elif i == ROW_MEAN_CLAMPED:
                g *= 0.1 * eps1 ** 0.5
            else:
                g *= max(1e-2, 40.0 * eps1) * GROWTH[i][step]      # well above eps1 (bf16: 2^-7), so the clamps act where the arena means them to
            if i == 7:
                g[0] = 0.0                                     # an exactly-zero gradient element: u = 0
                g[1] = 0.01 * eps1                             # and one below eps1: the eps1^2 clamp on a 1-D variance
            gs[step][o:o + k] = g.reshape(-1)
    return offs, n, p.to(dtype), [g.to(dtype) for g in gs]


def tensors_of(flat, offs, shapes=None):
    shapes = ARENA_SHAPES if shapes is None else shapes
    out = []
    for s, o in zip(shapes, offs):
        k = 1
        for v in s:
            k *= v
        out.append(flat[o:o + k].view(s))
    return out


def pad_mask(offs, n, shapes=None):
    """True at the pad elements of an arena of length n"""
    m = torch.ones(n, dtype=torch.bool)
    for t in tensors_of(m, offs, shapes):
        t.fill_(False)
    return m


# ---- CPU stand-in for the st355_adafactor_* wrappers ---------------------------------------------------------------------------------------------
class AdafactorPlanCPU:
    def __init__(self, offsets, shapes, device):
        self.n = len(shapes)
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.offsets = [int(o) for o in offsets]
        self.factors = [factor_shape(s) for s in self.shapes]
        self.rv_offsets, self.cv_offsets, self.var_offsets = [], [], []
        rv = cv = var = 0
        for batch, R, C in self.factors:
            self.rv_offsets.append(rv)
            self.cv_offsets.append(cv)
            self.var_offsets.append(var)
            if R == 0:
                var += C
            else:
                rv += batch * R
                cv += batch * C
        self.rv_len, self.cv_len, self.var_len = rv, cv, var
        self.end = self.offsets[-1] + max(1, self.factors[-1][0] * max(1, self.factors[-1][1]) * self.factors[-1][2])
        self.ws_floats = 0


def adafactor_step_cpu(plan, pflat, gflat, row_var, col_var, variance, step, lr, beta2_decay=-0.8, eps1=None, eps2=1e-3, d=1.0, weight_decay=0.0,
                       grad_scale=1.0):
    """fp32 arithmetic in plain torch, the state in fp32, p rounded once into the arena dtype — an independent evaluation of the rule, not a copy of
    the kernels' summation order"""
    if eps1 is None:
        eps1 = torch.finfo(pflat.dtype).eps
    c = scalars_f32(step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale)
    for i, ((batch, R, C), off) in enumerate(zip(plan.factors, plan.offsets)):
        k = batch * max(R, 1) * C
        shape3 = (C,) if R == 0 else (batch, R, C)
        p, g = pflat[off:off + k].view(shape3), gflat[off:off + k].view(shape3)
        if R == 0:
            state = {"variance": variance[plan.var_offsets[i]:plan.var_offsets[i] + C]}
        else:
            state = {"row_var": row_var[plan.rv_offsets[i]:plan.rv_offsets[i] + batch * R].view(batch, R, 1),
                     "col_var": col_var[plan.cv_offsets[i]:plan.cv_offsets[i] + batch * C].view(batch, 1, C)}
        new, _ = step_tensor(p.to(F32), g.to(F32), state, c)
        p.copy_(new)                                           # one rounding into the arena dtype (nearest even)


def install(monkeypatch):
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "AdafactorPlan", AdafactorPlanCPU)
    monkeypatch.setattr(ops, "adafactor_step", adafactor_step_cpu)

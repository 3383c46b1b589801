"""Fused AdamW(+EMA) optimizer — the entry a maintainer adds to `optimizer_choices`
(simpletuner/helpers/training/optimizer_param.py:76-96): {"precision": "any", "default_settings": {...}, "class": St355AdamW}.

torch.optim.AdamW semantics (decoupled decay, bias correction; optimizer_param.py:87-96 defaults), executed by
st355_adamw_ema_step: when the group's parameters are views of one contiguous arena (the LoRA flat arena, or a bf16
full-fine-tune arena) the whole step is ONE launch over the arena; otherwise one launch per tensor.  Standard
torch.optim.Optimizer API so `accelerator.prepare(optimizer)` / `accelerator.save_state` work unchanged.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

from .. import ops

F32 = torch.float32


def _contiguous_run(tensors):
    """True if `tensors` are back-to-back views of one allocation (same dtype), in order."""
    if not tensors:
        return False
    dt = tensors[0].dtype
    ptr = tensors[0].data_ptr()
    for t in tensors:
        if t.dtype != dt or not t.is_contiguous() or t.data_ptr() != ptr:
            return False
        ptr += t.numel() * t.element_size()
    return True


def flat_view(tensors):
    """The 1-D view over `tensors` when they are back-to-back views of one allocation (`_contiguous_run`), else None — also for an empty list or a
    list with a missing (None) entry, so callers need no pre-check.  Writes through the view land in the tensors."""
    if not tensors or any(t is None for t in tensors) or not _contiguous_run(tensors):
        return None
    return torch.as_strided(tensors[0], (sum(t.numel() for t in tensors),), (1,))


def _unpack_saved_state(opt: torch.optim.Optimizer, state_dict: dict):
    """torch.optim.Optimizer.load_state_dict's matching rules (groups by position, parameters by position inside a group; saved hyper-parameters
    replace the live ones) WITHOUT its dtype policy: torch casts every floating state tensor to the parameter's dtype, which would round the fp32
    moments of bf16 parameters to bf16 on every resume.  Returns {param: saved per-parameter state}."""
    saved_groups = state_dict["param_groups"]
    if len(saved_groups) != len(opt.param_groups):
        raise ValueError("loaded state dict has a different number of parameter groups")
    by_param = {}
    for saved, live in zip(saved_groups, opt.param_groups):
        if len(saved["params"]) != len(live["params"]):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for k, v in saved.items():
            if k != "params":
                live[k] = v
        for pid, p in zip(saved["params"], live["params"]):
            if pid in state_dict["state"]:
                by_param[p] = state_dict["state"][pid]
    return by_param


class _ArenaOptimizer(torch.optim.Optimizer):
    """What the fused arena optimizers (AdamW, AdamWBF16, Lion, Muon, SOAP, Adafactor) share: per parameter group, flat state buffers over the group's trainable parameters with the torch-compatible
    per-parameter state installed as views of them (`_flat[gi]`: ok, ps, n, one entry per declared buffer, the subclass's extras); a
    `load_state_dict` that copies a checkpoint INTO those buffers in the dtype each is kept in; and the test for the one-launch path.
    A subclass declares `_buffers`, adds its extras in `_group_extras` / `_load_extras`, and issues its `ops.*` calls in `step`."""
    fuses_ema = False        # True where the kernel can apply the EMA update in the same launch (the trainer then hands over ema_shadow_flat / ema_decay)
    always_flat = False      # True: flat state buffers even when the parameters are not one contiguous run
    _buffers: Dict[str, tuple] = {}    # per-parameter state key -> (key in _flat[gi], dtype; None = the parameter's own)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.grad_scale = 1.0           # set by the gradient-sync layer (1/world_size) or by clipping: folded into the kernel
        self.ema_shadow_flat: Optional[torch.Tensor] = None   # optional fused EMA (flat arena path only; used where fuses_ema)
        self.ema_decay = 0.0
        self.ema_applied = False
        self._flat = {}

    # ---- what a subclass may override ----
    def _group_params(self, group):
        return [p for p in group["params"] if p.requires_grad]

    def _check_param(self, p) -> None:
        """refuse a parameter this optimizer cannot step"""

    def _buffer_dtype(self, key, group, p):
        """dtype of state buffer `key` for parameters like p, or None where the group carries no such buffer"""
        dtype = self._buffers[key][1]
        return p.dtype if dtype is None else dtype

    def _group_extras(self, gi, group, st) -> None:
        """whatever `_flat[gi]` and the per-parameter states hold beyond the declared buffers"""

    def _load_extras(self, st, mine, old) -> None:
        """restore one parameter's extras (`mine`: its live state, `old`: its saved state)"""

    # ---- group construction ----
    def _build_group(self, gi, group):
        ps = self._group_params(group)
        for p in ps:
            self._check_param(p)
        st = dict(ok=flat_view([p.data for p in ps]) is not None, ps=ps, n=sum(p.numel() for p in ps))
        flat = st["ok"] or self.always_flat
        for key, (flat_key, _) in self._buffers.items():
            dtype = self._buffer_dtype(key, group, ps[0]) if flat else None
            st[flat_key] = None if dtype is None else torch.zeros(st["n"], dtype=dtype, device=ps[0].device)
        if flat:
            off = 0
            for p in ps:   # torch-compatible per-parameter state = views of the flat buffers
                self.state[p] = {key: st[flat_key][off:off + p.numel()].view_as(p)
                                 for key, (flat_key, _) in self._buffers.items() if st[flat_key] is not None}
                off += p.numel()
        self._group_extras(gi, group, st)
        self._flat[gi] = st
        return st

    def _group_flat(self, gi, group):
        st = self._flat.get(gi)
        return st if st is not None else self._build_group(gi, group)

    def _tensor_state(self, group, p):
        """p's state with every declared buffer present: the flat views where the group has them, else per-tensor buffers created on first use"""
        s = self.state[p]
        for key in self._buffers:
            if key not in s:
                dtype = self._buffer_dtype(key, group, p)
                if dtype is not None:
                    s[key] = torch.zeros(p.numel(), dtype=dtype, device=p.device).view_as(p)
        return s

    # ---- resume ----
    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """resume (`accelerator.load_state`, save_hooks.py): the saved per-parameter buffers are copied INTO the flat buffers (created here if the
        optimizer has not stepped yet), each in the dtype this optimizer keeps it in, so the one-launch path continues from them; `_load_extras`
        restores the rest"""
        saved = _unpack_saved_state(self, state_dict)
        self._flat = {}
        for p in list(self.state):
            del self.state[p]
        for gi, group in enumerate(self.param_groups):
            st = self._build_group(gi, group)
            for p in st["ps"]:
                old = saved.get(p)
                if not old:
                    continue
                mine = self._tensor_state(group, p)
                for key in self._buffers:
                    if key in mine and old.get(key) is not None:
                        mine[key].copy_(old[key].to(device=p.device, dtype=mine[key].dtype).view_as(p))
                self._load_extras(st, mine, old)

    # ---- the one-launch path ----
    def _fused_views(self, st, ps):
        """(pflat, gflat, ema) when `ps` are all of the group's parameters and they and their gradients are contiguous runs, else None.  ema is the
        shadow arena the launch should update as well: only with one group, of the arena's length and dtype"""
        if not st["ok"] or len(ps) != len(st["ps"]):
            return None
        gflat = flat_view([p.grad for p in ps])
        pflat = flat_view([p.data for p in ps]) if gflat is not None else None
        if pflat is None:
            return None
        ema = self.ema_shadow_flat if self.fuses_ema else None
        if ema is not None and not (len(self.param_groups) == 1 and ema.numel() == st["n"] and ema.dtype == pflat.dtype):
            ema = None
        return pflat, gflat, ema


class St355AdamW(_ArenaOptimizer):
    fuses_ema = True
    _buffers = {"exp_avg": ("m", F32), "exp_avg_sq": ("v", F32)}     # fp32 moments, also for bf16 parameters

    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, **_ignored):
        if amsgrad:
            raise NotImplementedError("amsgrad is not implemented in the fused kernel")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _group_extras(self, gi, group, st):
        st["step"] = 0
        if st["ok"]:
            for p in st["ps"]:
                self.state[p]["step"] = torch.tensor(0.0)

    def _tensor_state(self, group, p):
        s = super()._tensor_state(group, p)
        if "step" not in s:
            s["step"] = torch.tensor(0.0)
        return s

    def _load_extras(self, st, mine, old):
        k = int(float(old["step"]))
        mine["step"] = torch.tensor(float(k))
        st["step"] = max(st["step"], k)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for gi, group in enumerate(self.param_groups):
            st = self._group_flat(gi, group)
            ps = [p for p in st["ps"] if p.grad is not None]
            if not ps:
                continue
            b1, b2 = group["betas"]
            st["step"] += 1
            step = st["step"]
            fused = self._fused_views(st, ps)
            if fused is not None:
                pflat, gflat, ema = fused
                ops.adamw_ema_step(pflat, gflat, st["m"], st["v"], step, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                   grad_scale=self.grad_scale, ema=ema, ema_decay=self.ema_decay)
                self.ema_applied = ema is not None      # the trainer falls back to EMAModel.step when the fused form did not run
                for p in ps:
                    self.state[p]["step"] += 1
                continue
            for p in ps:   # generic path: one launch per tensor
                s = self._tensor_state(group, p)
                s["step"] += 1
                g = p.grad.contiguous()
                if g.dtype != p.dtype:
                    g = g.to(p.dtype)
                ops.adamw_ema_step(p.data.view(-1), g.view(-1), s["exp_avg"].view(-1), s["exp_avg_sq"].view(-1), int(s["step"].item()),
                                   group["lr"], b1, b2, group["eps"], group["weight_decay"], grad_scale=self.grad_scale)
        return loss


class St355AdamWBF16(_ArenaOptimizer):
    """AdamWBF16 — the reference examples' default optimizer (optimizers/adamw_bfloat16/__init__.py:20-111), as ONE fused launch.

    Same constructor (keyword-only lr, betas, eps, weight_decay), same `step(zero_grad=False)`, same per-parameter state keys
    (`step`, `exp_avg`, `exp_avg_sq`, `shift`, `accumulated_decay`) so `accelerator.save_state` round-trips; the states are views of
    flat bf16 arenas.  The per-tensor delayed-decay schedule (decay owed += weight_decay*lr; applied only above 5e-3; random initial
    phase per tensor) is host arithmetic exactly as in the reference; the element-wise math is st355_adamw_bf16_sr_step.
    Parameters must be bf16 and, for the fused path, views of one contiguous arena (as the full-fine-tune engine allocates them);
    otherwise one launch per tensor.  `rand_bits_hook(p_index, step) -> int32[4, n]` lets parity tests inject the reference's draws."""
    decay_threshold = 5e-3
    always_flat = True
    _buffers = {"exp_avg": ("m", torch.bfloat16), "exp_avg_sq": ("v", torch.bfloat16), "shift": ("shift", torch.bfloat16)}

    def __init__(self, params, *, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, seed: int = 0):
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(betas=betas, eps=eps, weight_decay=weight_decay, lr=lr))
        self.seed = int(seed)
        self.rand_bits_hook = None
        self._launches = 0

    def _check_param(self, p):
        assert p.dtype == torch.bfloat16, "only bfloat 16 is supported."

    def _init_group(self, gi, group):
        return self._build_group(gi, group)

    def _group_extras(self, gi, group, st):
        st["step"] = 0
        # "Each weight has its own starting point to avoid simultaneous updates in all weights" (:80-84).  The reference draws these phases from the
        # global torch RNG; here they come from a generator private to (optimizer seed, group), so data-parallel replicas — whose global RNG streams
        # differ by rank — release their delayed decay on the same steps and stay bit-identical.
        phase_rng = torch.Generator().manual_seed(1_000_003 * self.seed + gi)
        ends, off = [], 0
        for p in st["ps"]:
            self.state[p].update(step=0.0, accumulated_decay=float(torch.rand([], generator=phase_rng) * self.decay_threshold))
            off += p.numel()
            ends.append(off)
        st["seg_end"] = torch.tensor(ends, dtype=torch.int64, device=st["ps"][0].device)

    def _load_extras(self, st, mine, old):
        """per-tensor step and the owed decay: the delayed-decay phase of every tensor continues where it stopped
        (optimizers/adamw_bfloat16/__init__.py:80-95)"""
        mine["step"] = float(old["step"])
        mine["accumulated_decay"] = float(old["accumulated_decay"])
        st["step"] = max(st["step"], int(float(old["step"])))

    @torch.no_grad()
    def step(self, zero_grad: bool = False, closure=None):
        loss = closure() if closure is not None else None
        for gi, group in enumerate(self.param_groups):
            st = self._group_flat(gi, group)
            ps = st["ps"]
            if any(p.grad is None for p in ps):
                raise RuntimeError("St355AdamWBF16 expects a gradient for every parameter of the group (fused arena step)")
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            st["step"] += 1
            decays = []
            for p in ps:                                   # reference :89-95, host scalars
                s = self.state[p]
                s["step"] += 1
                s["accumulated_decay"] += group["weight_decay"] * lr
                acc = s["accumulated_decay"]
                dec = acc if acc > self.decay_threshold else 0.0
                s["accumulated_decay"] -= dec
                decays.append(dec)
            if any(d != 0.0 for d in decays):
                seg_decay = torch.tensor(decays, dtype=F32, device=ps[0].device)
            else:
                # no tensor releases its owed decay this step (the common case: weight_decay * lr per step against the 5e-3 threshold): a resident zero vector —
                # the host->device copy of the list is a blocking copy, i.e. a host sync in every step (6.8 ms of a 100 ms graph-replayed step, measured r5)
                seg_decay = st.get("zero_decay")
                if seg_decay is None:
                    seg_decay = st["zero_decay"] = torch.zeros(len(ps), dtype=F32, device=ps[0].device)
            fused = self._fused_views(st, ps) if self.rand_bits_hook is None else None
            if fused is not None:
                pflat, gflat, _ = fused
                ops.adamw_bf16_sr_step(pflat, gflat, st["m"], st["v"], st["shift"], st["step"], lr, beta1, beta2, group["eps"],
                                       seg_end=st["seg_end"], seg_decay=seg_decay, seed=self.seed, offset=4 * st["n"] * st["step"],
                                       grad_scale=self.grad_scale)
                self._launches += 1
            else:
                off = 0
                for i, p in enumerate(ps):
                    k = p.numel()
                    g = p.grad.contiguous().view(-1)
                    rb = self.rand_bits_hook(i, st["step"]) if self.rand_bits_hook is not None else None
                    ops.adamw_bf16_sr_step(p.data.view(-1), g, st["m"][off:off + k], st["v"][off:off + k], st["shift"][off:off + k],
                                           st["step"], lr, beta1, beta2, group["eps"], seg_end=st["seg_end"][i:i + 1] - off,
                                           seg_decay=seg_decay[i:i + 1], rand_bits=rb, seed=self.seed + i,
                                           offset=4 * k * st["step"], grad_scale=self.grad_scale)
                    self._launches += 1
                    off += k
            if zero_grad:
                for p in ps:
                    p.grad.zero_()
        return loss


class St355Lion(_ArenaOptimizer):
    """Lion (Chen et al. 2023) with the constructor of optimi's Lion — the reference's "optimi-lion" entry (optimizer_param.py:327-338) — as ONE
    st355_lion_step launch per parameter group when the group's parameters and gradients are contiguous runs (the LoRA adapter arena in fp32,
    a full-fine-tune arena in bf16), else one launch per tensor.

    Per-parameter state: `exp_avg` in the parameter's dtype and, for bf16 parameters with `kahan_sum` true or None, `kahan_comp` (bf16) — views of
    flat buffers on the one-launch path.  fp32 parameters never carry a compensation buffer.  Weight decay is decoupled and scaled by the
    learning rate (decouple_lr=False); `decouple_lr=True` is refused, `max_lr` only matters there; `foreach` is accepted and ignored.  optimi is
    not executed anywhere in this project: the rule is the published one, and exchanging optimizer checkpoints with optimi
    itself is unverified."""
    fuses_ema = True
    _buffers = {"exp_avg": ("m", None), "kahan_comp": ("comp", torch.bfloat16)}

    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.99), weight_decay: float = 0.0, decouple_lr: bool = False, max_lr=None,
                 kahan_sum=True, foreach=True, **_ignored):
        if decouple_lr:
            raise NotImplementedError("optimi-lion: decouple_lr=True (fully decoupled weight decay) is not built on the st355 path")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: lr={lr}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta1 parameter: beta1={betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta2 parameter: beta2={betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight decay: weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay, decouple_lr=False, max_lr=max_lr, kahan_sum=kahan_sum))

    def _check_param(self, p):
        if p.dtype not in (F32, torch.bfloat16):
            raise NotImplementedError(f"optimi-lion: parameters must be fp32 or bf16 on the st355 path, got {p.dtype}")

    def _buffer_dtype(self, key, group, p):
        if key == "kahan_comp" and not (p.dtype == torch.bfloat16 and group["kahan_sum"] in (True, None)):
            return None          # fp32 parameters, or kahan_sum=False: no compensation buffer
        return super()._buffer_dtype(key, group, p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for gi, group in enumerate(self.param_groups):
            st = self._group_flat(gi, group)
            ps = [p for p in st["ps"] if p.grad is not None]
            if not ps:
                continue
            b1, b2 = group["betas"]
            fused = self._fused_views(st, ps)
            if fused is not None and fused[1].dtype == fused[0].dtype:
                pflat, gflat, ema = fused
                ops.lion_step(pflat, gflat, st["m"], group["lr"], b1, b2, group["weight_decay"], grad_scale=self.grad_scale, comp=st["comp"],
                              ema=ema, ema_decay=self.ema_decay)
                self.ema_applied = ema is not None      # the trainer falls back to EMAModel.step when the fused form did not run
                continue
            for p in ps:   # generic path: one launch per tensor
                s = self._tensor_state(group, p)
                g = p.grad.contiguous()
                if g.dtype != p.dtype:
                    g = g.to(p.dtype)
                comp = s.get("kahan_comp")
                ops.lion_step(p.data.view(-1), g.view(-1), s["exp_avg"].view(-1), group["lr"], b1, b2, group["weight_decay"],
                              grad_scale=self.grad_scale, comp=None if comp is None else comp.view(-1))
        return loss


# ---- Muon ------------------------------------------------------------------------------------------------------------------------
MUON_NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)     # muon/__init__.py:16-19 (DEFAULT_A, DEFAULT_B, DEFAULT_C)
MUON_NS_STEPS = 5
MUON_EPS = 1e-7
MUON_MAX_SHORT_SIDE = 128


def muon_cans_coefficients(ns_steps: int, cans_a_bound: float):
    """the CANS schedule of muon/__init__.py:45-78 in float64 on the host: iteration i is X <- c1 X + c3 (X X^T) X, i.e. (a, b, c) = (c1, c3, 0)"""
    lower, upper, inv_3 = float(cans_a_bound), 1.0, 1.0 / 3.0
    out = []
    for _ in range(ns_steps):
        a_sq, b_sq, ab = lower * lower, upper * upper, lower * upper
        e_sq = (a_sq + ab + b_sq) * inv_3
        e_pow_1_5 = e_sq * math.sqrt(e_sq)
        common_den_part = 2.0 * e_pow_1_5
        ab_part = a_sq * upper + b_sq * lower
        alpha_den = common_den_part + ab_part
        alpha = 6.0 / alpha_den
        out.append((alpha * e_sq, -alpha * inv_3, 0.0))
        eps_val = (common_den_part - ab_part) / alpha_den
        lower, upper = 1.0 - eps_val, 1.0 + eps_val
    return out


def muon_coefficients(group: dict):
    """one (a, b, c) per Newton-Schulz iteration for a parameter group's settings"""
    if group["use_cans"]:
        return muon_cans_coefficients(group["ns_steps"], group["cans_a_bound"])
    return [tuple(float(v) for v in group["ns_coefficients"])] * group["ns_steps"]


class St355Muon(_ArenaOptimizer):
    """MuonClip (optimizers/muon/__init__.py) over the fp32 adapter arena, as one st355_muon_step call per parameter group.

    Same constructor (every keyword of MuonClip), same `step(closure=None, attention_max_logits=None)`, same per-parameter state keys
    (`momentum_buffer`, `factored=False`; the buffers are views of one flat fp32 arena), same `register_attention_params[_from_model]` and
    `state_dict()["param_names"]`.  The arithmetic is the reference's intent, not its literal output: the Newton-Schulz
    iterate is never written over its own input and the momentum buffer keeps m.  Parameters must be 2-D fp32 views of one contiguous arena
    with a short side of at most 128 (the LoRA adapter arena); `stochastic_rounding` is accepted and, as for the reference's non-bf16
    parameters, has no effect.  `use_smmf` and `vector_reshape` are refused."""
    _buffers = {"momentum_buffer": ("m", F32)}

    def __init__(self, params, lr: float = 2e-4, momentum: float = 0.95, weight_decay: float = 0.1, qk_clip_threshold: float = 100.0,
                 qk_clip_alpha: float = 0.5, ns_steps: int = MUON_NS_STEPS, ns_coefficients=MUON_NS_COEFFICIENTS, eps: float = MUON_EPS,
                 rms_scale_factor: float = 0.2, use_smmf: bool = False, vector_reshape: bool = False, stochastic_rounding: bool = True,
                 use_cans: bool = False, cans_a_bound: float = 1e-4):
        if lr < 0.0:                                               # muon/__init__.py:171-180, same texts
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0 or momentum >= 1.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if ns_steps >= 100:
            raise ValueError("Number of steps must be less than 100 for computational efficiency")
        if not use_cans and len(ns_coefficients) != 3:
            raise ValueError("ns_coefficients must be a tuple of exactly 3 values")
        if use_smmf:
            raise NotImplementedError("muon: use_smmf (the factored momentum) is not built on the st355 path")
        if vector_reshape:
            raise NotImplementedError("muon: vector_reshape (factored 1-D momentum) is not built on the st355 path")
        if ns_steps < 1:
            raise NotImplementedError("muon: ns_steps must be at least 1 on the st355 path")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, qk_clip_threshold=qk_clip_threshold, qk_clip_alpha=qk_clip_alpha,
                        ns_steps=ns_steps, ns_coefficients=ns_coefficients, eps=eps, rms_scale_factor=rms_scale_factor, use_smmf=use_smmf,
                        vector_reshape=vector_reshape, use_cans=use_cans, cans_a_bound=cans_a_bound)
        super().__init__(params, defaults)
        for group in self.param_groups:
            ps = group["params"]
            for i, p in enumerate(ps):
                if p.dim() != 2:
                    raise NotImplementedError(f"muon: parameter {i} has {p.dim()} dimensions; only 2-D matrices are built on the st355 path")
                if min(p.shape) > MUON_MAX_SHORT_SIDE:
                    raise NotImplementedError(f"muon: parameter {i} of shape {tuple(p.shape)} has a short side above {MUON_MAX_SHORT_SIDE}")
                if p.dtype != F32:
                    raise NotImplementedError(f"muon: parameter {i} is {p.dtype}; the st355 path steps fp32 adapter values")
            if flat_view([p.data for p in ps]) is None:
                raise NotImplementedError("muon: the parameters of a group must be one contiguous fp32 run (the adapter arena)")
        self.stochastic_rounding = stochastic_rounding
        self._param_to_name: Dict[int, str] = {}
        self.abi_calls = 0              # st355 calls issued by step(): one per parameter group, whatever the number of matrices

    def _group_params(self, group):
        return list(group["params"])

    def _group_extras(self, gi, group, st):
        ps = st["ps"]
        base = ps[0].data_ptr()
        st["plan"] = ops.MuonPlan([(p.data_ptr() - base) // 4 for p in ps], [tuple(p.shape) for p in ps], ps[0].device)
        for p in ps:   # MuonClip's per-parameter state (:243-244)
            self.state[p]["factored"] = False

    @torch.no_grad()
    def step(self, closure=None, attention_max_logits: Optional[Dict[str, torch.Tensor]] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if attention_max_logits is not None:
            self._check_qk_clip(attention_max_logits)
        for gi, group in enumerate(self.param_groups):
            if all(p.grad is None for p in group["params"]):
                continue
            st = self._group_flat(gi, group)
            fused = self._fused_views(st, st["ps"])
            if fused is None:
                raise RuntimeError("St355Muon expects the gradients of every parameter of a group as one flat fp32 arena (fused step)")
            pflat, gflat, _ = fused
            ops.muon_step(st["plan"], pflat, gflat, st["m"], muon_coefficients(group), group["lr"], momentum=group["momentum"],
                          weight_decay=group["weight_decay"], eps=group["eps"], rms_scale_factor=group["rms_scale_factor"],
                          grad_scale=self.grad_scale)
            self.abi_calls += 1
        return loss

    def _check_qk_clip(self, attention_max_logits: Dict[str, torch.Tensor]) -> None:
        """MuonClip._apply_qk_clip (:347-378) matches parameters to the published max logits by name and skips the rest.  Under LoRA no trained
        parameter's name is ever published (the logits are keyed by the base layer's weight), so the clip never runs; a match would mean a
        clip this path does not implement, and is refused rather than skipped"""
        for group in self.param_groups:
            for p in group["params"]:
                name = self._get_param_name(p)
                if name and name in attention_max_logits:
                    raise NotImplementedError(f"muon: QK-clip of trained parameter '{name}' is not built on the st355 path")

    def _get_param_name(self, param: torch.Tensor) -> str:
        return self._param_to_name.get(id(param), "")

    def register_attention_params(self, param_name_mapping: Dict[str, torch.nn.Parameter]) -> None:
        self._param_to_name.update({id(param): name for name, param in param_name_mapping.items()})

    def register_attention_params_from_model(self, model: torch.nn.Module, name_filter: Optional[Callable[[str], bool]] = None) -> None:
        if model is None:
            return
        if name_filter is None:
            name_filter = lambda n: ("attn" in n.lower() or "attention" in n.lower()) and ("q" in n.lower() or "k" in n.lower())  # noqa: E731
        mapping = {name: param for name, param in model.named_parameters() if param is not None and name_filter(name)}
        if mapping:
            self.register_attention_params(mapping)

    def state_dict(self) -> Dict[str, object]:
        base = super().state_dict()
        base["param_names"] = {gi: [self._param_to_name.get(id(p), "") for p in group.get("params", [])] for gi, group in enumerate(self.param_groups)}
        return base

    def load_state_dict(self, state_dict: dict) -> None:
        """resume: the momentum buffers as in the base class; the saved parameter names are registered again (MuonClip.load_state_dict)"""
        super().load_state_dict(state_dict)
        for gi, names in (state_dict.get("param_names") or {}).items():
            gi = int(gi)
            if gi >= len(self.param_groups):
                continue
            for p, name in zip(self.param_groups[gi].get("params", []), names):
                if name:
                    self._param_to_name[id(p)] = name


# ---- SOAP ------------------------------------------------------------------------------------------------------------------------
SOAP_MAX_SHORT_SIDE = 128


class St355Soap(_ArenaOptimizer):
    """SOAP (optimizers/soap/__init__.py: Adam in the eigenbasis of Shampoo's preconditioner) over the fp32 adapter arena, as one st355_soap_step
    call per parameter group, with the RANK side of every adapter matrix preconditioned and the long side left as identity: every parameter
    needs short <= max_precond_dim < long (DESIGN.md §7 — with the long side preconditioned as well the reference's own trajectory is not
    reproducible, so that is refused, not approximated).

    Same constructor (every keyword of SOAP, same defaults), same per-parameter state in the reference's layout: `step` (int), `exp_avg`
    (original basis), `exp_avg_sq` (rotated basis), `GG` and `Q` as two-element lists with `[]` on the identity side, `precondition_frequency`,
    `shampoo_beta` — the tensors are views of flat fp32 buffers, and a `state_dict()` of the reference class loads here.  The first call only
    builds GG and its eigenbasis (:138-155); afterwards the basis is refreshed after the update of every step with step % precondition_frequency
    == 0 (:331-332).  Parameters must be 2-D fp32 views of one contiguous arena with a short side of at most 128.  `merge_dims` and
    `normalize_grads` are refused; `precondition_1d` and `data_format` have no effect on 2-D parameters and are accepted."""
    _buffers = {"exp_avg": ("m", F32), "exp_avg_sq": ("v", F32)}

    def __init__(self, params, lr: float = 3e-3, betas=(0.95, 0.95), shampoo_beta: float = -1, eps: float = 1e-8, weight_decay: float = 0.01,
                 precondition_frequency: int = 10, max_precond_dim: int = 10000, merge_dims: bool = False, precondition_1d: bool = False,
                 normalize_grads: bool = False, data_format: str = "channels_first", correct_bias: bool = True):
        if merge_dims:
            raise NotImplementedError("soap: merge_dims=True is not built on the st355 path")
        if normalize_grads:
            raise NotImplementedError("soap: normalize_grads=True (a per-tensor mean before the apply) is not built on the st355 path")
        if int(precondition_frequency) < 1:
            raise ValueError(f"Invalid precondition_frequency: {precondition_frequency}")
        defaults = dict(lr=lr, betas=betas, shampoo_beta=shampoo_beta, eps=eps, weight_decay=weight_decay,
                        precondition_frequency=precondition_frequency, max_precond_dim=max_precond_dim, merge_dims=merge_dims,
                        precondition_1d=precondition_1d, normalize_grads=normalize_grads, correct_bias=correct_bias)
        super().__init__(params, defaults)
        self._data_format = data_format
        for group in self.param_groups:
            ps = group["params"]
            mpd = group["max_precond_dim"]
            for i, p in enumerate(ps):
                if p.dim() != 2:
                    raise NotImplementedError(f"soap: parameter {i} has {p.dim()} dimensions; only 2-D matrices are built on the st355 path")
                if p.dtype != F32:
                    raise NotImplementedError(f"soap: parameter {i} is {p.dtype}; the st355 path steps fp32 adapter values")
                short, long = min(p.shape), max(p.shape)
                if short > SOAP_MAX_SHORT_SIDE:
                    raise NotImplementedError(f"soap: parameter {i} of shape {tuple(p.shape)} has a short side above {SOAP_MAX_SHORT_SIDE}")
                if not short <= mpd < long:
                    hint = SOAP_MAX_SHORT_SIDE if short <= SOAP_MAX_SHORT_SIDE < long else short
                    raise NotImplementedError(
                        f"soap: max_precond_dim={mpd} with parameter {i} of shape {tuple(p.shape)} is not built on the st355 path: only the rank side "
                        f"is preconditioned, which needs {short} <= max_precond_dim <= {long - 1} (short side <= max_precond_dim < long side); "
                        f"set --optimizer_config=max_precond_dim={hint}")
            if flat_view([p.data for p in ps]) is None:
                raise NotImplementedError("soap: the parameters of a group must be one contiguous fp32 run (the adapter arena)")
        self.abi_calls = 0              # st355 calls issued by step(): one per parameter group, whatever the number of matrices

    def _group_params(self, group):
        return list(group["params"])

    def _group_extras(self, gi, group, st):
        ps = st["ps"]
        base = ps[0].data_ptr()
        plan = st["plan"] = ops.SoapPlan([(p.data_ptr() - base) // 4 for p in ps], [tuple(p.shape) for p in ps], ps[0].device)
        st["gg"] = torch.zeros(plan.qq, dtype=F32, device=ps[0].device)
        st["q"] = torch.zeros(plan.qq, dtype=F32, device=ps[0].device)
        st["step"] = 0
        st["ready"] = False             # True once the first call has built the eigenbasis
        st["precondition_frequency"] = int(group["precondition_frequency"])
        st["shampoo_beta"] = float(group["shampoo_beta"] if group["shampoo_beta"] >= 0 else group["betas"][1])     # :144
        for p, off, r in zip(ps, plan.q_offsets, plan.short):
            gg, q = st["gg"][off:off + r * r].view(r, r), st["q"][off:off + r * r].view(r, r)
            wide = p.shape[0] < p.shape[1]
            self.state[p].update(step=0, GG=[gg, []] if wide else [[], gg], Q=[q, []] if wide else [[], q],
                                 precondition_frequency=st["precondition_frequency"], shampoo_beta=st["shampoo_beta"])

    def _load_extras(self, st, mine, old):
        """the preconditioner, its eigenbasis and the counters of one parameter (reference layout: the matrix on the rank side, [] on the other)"""
        for key in ("GG", "Q"):
            saved = old.get(key)
            if saved is None:
                continue
            for dst, src in zip(mine[key], saved):
                if torch.is_tensor(dst) != torch.is_tensor(src) or (torch.is_tensor(dst) and dst.shape != src.shape):
                    raise NotImplementedError(f"soap: the saved {key} preconditions another side than the st355 path (max_precond_dim must lie between "
                                              "the two sides of every parameter)")
                if torch.is_tensor(dst):
                    dst.copy_(src.to(device=dst.device, dtype=F32))
        k = int(old.get("step", 0))
        mine["step"] = k
        # the basis exists once the first call has run: the buffers hold an all-zero Q until then (also in a checkpoint written before any step)
        ready = old.get("Q") is not None and any(torch.is_tensor(t) and bool(t.any()) for t in old["Q"])
        freq, sb = int(old.get("precondition_frequency", st["precondition_frequency"])), float(old.get("shampoo_beta", st["shampoo_beta"]))
        if st.get("_loaded") and (st["step"], st["ready"], st["precondition_frequency"], st["shampoo_beta"]) != (k, ready, freq, sb):
            raise NotImplementedError("soap: the parameters of a group must share step, precondition_frequency and shampoo_beta (one fused call)")
        st.update(step=k, ready=ready, precondition_frequency=freq, shampoo_beta=sb, _loaded=True)
        mine["precondition_frequency"], mine["shampoo_beta"] = freq, sb

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for gi, group in enumerate(self.param_groups):
            if all(p.grad is None for p in group["params"]):
                continue
            st = self._group_flat(gi, group)
            fused = self._fused_views(st, st["ps"])
            if fused is None:
                raise RuntimeError("St355Soap expects the gradients of every parameter of a group as one flat fp32 arena (fused step)")
            pflat, gflat, _ = fused
            b1, b2 = group["betas"]
            lr = group["lr"]
            first = not st["ready"]
            step_size, refresh = 0.0, False
            if not first:
                st["step"] += 1
                t = st["step"]
                step_size = lr
                if group["correct_bias"]:                                      # :187-191, host doubles
                    step_size = step_size * ((1.0 - b2 ** t) ** 0.5) / (1.0 - b1 ** t)
                refresh = t % st["precondition_frequency"] == 0               # :331-332
            ops.soap_step(st["plan"], pflat, gflat, st["m"], st["v"], st["gg"], st["q"], step_size, b1, b2, group["eps"],
                          lr * group["weight_decay"] if group["weight_decay"] > 0.0 else 0.0, 1.0 - st["shampoo_beta"], first, refresh,
                          grad_scale=self.grad_scale)
            st["ready"] = True
            self.abi_calls += 1
            for p in st["ps"]:
                self.state[p]["step"] = st["step"]
        return loss


# ---- Adafactor -------------------------------------------------------------------------------------------------------------------
class St355Adafactor(_ArenaOptimizer):
    """torch.optim.Adafactor — the reference's "torch-adafactor" entry (optimizer_param.py:154-163) — as ONE st355_adafactor_step call (five
    launches) per parameter group, whatever the number of tensors.  The rule is `_single_tensor_adafactor` of the installed torch.

    Same constructor and defaults; `foreach` is accepted and ignored, `maximize=True` and a tensor `lr` are refused.  Per-parameter state in torch's
    layout: `step` (float scalar tensor), `row_var [..., R, 1]` and `col_var [..., 1, C]` for tensors of two or more dims (factored over the last
    two, the leading dims a batch), `variance` like p for 1-D tensors — views of three flat buffers sized by the plan, fp32 also for bf16 parameters
    (torch keeps them in bf16).  No state buffer has the arena's length.  Parameters must be fp32 or bf16 views of one contiguous arena; there is
    no per-tensor path.  A `state_dict()` of torch.optim.Adafactor on the same shapes loads here, in either dtype."""

    def __init__(self, params, lr=1e-2, beta2_decay: float = -0.8, eps=(None, 1e-3), d: float = 1.0, weight_decay: float = 0.0, *, foreach=None,
                 maximize: bool = False):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("torch-adafactor: a tensor lr is not built on the st355 path (the learning rate crosses the ABI as a host scalar)")
        if maximize:
            raise NotImplementedError("torch-adafactor: maximize=True is not built on the st355 path")
        if not 0.0 <= lr:                                             # torch/optim/_adafactor.py:38-49, same texts
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 >= beta2_decay:
            raise ValueError(f"beta2_decay should be <= 0 but is: {beta2_decay}")
        if eps[0] is not None and not 0.0 <= eps[0]:
            raise ValueError(f"epsilon1 should be >= 0 but is: {eps[0]}")
        if not 0.0 <= eps[1]:
            raise ValueError(f"epsilon2 should be >= 0 but is: {eps[1]}")
        if not 1.0 <= d:
            raise ValueError(f"Clipping threshold d should be >= 1 but is: {d}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight_decay should be >= 0 but is: {weight_decay}")
        super().__init__(params, dict(lr=lr, beta2_decay=beta2_decay, eps=tuple(eps), d=d, weight_decay=weight_decay, foreach=foreach, maximize=False))
        self.abi_calls = 0              # st355 calls issued by step(): one per parameter group, whatever the number of tensors

    def _group_params(self, group):
        return list(group["params"])

    def _check_param(self, p):
        if p.dtype not in (F32, torch.bfloat16):
            raise NotImplementedError(f"torch-adafactor: parameters must be fp32 or bf16 on the st355 path, got {p.dtype}")
        if p.dim() < 1 or p.numel() == 0:
            raise NotImplementedError(f"torch-adafactor: a parameter of shape {tuple(p.shape)} is not built on the st355 path")

    def _group_extras(self, gi, group, st):
        ps = st["ps"]
        if not st["ok"]:
            raise NotImplementedError("torch-adafactor: the parameters of a group must be one contiguous run of one dtype (an st355 arena)")
        base, esz, dev = ps[0].data_ptr(), ps[0].element_size(), ps[0].device
        plan = st["plan"] = ops.AdafactorPlan([(p.data_ptr() - base) // esz for p in ps], [tuple(p.shape) for p in ps], dev)
        st["row_var"] = torch.zeros(plan.rv_len, dtype=F32, device=dev)
        st["col_var"] = torch.zeros(plan.cv_len, dtype=F32, device=dev)
        st["variance"] = torch.zeros(plan.var_len, dtype=F32, device=dev)
        st["step"] = 0
        st["step_t"] = torch.tensor(0.0)    # torch's per-parameter `step` (a float scalar tensor): ONE tensor shared by the group's parameters, so a step is one host increment
        for p, (batch, R, C), ro, co, vo in zip(ps, plan.factors, plan.rv_offsets, plan.cv_offsets, plan.var_offsets):
            s = self.state[p]
            s["step"] = st["step_t"]
            if R == 0:
                s["variance"] = st["variance"][vo:vo + C].view_as(p)
            else:
                s["row_var"] = st["row_var"][ro:ro + batch * R].view(*p.shape[:-1], 1)
                s["col_var"] = st["col_var"][co:co + batch * C].view(*p.shape[:-2], 1, p.shape[-1])

    def _load_extras(self, st, mine, old):
        """the factors (or the variance) of one parameter, saved in either dtype, into the fp32 views; the step count is the group's"""
        for key in ("row_var", "col_var", "variance"):
            if (key in mine) != (old.get(key) is not None):
                raise NotImplementedError(f"torch-adafactor: the saved state has {'a' if key not in mine else 'no'} '{key}' for a parameter of "
                                          f"{'one dim' if 'variance' in mine else 'two or more dims'}")
            if key in mine:
                if tuple(old[key].shape) != tuple(mine[key].shape):
                    raise ValueError(f"torch-adafactor: saved '{key}' of shape {tuple(old[key].shape)}, expected {tuple(mine[key].shape)}")
                mine[key].copy_(old[key].to(device=mine[key].device, dtype=F32))
        k = int(float(old["step"]))
        if st.get("_loaded") and st["step"] != k:
            raise NotImplementedError("torch-adafactor: the parameters of a group must share one step count (one fused call)")
        st.update(step=k, _loaded=True)
        st["step_t"].fill_(float(k))

    def state_dict(self):
        """every parameter gets its own copy of the shared `step` tensor: torch's class increments `step` once per parameter, so a state dict whose entries
        shared one tensor would count a step N times there"""
        base = super().state_dict()
        base["state"] = {k: {**v, "step": v["step"].clone()} if "step" in v else v for k, v in base["state"].items()}
        return base

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if all(p.grad is None for p in group["params"]):
                continue
            st = self._group_flat(gi, group)
            fused = self._fused_views(st, st["ps"])
            if fused is None or fused[1].dtype != fused[0].dtype:
                raise RuntimeError("St355Adafactor expects the gradients of every parameter of a group as one flat arena of the parameters' dtype (fused step)")
            pflat, gflat, _ = fused
            st["step"] += 1
            eps1, eps2 = group["eps"]
            ops.adafactor_step(st["plan"], pflat, gflat, st["row_var"], st["col_var"], st["variance"], st["step"], group["lr"], group["beta2_decay"],
                               eps1, eps2, group["d"], group["weight_decay"], self.grad_scale)
            self.abi_calls += 1
            st["step_t"] += 1
        return loss


# what the reference's registry `optimizer_choices` holds for these names (optimizer_param.py:76-96 "st355-adamw"-style entry, the reference's own
# "adamw_bf16", "muon" :432-447, "optimi-lion" :327-338, "soap" :415-431 and "torch-adafactor" :154-163), with the fused classes substituted
OPTIMIZER_CHOICE = {
    "st355-adamw": {
        "precision": "any",
        "default_settings": {"betas": (0.9, 0.999), "weight_decay": 1e-2, "eps": 1e-8},
        "class": St355AdamW,
    },
    "adamw_bf16": {
        "precision": "bf16",
        "default_settings": {"betas": (0.9, 0.999), "weight_decay": 1e-2, "eps": 1e-6},
        "class": St355AdamWBF16,
    },
    "muon": {
        "precision": "any",
        "default_settings": {"momentum": 0.95, "weight_decay": 0.1, "eps": 1e-7, "rms_scale_factor": 0.2, "use_smmf": False, "vector_reshape": False,
                             "stochastic_rounding": True, "use_cans": False, "cans_a_bound": 1e-4, "qk_clip_threshold": 100.0, "qk_clip_alpha": 0.5},
        "class": St355Muon,
    },
    "optimi-lion": {
        "precision": "any",
        "default_settings": {"betas": (0.9, 0.99), "weight_decay": 0.0, "decouple_lr": False, "max_lr": None, "kahan_sum": True, "foreach": True},
        "class": St355Lion,
    },
    "soap": {
        "precision": "any",
        "default_settings": {"betas": (0.95, 0.95), "shampoo_beta": -1, "eps": 1e-8, "weight_decay": 0.01, "precondition_frequency": 10,
                             "max_precond_dim": 10000, "merge_dims": False, "precondition_1d": False, "normalize_grads": False,
                             "data_format": "channels_first", "correct_bias": True},
        "class": St355Soap,
    },
    "torch-adafactor": {
        "precision": "any",
        "default_settings": {"beta2_decay": -0.8, "eps": (None, 1e-3), "d": 1.0, "weight_decay": 0.0},
        "class": St355Adafactor,
    },
}


def parse_optimizer_config(config) -> dict:
    """convert_arg_to_parameters (optimizer_param.py:885-909): `--optimizer_config=k=v,k=v` by the reference's rules, plus the generic beta pair"""
    out = {}
    text = getattr(config, "optimizer_config", None)
    if text is not None and text:
        for param in [kv.split("=") for kv in text.split(",")]:
            if "." in param[1]:
                out[param[0]] = float(param[1])
            elif str(param[1]).isdigit():
                out[param[0]] = int(param[1])
            elif param[1].lower() == "true":
                out[param[0]] = True
            elif param[1].lower() == "false":
                out[param[0]] = False
            elif param[1].lower() == "none":
                out[param[0]] = None
            elif "e-" in param[1]:
                out[param[0]] = float(param[1])
            else:
                out[param[0]] = param[1]
    if getattr(config, "optimizer_beta1", None) is not None and getattr(config, "optimizer_beta2", None) is not None:
        out["betas"] = tuple([config.optimizer_beta1, config.optimizer_beta2])
    return out


def optimizer_settings(name: str, config) -> dict:
    """optimizer_parameters (optimizer_param.py): the registry's default settings updated by the parsed optimizer_config"""
    import copy
    settings = copy.deepcopy(OPTIMIZER_CHOICE[name].get("default_settings", {}))
    settings.update(parse_optimizer_config(config))
    if name == "torch-adafactor" and ("eps1" in settings or "eps2" in settings):
        # the registry's `eps` is a pair, which `k=v,k=v` cannot spell: eps1= / eps2= set its two halves (an explicit eps1 is used as given)
        eps = tuple(settings["eps"])
        settings["eps"] = (settings.pop("eps1", eps[0]), settings.pop("eps2", eps[1]))
    return settings

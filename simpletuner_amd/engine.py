"""Host code the engines share (flux/, sd3/, pixart/ transformer.py, unet/unet.py): nothing here knows a model family.

  * `attach` / `frozen` / `LoraGroup`: parameters under dotted checkpoint names, the adapters of projections that share an input;
  * `AdapterArena` / `lora_pairs`: the ONE fp32 arena of everything trained beside the base (two-phase: plan, build), the A / B pairs of a plan laid out and drawn;
  * `lokr_factorization` / `LokrGroup`: the LyCORIS LoKr adapters of such a group (the Kronecker delta folded into the GEMM operands, the structured gradients);
  * `LoraDropout`: a component's LoRA-dropout state (threshold, Philox key, the device-resident call counter);
  * `LoraDora`: a group's DoRA state (magnitudes, the row scale, the folded GEMM operands);
  * `tlora_active_rank` / `TLora`: T-LoRA's timestep -> active-rank rule, a component's state (the device table) and one forward's binding of it to the timesteps;
  * `lin_w` / `lin_wT` / `lora_down` ... `lora_grads`: one adapter site of a block's forward / backward, phase by phase, a no-op without an adapter;
  * `rows_of` / `problems` / `compact`: a stream's rows of a joint [B * S, C] buffer as GEMM operands;
  * `layersync_indices` / `LayerSyncTap`: the LayerSync regulariser's forward taps and the injection of its gradient into the dX chain;
  * `internal_guidance_index` / `InternalGuidanceHead` / `InternalGuidanceTap`: the Internal Guidance head's parameters, its forward tap and its backward;
  * `nextlat_index` / `NextLatHead` / `NextLatTap`: the NextLat predictor's parameters, its forward tap (the state loss) and its backward;
  * `self_flow_indices` / `SelfFlowHead` / `SelfFlowTap` / `CaptureTap`: Self-Flow's projector, its forward tap (the alignment to the EMA teacher's features) and its
    backward, and the teacher forward's capture tap; `ArenaModule.teacher_values`: the adapter operands packed from another flat buffer (the EMA shadow);
  * `pad64` / `pad64_empty`: operands of the TN weight-gradient GEMM (contraction granule: 64 rows);
  * `ArenaModule`: every base parameter a view of ONE bf16 arena (two-pass construction), checkpoint load / save over the parameter names;
  * `FullGrads`: the per-backward helper of full-rank training — weight / bias gradients into the gradient arena, the modulation rows' reductions, the fused
    modulation matrix's gradient row block by row block, the modulation Linear's and the conditioning MLPs' backward.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

BF16 = torch.bfloat16
F32 = torch.float32


# ------------------------------------------------------------------------------------------------
# helpers to register parameters under dotted (checkpoint) names
# ------------------------------------------------------------------------------------------------
class Holder(nn.Module):
    pass


def attach(root: nn.Module, dotted: str, param: nn.Parameter):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if not hasattr(mod, p):
            mod.add_module(p, Holder())
        mod = getattr(mod, p)
    mod.register_parameter(parts[-1], param)


def frozen(t: torch.Tensor) -> nn.Parameter:
    return nn.Parameter(t, requires_grad=False)


class AdapterArena:
    """The lay-out of everything a model trains beside its frozen base: ONE fp32 arena `model.lora_flat` and its twin `model.lora_grad_flat` (one optimizer launch, one
    exchange over slices of it).  `add` plans a tensor and returns its slot, `lo` / `hi` known at once; `build` allocates both arenas (the total rounded up to 8),
    fills every slot's `p` / `g` (parameter / gradient view), attaches one nn.Parameter per slot in `add` order and publishes `model._lora_params` and
    `model._lora_offsets` [(lo, n)] — what the node's backward cuts the flat gradient by."""

    def __init__(self, model, dev):
        self.model, self.dev, self.slots, self.end = model, dev, [], 0

    def add(self, name: str, shape, align: int = 1):
        lo = (self.end + align - 1) // align * align
        self.end = lo + math.prod(shape)
        self.slots.append(SimpleNamespace(name=name, shape=tuple(shape), lo=lo, hi=self.end, p=None, g=None))
        return self.slots[-1]

    def build(self, seed: int) -> torch.Generator:
        """-> the device generator the initial values are drawn from, seeded"""
        m, total = self.model, (self.end + 7) // 8 * 8
        m.lora_flat, m.lora_grad_flat = torch.zeros(total, dtype=F32, device=self.dev), torch.zeros(total, dtype=F32, device=self.dev)
        m._lora_params, m._lora_offsets = [], [(s.lo, s.hi - s.lo) for s in self.slots]
        for s in self.slots:
            par = nn.Parameter(m.lora_flat[s.lo:s.hi].view(s.shape))
            attach(m, s.name, par)          # (replaces a frozen base-arena view of the same name, when there is one: the heads)
            s.p, s.g = par.data, m.lora_grad_flat[s.lo:s.hi].view(s.shape)
            m._lora_params.append(par)
        return torch.Generator(device=self.dev).manual_seed(seed)


def lora_pairs(arena: AdapterArena, plan, rank: int, init_b_std: float, fan_in: Optional[int] = None, pad=None, divide: bool = False):
    """Plans lora_A [rank, K] / lora_B [N, rank] (peft names) of every (group, name, N, K) of `plan`, pair by pair, and sets the groups' `flat_lo` / `flat_hi`.
    Returns `draw(gen)` for after `arena.build()`: A ~ U(-1, 1) / sqrt(fan_in or K) (kaiming_uniform(a = sqrt 5), peft's default for lora_A), then B ~ N(0, init_b_std)
    if init_b_std > 0 — both drawn at the full shape — and the groups' A / B / gA / gB lists.  pad: a boolean mask of a padded axis' lanes, zeroed in an A whose K
    and a B whose N is that axis.  divide: the draw is divided by sqrt(K), not multiplied by its reciprocal (the last bit differs)."""
    pairs = []
    for (g, name, N, K) in plan:
        sa, sb = arena.add(name + ".lora_A.default.weight", (rank, K)), arena.add(name + ".lora_B.default.weight", (N, rank))
        if not g.flat_hi:
            g.flat_lo = sa.lo
        g.flat_hi = sb.hi
        pairs.append((g, sa, sb))

    def draw(gen):
        for g, sa, sb in pairs:
            (N, _), (_, K) = sb.shape, sa.shape
            u = torch.rand(rank, K, generator=gen, device=arena.dev) * 2 - 1
            sa.p.copy_(u / math.sqrt(K) if divide else u * (1.0 / math.sqrt(fan_in or K)))
            if init_b_std > 0:
                sb.p.copy_(torch.randn(N, rank, generator=gen, device=arena.dev) * init_b_std)
            if pad is not None and K == pad.numel():
                sa.p[:, pad] = 0
            if pad is not None and N == pad.numel():
                sb.p[pad] = 0
            g.A.append(sa.p); g.B.append(sb.p); g.gA.append(sa.g); g.gB.append(sb.g)
    return draw


class LoraDropout:
    """LoRA dropout (peft `lora_dropout`) of one trained component: y = base(x) + (alpha / r) B A dropout(x).  The mask is never stored: a keep bit is a pure
    function of (key, call, stream, row, col) (st355_lora_drop in include/st355.h) that the forward, every recompute pass and the gradient kernels regenerate.
      thr     T = round(p * 65536): an element is dropped iff its 16-bit lane < T; the realised probability is p' = T / 65536, the scale 1 / (1 - p')
      key     (key0, key1) from the run's seed and the data-parallel rank: replicas draw different masks
      call    ONE int32 on the device, read by the kernels through its pointer.  `advance()` — once per training forward of the component, never per recompute —
              is a one-thread launch that belongs to the step: a captured step reads and advances the counter on the device, two replays use different masks.
              A forward uses the value it advanced to, and so does its backward.  `calls` (host) mirrors the eager count for save / resume."""

    def __init__(self, p: float, seed: int, rank: int, device, calls: int = 0):
        self.p = float(p)
        self.thr = ops.lora_dropout_threshold(p)
        self.p_real = self.thr / 65536.0
        seed, rank = int(seed), int(rank)
        self.key0 = seed & 0xFFFFFFFF
        self.key1 = ((seed >> 32) ^ (rank * 0x9E3779B9)) & 0xFFFFFFFF
        self.call = torch.zeros(1, dtype=torch.int32, device=device)
        self.set_calls(calls)

    def set_calls(self, calls: int):
        c = int(calls) & 0xFFFFFFFF
        self.call.fill_(c - (1 << 32) if c >= (1 << 31) else c)           # the kernels read the 32 bits as unsigned

    def calls(self) -> int:
        return int(self.call.item()) & 0xFFFFFFFF

    def advance(self):
        ops.lora_dropout_advance(self.call)


class LoraDora:
    """DoRA (peft `use_dora`; Liu et al. 2024) of one LoraGroup: y = g . (x W^T + s (x A^T) B^T) + b with g = m / ||W + s B A||_row, the norm detached.  The row
    scale is folded into the GEMM operands once per forward (LoraGroup.fold), so every GEMM route and epilogue runs as it is on the folded copies:
      m / gm       the trainable magnitudes of the group's targets and their gradients, [N_total] fp32 views of the arenas
      inv_norm, g  [N_total] fp32 of the last fold
      Wf / WfT     bf16(g . W) and its transpose (what `lin.w` / `lin.wT` are to a plain LoRA);  Bf / BfT  bf16(g . B_blk) and its transpose
    The folded copies double the adapted weights' memory; they live for the whole step."""

    def __init__(self, group, lin, m, gm, flat_lo: int):
        dev = lin.w.device
        N, K, K2 = group.N_total, group.K, group.K2
        self.lin, self.m, self.gm = lin, m, gm
        self.flat_lo, self.flat_hi = flat_lo, flat_lo + N
        self.inv_norm, self.g = torch.zeros(N, dtype=F32, device=dev), torch.zeros(N, dtype=F32, device=dev)
        e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)
        self.Wf, self.WfT, self.Bf, self.BfT = e(N, K), e(K, N), e(N, K2), e(K2, N)


def tlora_active_rank(t: int, T: int, R: int, Rmin: int, alpha: float) -> int:
    """T-LoRA's active rank at integer timestep t (the reference's documentation/experimental/T_LORA.md, "How the masking works internally"), in Python floats
    in exactly this order: r = min(R, int(((T - t) / T) ** alpha * (R - Rmin)) + Rmin)"""
    return min(R, int(((T - t) / T) ** alpha * (R - Rmin)) + Rmin)


class TLora:
    """T-LoRA (LyCORIS `algo: tlora`) of one trained component: every adapted Linear computes y_b = base(x_b) + s (mask_b . (x_b A^T)) B^T with mask_b the first
    r_b rank columns, r_b = tlora_active_rank(int(timestep_b)).  `table`: int32 [T + 1] on the device, built here once — the mask kernel gathers from it with the
    device timestep (no host read: a captured step replays with whatever timesteps its static input holds).  `at(timesteps)` binds one forward's [B] timesteps:
    the object the adapter-site helpers take as `tl`; the recompute passes and the backward of that forward use the same one, so every pass regenerates the
    same mask."""

    def __init__(self, R: int, Rmin: int, alpha: float, T: int, device):
        self.R, self.Rmin, self.alpha, self.T = int(R), int(Rmin), float(alpha), int(T)
        if not 1 <= self.Rmin <= self.R:
            raise ValueError(f"tlora_min_rank must lie in [1, linear_dim = {self.R}], got {self.Rmin}")
        if not self.alpha > 0.0:
            raise ValueError(f"tlora_alpha must be positive, got {self.alpha}")
        if self.T < 1:
            raise ValueError(f"num_train_timesteps must be positive, got {self.T}")
        self.ranks = [tlora_active_rank(t, self.T, self.R, self.Rmin, self.alpha) for t in range(self.T + 1)]
        self.table = torch.tensor(self.ranks, dtype=torch.int32).to(device)

    def at(self, timesteps):
        return SimpleNamespace(table=self.table, timesteps=timesteps)


class LoraGroup:
    """LoRA adapters of the projections that share one input (one fused GEMM).  peft semantics: y += (alpha/r) B A dropout(x): `streams` are the targets' mask
    stream ids (their index in the component's ordered target list — q / k / v share x but draw independent masks, as peft's per-module nn.Dropout); `down` /
    `grads` / `dx_add` take the component's LoraDropout state, None = no dropout (eval, p = 0): the unmasked routes."""

    def __init__(self, K: int, N_total: int, targets: List[Tuple[str, int, int]], rank: int, alpha: float, device, streams=None):
        self.K, self.N_total, self.targets = K, N_total, targets
        self.streams = list(range(len(targets))) if streams is None else list(streams)
        self.rank, self.scale = rank, alpha / rank
        # adapter columns inside the K-extension: 32 / 64 (one pass of the rank-space kernels), above 64 a multiple of 64 walked in 64-column slabs
        # (the reference's sd3.peft-lora example trains rank 128)
        self.r_pad = 32 if rank <= 32 else (rank + 63) // 64 * 64
        self.K2 = (len(targets) * self.r_pad + 63) // 64 * 64
        self.k2_real = len(targets) * rank          # adapter columns inside the padded extension (algorithmic-work accounting of the profiler)
        z = lambda *s: torch.zeros(*s, dtype=BF16, device=device)
        self.A_cat, self.A_cat_T = z(self.K2, K), z(K, self.K2)
        self.B_blk, self.B_blk_T = z(N_total, self.K2), z(self.K2, N_total)
        self.A: List[torch.Tensor] = []   # fp32 params (views into the flat arena), filled by the owner
        self.B: List[torch.Tensor] = []
        self.gA: List[torch.Tensor] = []  # fp32 grad views
        self.gB: List[torch.Tensor] = []
        self.flat_lo = self.flat_hi = 0   # this group's [lo, hi) element range inside the flat gradient arena
        self.dora: Optional[LoraDora] = None          # enable_dora(): the group's magnitudes and folded operands; None = plain LoRA (nothing allocated or launched)

    # ---- DoRA ----
    def enable_dora(self, lin, m, gm, flat_lo: int):
        """m / gm: the group's magnitudes and their gradients, [N_total] fp32 views of the arenas (the targets' vectors back to back, from element flat_lo)"""
        if self.K % 8 or len(self.targets) > 4 or self.r_pad > 128:
            raise NotImplementedError(f"use_dora: the adapters of {self.targets[0][0]} (in_features {self.K}, {len(self.targets)} targets, rank {self.rank}) are "
                                      "outside the fold kernel (in_features % 8 == 0, at most 4 targets per input, rank <= 128)")
        self.dora = LoraDora(self, lin, m, gm, flat_lo)

    def fold(self, init: bool = False):
        """after pack(): g = m / ||W + s B A||_row from the packed operands, then W' = g . W, B_blk' = g . B_blk and their transposes (ops.dora_fold).  The folded
        copies stay for the whole step: the forward, every recompute pass and the backward's dx / U products read them."""
        d = self.dora
        ops.dora_fold(d.lin.w, self.A_cat_T, self.B_blk, d.m, [(n_off, N) for (_, n_off, N) in self.targets], self.r_pad, d.inv_norm, d.g, d.Wf, d.WfT, d.Bf, d.BfT,
                      init=init)

    # the operands the GEMMs of an adapted Linear read: the folded ones under DoRA, else the Linear's own and the packed ones
    def w_of(self, lin):
        return lin.w if self.dora is None else self.dora.Wf

    def wT_of(self, lin):
        return lin.wT if self.dora is None else self.dora.WfT

    @property
    def B_fwd(self):
        return self.B_blk if self.dora is None else self.dora.Bf

    @property
    def B_fwd_T(self):
        return self.B_blk_T if self.dora is None else self.dora.BfT

    def _grads_dora(self, x, T, dy, accumulate: bool, sync):
        """dm = (1 / norm) sum_rows dy . y0 with y0 = x W^T + s (x A^T) B^T recomputed on the forward's GEMM route from the UNSCALED operands (no bias, no epilogue;
        nothing saved), and dB_g = g . (s dy_g^T T_g): the unscaled product into scratch by skinny_tn, then the row scale (gradient accumulation rules out scaling
        gB afterwards)"""
        d = self.dora
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("use_dora: an input that only exists as K segments is not built")
        M = x.shape[0] * x.shape[1] if x.dim() == 3 else x.shape[0]
        y0 = ops.dora_y0_scratch(T.device, M, self.N_total)
        ops.gemm(x, d.lin.w, a2=T, b2=self.B_blk, out=y0)
        ops.dora_dmag(dy, y0, d.inv_norm, d.gm, accumulate=accumulate)
        cw = min(self.r_pad, 64)
        for g, (_, n_off, N) in enumerate(self.targets):
            P = ops.dora_db_scratch(T.device, N, self.rank)
            for s0 in range(0, self.rank, cw):
                c0, r_used = g * self.r_pad + s0, min(cw, self.rank - s0)
                ops.skinny_tn(dy[..., n_off:n_off + N], T[:, c0:c0 + cw], P[:, s0:], self.rank, 1, r_used, alpha=self.scale, accumulate=False)
            ops.dora_db_finish(P, d.g[n_off:n_off + N], self.gB[g], accumulate=accumulate)
        if sync is not None:
            sync.ready(d.flat_lo, d.flat_hi)

    def pack(self):
        for g, (_, n_off, _) in enumerate(self.targets):
            ops.lora_pack(self.A[g], self.B[g], self.scale, self.A_cat, self.A_cat_T, self.B_blk, self.B_blk_T,
                          k2_off=g * self.r_pad, n_off=n_off)

    def down(self, x, drop=None, out=None, tl=None):
        """T = x A_cat^T [M, K2] bf16 — under dropout T_g = scale (keep_g . x) A_g^T for every target in one pass over x.  x: compact [M, K] or a [B, rows, K]
        view of a joint buffer (the mask follows the logical row b * rows + s either way).  tl: T-LoRA — the inactive rank columns of every sample are zeroed
        right behind the product."""
        if drop is None:
            T = ops.gemm(x, self.A_cat) if out is None else ops.gemm(x, self.A_cat, out=out)
            return T if tl is None else self.tlora_mask(T, tl)
        self._drop_check()
        return ops.lora_down_drop(x, self.A_cat, self.r_pad, self.streams, drop, out=out)

    def up(self, dy, out=None, tl=None):
        """U = dy B_blk [M, K2] bf16: the adapter term of the backward's dx and the left operand of dA (tl: T-LoRA's mask, as on T)"""
        U = ops.gemm(dy, self.B_fwd_T, out=out)
        return U if tl is None else self.tlora_mask(U, tl)

    def tlora_mask(self, t, tl):
        """T-LoRA: zeroes the rank columns >= r_b of sample b's rows of a rank-space operand [B * rows, K2] in place (ops.tlora_mask) — always launched, whatever
        the ranks are: nothing here depends on device data"""
        return ops.tlora_mask(t, self.r_pad, self.rank, len(self.targets), t.shape[0] // tl.timesteps.numel(), tl.table, tl.timesteps)

    def dx_add(self, dx, U, drop):
        """dx += scale sum_g keep_g . (U_g A_g): the adapter term of the projection's input gradient under dropout (the mask sits between U and A, so the term
        cannot ride the K-extension of the dx GEMM); in place, before anything consumes dx"""
        self._drop_check()
        return ops.lora_dx_drop(dx, U, self.A_cat_T, self.r_pad, self.streams, drop)

    def _drop_check(self):
        if self.K % 8 or len(self.targets) > 4 or self.r_pad > 128:
            raise NotImplementedError(f"lora_dropout: the adapters of {self.targets[0][0]} (in_features {self.K}, {len(self.targets)} targets, rank {self.rank}) are "
                                      "outside the masked kernels (in_features % 8 == 0, at most 4 targets per input, rank <= 128); set --lora_dropout=0")

    def grads(self, x, T, dy, U, accumulate: bool, sync=None, drop=None):
        """dB_g = s * dy_g^T T_g ; dA_g = U_g^T x   (rank-space backward: both products are [*, r]).  x: the projection's input, or — an input that only
        exists as K segments (the single block's proj_out reads [attn | mlp] as a two-segment K loop) — a list of (segment, first input column).
        drop: dA_g = scale U_g^T (keep_g . x) (T already carries the mask, dB is unchanged)."""
        if drop is not None:
            return self._grads_drop(x, T, dy, U, accumulate, sync, drop)
        segs = x if isinstance(x, (list, tuple)) else [(x, 0)]
        multi = len(segs) == 1 and 1 < len(self.targets) <= 4 and self.r_pad == 32 and U.shape[1] >= 128   # q / k / v share x: dA of all three in ONE pass over x
        cw = min(self.r_pad, 64)                                 # rank-space kernels take 32 or 64 adapter columns per pass
        dora = self.dora is not None          # DoRA: U = (g . dy) B_blk^T already carries the row scale, so dA is the product below as it is; dm and dB are not
        if dora:
            self._grads_dora(x, T, dy, accumulate, sync)
        for g, (_, n_off, N) in enumerate(self.targets):
            for s0 in range(0, self.rank, cw):
                c0, r_used = g * self.r_pad + s0, min(cw, self.rank - s0)
                if not dora:
                    ops.skinny_tn(dy[..., n_off:n_off + N], T[:, c0:c0 + cw], self.gB[g][:, s0:], self.rank, 1, r_used, alpha=self.scale, accumulate=accumulate)
                if not multi:
                    for (xs, k0) in segs:
                        ops.skinny_tn(xs, U[:, c0:c0 + cw], self.gA[g][s0:, k0:], 1, self.K, r_used, alpha=1.0, accumulate=accumulate)
        if multi:
            ops.skinny_tn_multi(x, U, self.gA, 1, self.K, self.rank, alpha=1.0, accumulate=accumulate)
        if sync is not None:
            sync.ready(self.flat_lo, self.flat_hi)

    def _grads_drop(self, x, T, dy, U, accumulate: bool, sync, drop):
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("lora_dropout: an input that only exists as K segments needs the logical column offset in the mask (not built)")
        self._drop_check()
        multi = 1 < len(self.targets) <= 4 and self.r_pad == 32 and U.shape[1] >= 128            # q / k / v share x: dA of all three in ONE pass over x
        cw = min(self.r_pad, 64)
        for g, (_, n_off, N) in enumerate(self.targets):
            for s0 in range(0, self.rank, cw):
                c0, r_used = g * self.r_pad + s0, min(cw, self.rank - s0)
                ops.skinny_tn(dy[..., n_off:n_off + N], T[:, c0:c0 + cw], self.gB[g][:, s0:], self.rank, 1, r_used, alpha=self.scale, accumulate=accumulate)
                if not multi:
                    ops.skinny_tn_drop(x, U[:, c0:c0 + cw], self.gA[g][s0:], 1, self.K, r_used, self.streams[g], drop, accumulate=accumulate)
        if multi:
            ops.skinny_tn_drop_multi(x, U, self.gA, 1, self.K, self.rank, self.streams, drop, accumulate=accumulate)
        if sync is not None:
            sync.ready(self.flat_lo, self.flat_hi)


def lokr_factorization(dim: int, factor: int = -1) -> Tuple[int, int]:
    """LyCORIS' factor rule: (m, n) with m <= n and m * n = dim.  A positive factor that divides dim gives (factor, dim // factor), sorted.  Otherwise (a negative
    factor means dim) m steps from 1 through the divisors of dim while m + n does not grow, m <= factor and m < n; the last accepted pair, sorted."""
    dim, factor = int(dim), int(factor)
    if factor > 0 and dim % factor == 0:
        return tuple(sorted((factor, dim // factor)))
    if factor < 0:
        factor = dim
    m, n = 1, dim
    while m < n:
        nm = m + 1
        while dim % nm:
            nm += 1
        nn_ = dim // nm
        if nm + nn_ > m + n or nm > factor:
            break
        m, n = nm, nn_
    return (m, n) if m <= n else (n, m)


@torch.no_grad()
def lokr_init_norm(W, w2, scale: float, generator=None):
    """the reference's `init_lokr_norm` start of one w2 (helpers/training/peft_init.py): a standard normal draw of w2's shape, rescaled first to the frozen weight's
    norm, then to its standard deviation, then shifted to its mean — in that order, the statistics taken on the fp32 image of the weight — and multiplied by `scale`"""
    z = torch.randn(w2.shape, dtype=w2.dtype, device=w2.device, generator=generator)
    Wd = W.to(F32)          # (the reference takes the weight through Tensor.dequantize(), which hands a bf16 weight back as fp32)
    norm, mean, std = (f().to(w2.dtype) for f in (Wd.norm, Wd.mean, Wd.std))
    z = z * (norm / z.norm())
    z = z * (std / z.std())
    z = z - z.mean() + mean
    w2.copy_(z * scale)


class LokrGroup:
    """LyCORIS LoKr adapters (`algo: lokr`, both factors full) of the projections that share one input (one fused GEMM), beside LoraGroup and answering the same
    adapter-site calls.  Target g owns rows [n_off, n_off + N) of the fused W [N_total, K]: dW_g = s kron(w1_g, w2_g) with w1 [ol, im], w2 [ok, in],
    (ol, ok) = lokr_factorization(N, factor), (im, in) = lokr_factorization(K, factor).  The forward is the merged-weight one: `fold(mult)` — once per engine
    forward, never in a recompute pass — writes Wf = bf16(W + dW), its transpose and the bf16 copy of every w2; `w_of` / `wT_of` hand the folded copies to every
    GEMM of the forward, of the recompute passes and of the backward's dx.  There is no rank-space side path: `down` / `up` return nothing, so the K-extension
    keyword helpers stay empty.  The folded copies double the adapted weights' memory; they live for the whole step."""

    K2 = 0          # no K-extension
    dora = None
    scale = 1.0     # (the adapter scale a LoraGroup carries in alpha / r lives in `s`, set by every fold)

    def __init__(self, lin, targets: List[Tuple[str, int, int]], factors: List[int], device):
        N_total, K = lin.w.shape
        self.lin, self.K, self.N_total, self.targets = lin, K, N_total, targets
        self.shapes = []                        # per target (ol, ok, im, in)
        for (name, n_off, N), f in zip(targets, factors):
            (ol, ok), (im, in_) = lokr_factorization(N, f), lokr_factorization(K, f)
            self.shapes.append((ol, ok, im, in_))
        self.check(targets, self.shapes, factors)
        e = lambda *s: torch.empty(*s, dtype=BF16, device=device)
        self.Wf, self.WfT = e(N_total, K), e(K, N_total)
        self.w2b = [e(ok, in_) for (_, ok, _, in_) in self.shapes]
        self.w1: List[torch.Tensor] = []        # fp32 params (views into the flat arena), filled by the owner
        self.w2: List[torch.Tensor] = []
        self.g1: List[torch.Tensor] = []        # fp32 grad views
        self.g2: List[torch.Tensor] = []
        self.flat_lo = self.flat_hi = 0
        self.s = 1.0                            # the scale of the last fold: what the backward's gradients carry

    @staticmethod
    def check(targets, shapes, factors):
        """the shapes the kernels and the P GEMM route take, refused by name with the factor to choose"""
        if len(targets) > 4:
            raise NotImplementedError(f"lycoris lokr: {len(targets)} targets on one input ({targets[0][0]}); the fold kernel takes at most 4")
        for (name, _, N), (ol, ok, im, in_), f in zip(targets, shapes, factors):
            if ol > 16 or im > 16:
                raise NotImplementedError(f"lycoris lokr: factor={f} gives {name} a w1 of [{ol}, {im}]; the kernels take w1 sides up to 16 — set factor to a divisor "
                                          f"of {N} and {in_ * im} that is at most 16")
            if ok % 8 or in_ % 64:
                raise NotImplementedError(f"lycoris lokr: factor={f} splits {name} [{N}, {im * in_}] into w2 [{ok}, {in_}]; the gradient route needs ok % 8 == 0 and "
                                          f"in % 64 == 0 — choose a factor for which in_features / factor is a multiple of 64 (e.g. factor=8 or factor=4)")

    def fold(self, mult: float = 1.0):
        self.s = float(mult)
        ops.lokr_fold(self.lin.w, [(n_off, N, w1, w2, w2b) for (_, n_off, N), w1, w2, w2b in zip(self.targets, self.w1, self.w2, self.w2b)], self.s, self.Wf, self.WfT)

    def pack(self):
        pass

    def w_of(self, lin):
        return self.Wf

    def wT_of(self, lin):
        return self.WfT

    def down(self, x, drop=None, out=None, tl=None):
        return None

    def up(self, dy, out=None, tl=None):
        return None

    def grads(self, x, T, dy, U, accumulate: bool, sync=None, drop=None):
        """per target: dP = mix(dy), dw2 = s dP^T x, P = x.view(M im, in) w2^T on the GEMM route into scratch, dw1 = s sum dy . P — no [N, K] gradient is formed.
        x: the projection's input, compact [M, K] or a [B, rows, K] view of a joint buffer; dy likewise over the fused projection's N_total columns."""
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("lycoris lokr: an input that only exists as K segments is not built")
        if x.dim() == 2 and not x.is_contiguous():
            x = x.contiguous()
        M = x.shape[0] * x.shape[1] if x.dim() == 3 else x.shape[0]
        dev = x.device
        for g, ((_, n_off, N), (ol, ok, im, in_)) in enumerate(zip(self.targets, self.shapes)):
            dP = ops.lokr_scratch("dp", dev, M, im * ok)
            ops.lokr_mix(dy, n_off, self.w1[g], ok, dP)
            ops.lokr_dw2(dP, x, im, self.g2[g], alpha=self.s, accumulate=accumulate)
            P = ops.lokr_scratch("p", dev, M, im * ok)
            xv = x.view(M * im, in_) if x.dim() == 2 else x.unflatten(-1, (im, in_)).flatten(1, 2)
            ops.gemm(xv, self.w2b[g], out=P.view(M * im, ok))
            ops.lokr_dw1(dy, n_off, P, self.g1[g], ok, alpha=self.s, accumulate=accumulate)
        if sync is not None:
            sync.ready(self.flat_lo, self.flat_hi)


# ------------------------------------------------------------------------------------------------
# one adapter site = a Linear (`lin.w`, `lin.wT`, `lin.lora`: its LoraGroup or None), phase by phase: the callers issue every site's down / up GEMM, then the
# (grouped) base GEMM with the kwargs below, then the `lora_dx_finish`es, then the `lora_grads`.  Without an adapter (or with `lin` None) each does nothing.
# ------------------------------------------------------------------------------------------------
def lin_w(lin):
    """the weight operand of an adapted Linear's forward GEMM: its own, or under DoRA the group's folded copy g . W"""
    return lin.w if lin.lora is None else lin.lora.w_of(lin)


def lin_wT(lin):
    """likewise the K-major operand of its dgrad GEMM"""
    return lin.wT if lin.lora is None else lin.lora.wT_of(lin)


def lora_down(lin, x, drop=None, out=None, tl=None):          # forward: T = x A_cat^T (LoraGroup.down; tl: T-LoRA's rank mask on it)
    return None if lin is None or lin.lora is None else lin.lora.down(x, drop, out=out, tl=tl)


def lora_fwd_kw(lin, T) -> dict:                     # forward: the K-extension of the base GEMM, y += T B^T
    return {} if T is None else dict(a2=T, b2=lin.lora.B_fwd)


def lora_up(lin, dy, out=None, tl=None):             # backward: U = dy B [M, K2] (tl: T-LoRA's rank mask on it)
    return None if lin is None or lin.lora is None else lin.lora.up(dy, out, tl=tl)


def lora_dx_kw(lin, U, drop) -> dict:                # backward: the K-extension of the dx GEMM, dx += U A — not under dropout: the mask sits between U and A
    return dict(a2=U, b2=lin.lora.A_cat_T) if (U is not None and drop is None) else {}


def lora_dx_finish(lin, dx, U, drop):                # backward, under dropout: that term, masked, added in place before anything consumes dx (LoraGroup.dx_add)
    if U is not None and drop is not None:
        lin.lora.dx_add(dx, U, drop)


def lora_grads(lin, x, T, dy, U, accumulate: bool, sync=None, drop=None):          # backward: the adapter's own gradients (LoraGroup.grads)
    if lin is not None and lin.lora is not None:
        lin.lora.grads(x, T, dy, U, accumulate, sync, drop)


# ------------------------------------------------------------------------------------------------
# a stream's rows of a joint [B * S, C] buffer as GEMM operands
# ------------------------------------------------------------------------------------------------
def rows_of(joint, lo: int, rows: int, B: int, S: int):
    """rows [lo, lo + rows) of every sample of a joint [B * S, C] buffer, as a GEMM / skinny operand: a [B, rows, C] strided view (no copy)"""
    return joint.view(B, S, -1)[:, lo:lo + rows]


def problems(B: int, rows: int, pr: dict):
    """One projection over the `rows`-row block of every sample.  Operands may be compact [B * rows, C] tensors or [B, rows, C] views of joint
    buffers (rows_of).  When the blocks are tile-aligned (rows % 256 == 0) that is ONE segmented problem (st355_gemm_args.seg_rows: one grid of
    B * rows / 256 row tiles instead of B launches that each fill the 256 CUs badly); otherwise one problem per sample."""
    ROWED = ("a", "a2", "out", "aux_in", "aux_out")
    if B == 1:
        return [{k: (v[0] if k in ROWED and torch.is_tensor(v) and v.dim() == 3 else v) for k, v in pr.items()}]
    if rows % 256 == 0:
        return [pr]
    out = []
    for b in range(B):
        q = {}
        for k, v in pr.items():
            if k in ROWED and torch.is_tensor(v):
                q[k] = v[b] if v.dim() == 3 else v[b * rows:(b + 1) * rows]
            elif k == "gate":          # one gate row per sample, or — tokenwise timesteps — one per token row of this stream
                q[k] = v[b:b + 1] if v.shape[0] == B else v[b * rows:(b + 1) * rows]
            else:
                q[k] = v
        out.append(q)
    return out


def compact(t, B: int, rows: int):
    """a [B, rows, C] view as an operand of the rank-space gradient kernels: as is when they can walk it segmented, else a compact copy"""
    if t.dim() != 3:
        return t
    if B == 1:
        return t[0]
    return t if rows % 256 == 0 else t.reshape(B * rows, -1)


# ------------------------------------------------------------------------------------------------
# LayerSync (helpers/training/layersync.py): the regulariser's forward taps and its gradient's way into the hand-written dX chain
# ------------------------------------------------------------------------------------------------
def layersync_indices(student_idx, teacher_idx, n_blocks: int):
    """validated 0-based (student, teacher) block indices of `set_layersync`; the teacher defaults to the student (the reference's default when
    `layersync_teacher_block` is unset: similarity 1, gradient 0 up to rounding)"""
    s = int(student_idx)
    t = s if teacher_idx is None else int(teacher_idx)
    for role, i in (("student", s), ("teacher", t)):
        if not 0 <= i < n_blocks:
            raise ValueError(f"set_layersync: {role} block {i} is out of range (this model has {n_blocks} blocks)")
    if t < s:
        raise ValueError(f"set_layersync: the teacher block ({t}) must not lie below the student block ({s})")
    return s, t


class LayerSyncTap:
    """One per training forward (kept in its ctx).  `tap(g, view)` after block g of the saving forward — never in the recompute pass of a checkpointed segment —
    copies the student block's image-token rows [B, rows, D] into ONE compact bf16 buffer and, at the teacher block, turns that buffer in place into
    G = d sim / d student (ops.layersync_fwd; the teacher is read as the view it is).  `inject(view, dsim)` right before the student block's own backward adds
    dsim * G to the gradient with respect to that block's output; dsim stays on the device (it carries -lambda, the accumulation division and any loss scale)."""

    key = "layersync_similarity"

    def __init__(self, student: int, teacher: int):
        self.student, self.teacher = student, teacher
        self.block = student                  # where the backward hooks in
        self.G = self.cos = self.sim = self.output = None

    def tap(self, g: int, view):
        if g == self.student:
            B, rows, D = view.shape
            self.G = torch.empty(B * rows, D, dtype=BF16, device=view.device)
            self.cos = torch.empty(B * rows, dtype=F32, device=view.device)
            self.sim = torch.empty((), dtype=F32, device=view.device)
            self.G.view(B, rows, D).copy_(view)
        if g == self.teacher:
            B, rows, D = view.shape
            ops.layersync_fwd(self.G.view(B, rows, D), view, self.G, self.cos, self.sim)

    def finish(self, H: int, W: int):
        self.output = self.sim
        return self.output

    def inject(self, view, dsim):
        ops.layersync_inject(view, self.G, dsim.detach().to(F32))
        self.G = None

    def backward(self, dsim, dx_view, accumulate: bool = False, sync=None):
        self.inject(dx_view, dsim)            # nothing trains here: no gradients of its own to accumulate or hand to `sync`


# ------------------------------------------------------------------------------------------------
# Internal Guidance (helpers/training/internal_guidance.py): an auxiliary head LayerNorm(D, eps 1e-6) -> Linear(D -> 64) on one block's image-token output
# ------------------------------------------------------------------------------------------------
IG_NAMES = ("norm.weight", "norm.bias", "proj.weight", "proj.bias")          # under `internal_guidance_head.`: the reference module's parameter names


def internal_guidance_index(block_index, n_blocks: int) -> int:
    """validated 0-based block index (internal_guidance.py:194-197: used as it is, no LayerSync-style idx - 1 rule)"""
    i = int(block_index)
    if not 0 <= i < n_blocks:
        raise ValueError(f"internal_guidance_block_index must be within [0, {n_blocks - 1}], got {i}.")
    return i


def internal_guidance_shapes(D: int):
    return ((D,), (D,), (ops.IG_N, D), (ops.IG_N,))


class InternalGuidanceHead:
    """The head's four trainable tensors as views of the arena that trains (fp32 at the tail of the adapter arena, or bf16 inside the base parameter arena), their
    gradient views, the [lo, hi) element range of the gradient arena they span, and the folded bf16 operands the kernels read (ops.ig_fold, once per forward)."""

    def __init__(self, block: int, D: int, params, grads, flat_lo: int, flat_hi: int, device):
        self.block, self.D = block, D
        self.gamma, self.beta, self.W, self.b = params
        self.g_gamma, self.g_beta, self.g_W, self.g_b = grads          # re-pointed by the owner when it switches gradient arenas
        self.flat_lo, self.flat_hi = flat_lo, flat_hi
        self.Wf = torch.empty(ops.IG_N, D, dtype=BF16, device=device)
        self.WfT = torch.empty(D, ops.IG_N, dtype=BF16, device=device)
        self.c = torch.empty(ops.IG_N, dtype=BF16, device=device)

    @property
    def grads(self):
        return (self.g_gamma, self.g_beta, self.g_W, self.g_b)

    @torch.no_grad()
    def init_reference(self):
        """internal_guidance.py:93-97: LayerNorm affine (1, 0), zero projection"""
        self.gamma.fill_(1.0); self.beta.zero_(); self.W.zero_(); self.b.zero_()

    def fold(self):
        ops.ig_fold(self.gamma, self.beta, self.W, self.b, self.Wf, self.WfT, self.c)


class InternalGuidanceTap:
    """One per forward that wants the head's prediction (kept in the training forward's ctx).  `tap(g, view)` after block g of the saving forward — never in the
    recompute pass of a checkpointed segment — folds the current parameters and runs the head on the block's image-token rows [B, rows, D] (read as the view they
    are): xhat / rstd stay for the backward, y holds the tokens.  `prediction(H, W)`: the [B, 16, H, W] bf16 latent-shaped prediction.  `backward(d_pred, dx_view)`
    right before block g's own backward fills the head's four gradient views and adds d loss / d h into the gradient with respect to that block's output
    (dx_view None: the block lies below the first one that trains, only the head's gradients are wanted), then hands the head's range to `sync`."""

    key = "internal_guidance_prediction"

    def __init__(self, head: InternalGuidanceHead, channels: int = 16):
        self.head, self.block, self.channels = head, head.block, channels
        self.xhat = self.rstd = self.y = self.output = None
        self.B = self.rows = 0

    def tap(self, g: int, view):
        if g != self.block:
            return
        B, rows, D = view.shape
        dev = view.device
        self.B, self.rows = B, rows
        self.xhat = torch.empty(B * rows, D, dtype=BF16, device=dev)
        self.rstd = torch.empty(B * rows, dtype=F32, device=dev)
        self.y = torch.empty(B * rows, ops.IG_N, dtype=BF16, device=dev)
        self.head.fold()
        ops.ig_head_fwd(view, self.head.Wf, self.head.c, self.xhat, self.rstd, self.y)

    def prediction(self, H: int, W: int):
        if self.y is None:
            raise RuntimeError(f"Internal Guidance: block {self.block} was never reached by the forward")
        if (H // 2) * (W // 2) != self.rows:
            raise ValueError("Internal Guidance hidden-state token count does not match the diffusion target: "
                             f"tokens={self.rows}, patch_volume=4, spatial_shape=({H}, {W}).")
        return ops.unpatchify(self.y.view(self.B, self.rows, ops.IG_N), self.channels, H, W, order=1)

    def finish(self, H: int, W: int):
        self.output = self.prediction(H, W)
        return self.output

    def backward(self, d_pred, dx_view, accumulate: bool = False, sync=None):
        h = self.head
        if d_pred is None:                       # the prediction took no part in the loss
            if not accumulate:
                for g in h.grads:
                    g.zero_()
        else:
            dy = ops.patchify(d_pred.to(BF16).contiguous(), order=1).view(self.B * self.rows, ops.IG_N)
            ops.ig_wgrad(self.xhat, dy, h.gamma, h.beta, h.W, *h.grads, accumulate=accumulate)
            if dx_view is not None:
                ops.ig_head_bwd(self.xhat, self.rstd, dy, h.WfT, dx_view)
        if sync is not None:
            sync.ready(h.flat_lo, h.flat_hi)
        self.xhat = self.rstd = None


# ------------------------------------------------------------------------------------------------
# operands of the TN weight-gradient GEMM (contraction granule: 64 rows)
# ------------------------------------------------------------------------------------------------
def pad64_empty(rows: int, cols: int, dev):
    """[rows, cols] bf16, uninitialised, as the head of a parent buffer whose row count is rounded up to 64 and whose tail rows are ZERO: the weight-gradient GEMM
    reads the parent directly instead of a zero-padded copy of the tensor (two launches and a full copy per operand).  The view remembers its parent in
    `_st355_pad64`."""
    rp = (rows + 63) // 64 * 64
    if rp == rows:
        return torch.empty(rows, cols, dtype=BF16, device=dev)
    par = torch.empty(rp, cols, dtype=BF16, device=dev)
    par[rows:].zero_()
    t = par[:rows]
    t._st355_pad64 = par
    return t


def pad64(t):
    """the operand with a multiple of 64 contraction rows: as is when aligned or segmented (3-D), its zero-tailed parent when it was allocated by
    pad64_empty, else a zero-padded copy"""
    if t.dim() == 3:
        return t
    r = t.shape[0]
    if r % 64 == 0 and t.is_contiguous():
        return t
    par = getattr(t, "_st355_pad64", None)
    if par is not None:
        return par
    o = torch.zeros((r + 63) // 64 * 64, t.shape[1], dtype=BF16, device=t.device)
    o[:r] = t
    return o


# ------------------------------------------------------------------------------------------------
# NextLat (helpers/training/nextlat.py): a predictor LayerNorm(D, eps 1e-6) -> Linear(D -> 2D) -> GELU(erf) -> Linear(2D -> D) of token t + 1 from token t of one
# block's image-token output
# ------------------------------------------------------------------------------------------------
NEXTLAT_NAMES = ("norm.weight", "norm.bias", "up.weight", "up.bias", "down.weight", "down.bias")          # under `nextlat_predictor.`: the reference module's names


def nextlat_index(configured, n_blocks: int) -> int:
    """nextlat.py:103-106 as it is: `int(configured or -1)`, negative = the last block — so None, 0 and -1 all name the last block, and block 0 cannot be chosen"""
    c = int(configured or -1)
    i = n_blocks - 1 if c < 0 else c
    if not 0 <= i < n_blocks:
        raise ValueError(f"nextlat_block_index must be within [-1, {n_blocks - 1}], got {c}.")
    return i


def nextlat_shapes(D: int):
    return ((D,), (D,), (2 * D, D), (2 * D,), (D, 2 * D), (D,))


@torch.no_grad()
def nextlat_init_reference(params, D: int, generator=None):
    """nextlat.py:78-83 on the six tensors (NEXTLAT_NAMES order, any dtype): LayerNorm affine (1, 0), `up` as nn.Linear's default (kaiming_uniform(a = sqrt 5) =
    U(-1 / sqrt D, 1 / sqrt D) for weight and bias), `down` zero.  The one initialiser of every lay-out (adapter arena, base arena)."""
    gamma, beta, W_up, b_up, W_down, b_down = params
    bound = 1.0 / math.sqrt(D)
    gamma.fill_(1.0); beta.zero_()
    W_up.uniform_(-bound, bound, generator=generator); b_up.uniform_(-bound, bound, generator=generator)
    W_down.zero_(); b_down.zero_()


class NextLatHead:
    """The predictor's six trainable tensors as views of the arena that trains (fp32 at the tail of the adapter arena, or bf16 inside the base parameter arena), their
    gradient views, the [lo, hi) element range of the gradient arena they span, and the folded bf16 operands the GEMMs read (ops.nextlat_fold, once per forward)."""

    def __init__(self, block: int, D: int, params, grads, flat_lo: int, flat_hi: int, device):
        self.block, self.D = block, D
        self.gamma, self.beta, self.W_up, self.b_up, self.W_down, self.b_down = params
        self.g_gamma, self.g_beta, self.g_W_up, self.g_b_up, self.g_W_down, self.g_b_down = grads          # re-pointed by the owner when it switches gradient arenas
        self.flat_lo, self.flat_hi = flat_lo, flat_hi
        e = lambda *shp: torch.empty(*shp, dtype=BF16, device=device)
        self.W1f, self.W1fT, self.c1 = e(2 * D, D), e(D, 2 * D), e(2 * D)
        self.Wd, self.WdT, self.bd = e(D, 2 * D), e(2 * D, D), e(D)

    @property
    def params(self):
        return (self.gamma, self.beta, self.W_up, self.b_up, self.W_down, self.b_down)

    @property
    def grads(self):
        return (self.g_gamma, self.g_beta, self.g_W_up, self.g_b_up, self.g_W_down, self.g_b_down)

    def init_reference(self, generator=None):
        nextlat_init_reference(self.params, self.D, generator)

    def fold(self):
        ops.nextlat_fold(*self.params, self.W1f, self.W1fT, self.c1, self.Wd, self.WdT, self.bd)


class NextLatTap:
    """One per training forward (kept in its ctx).  `tap(g, view)` after block g of the saving forward — never in the recompute pass of a checkpointed segment — folds
    the current parameters and runs the predictor on rows 0 .. S-2 of the block's image-token rows [B, S, D] against rows 1 .. S-1 (both read as the views they are):
    `state_loss` (one fp32 on the device) is the mean smooth-L1 / MSE; xhat, rstd, U, A and psi = d loss / d pred (unscaled) stay for the backward.
    `backward(d_state, dx_view)` right before block g's own backward fills the six gradient views and adds d loss / d h into rows 0 .. S-2 of the gradient with
    respect to that block's output (dx_view None: the block lies below the first one that trains, only the predictor's gradients are wanted), then hands the
    predictor's range to `sync`.  The target rows are detached (nextlat.py:146): nothing flows into them."""

    key = "nextlat_state_loss"

    def __init__(self, head: NextLatHead, mode: str = "smooth_l1"):
        self.head, self.block, self.mode = head, head.block, mode
        self.xhat = self.rstd = self.U = self.A = self.psi = self.state_loss = self.output = None
        self.B = self.rows = 0

    def tap(self, g: int, view):
        if g != self.block:
            return
        B, S, D = view.shape
        if S < 2:
            raise ValueError("NextLat requires at least two hidden tokens to predict the next latent state.")          # nextlat.py:141-142
        h, dev = self.head, view.device
        rows = S - 1
        M = B * rows
        self.B, self.rows = B, rows
        self.xhat, self.rstd = pad64_empty(M, D, dev), torch.empty(M, dtype=F32, device=dev)
        self.U, self.A, self.psi = torch.empty(M, 2 * D, dtype=BF16, device=dev), pad64_empty(M, 2 * D, dev), pad64_empty(M, D, dev)
        self.state_loss = torch.empty(1, dtype=F32, device=dev)
        h.fold()
        ops.nextlat_rows(view[:, :rows], self.xhat, self.rstd)
        ops.gemm(self.xhat, h.W1f, bias=h.c1, out=self.U)
        ops.gelu_erf(self.U, self.A)
        ops.gemm(self.A, h.Wd, bias=h.bd, out=self.psi)                  # the prediction, overwritten with psi by the loss
        ops.nextlat_loss(self.psi, view[:, 1:], self.mode, self.state_loss)

    def state(self):
        if self.state_loss is None:
            raise RuntimeError(f"NextLat: block {self.block} was never reached by the forward")
        return self.state_loss.view(())

    def finish(self, H: int, W: int):
        self.output = self.state()
        return self.output

    def backward(self, d_state, dx_view, accumulate: bool = False, sync=None):
        h = self.head
        if d_state is None:                      # the state loss took no part in the loss
            if not accumulate:
                for g in h.grads:
                    g.zero_()
        else:
            M, D, dev = self.B * self.rows, h.D, self.psi.device
            # the chain is linear in psi: ONE device scalar carries the upstream gradient (nextlat_weight, the accumulation division) and the mean's 1 / (M D)
            s = (d_state.detach().to(device=dev, dtype=F32).reshape(1) * (1.0 / (M * D))).contiguous()
            dU = pad64_empty(M, 2 * D, dev)
            ops.gemm(self.psi, h.WdT, out=dU)                             # dA = psi W_down
            ops.gelu_erf_bwd(self.U, dU, dU)
            db = torch.empty(3 * D, dtype=F32, device=dev)
            db2, db1 = db[:D].view(1, D), db[D:].view(1, 2 * D)
            ops.colsum_prod(self.psi, db2)
            ops.nextlat_wgrad_down(ops.gemm_tn(pad64(self.psi), pad64(self.A)), db2.view(D), s, h.g_W_down, h.g_b_down, accumulate=accumulate)
            ops.colsum_prod(dU, db1)
            ops.nextlat_wgrad_up(ops.gemm_tn(pad64(dU), pad64(self.xhat)), db1.view(2 * D), h.gamma, h.beta, h.W_up, s, h.g_gamma, h.g_beta, h.g_W_up, h.g_b_up,
                                 accumulate=accumulate)
            if dx_view is not None:
                g = torch.empty(M, D, dtype=BF16, device=dev)
                ops.gemm(dU, h.W1fT, out=g)                               # g = dU W1f
                ops.nextlat_ln_bwd_add(g, self.xhat, self.rstd, s, dx_view[:, :self.rows])
        if sync is not None:
            sync.ready(h.flat_lo, h.flat_hi)
        self.xhat = self.rstd = self.U = self.A = self.psi = None


# ------------------------------------------------------------------------------------------------
# Self-Flow (helpers/training/crepa.py with crepa_feature_source=self_flow): a projector LayerNorm(D, eps 1e-5) -> Linear(D -> D) of one student block's image-token
# output, aligned by cosine to a deeper block of the EMA teacher's forward on the cleaner view
# ------------------------------------------------------------------------------------------------
SELF_FLOW_NAMES = ("0.weight", "0.bias", "1.weight", "1.bias")          # under `crepa_projector.`: the reference's nn.Sequential(LayerNorm, Linear)


def self_flow_indices(student_block, teacher_block, n_blocks: int):
    """validated 0-based (student, teacher) block indices, used as they are (`layer_{i}` of the hidden-state buffer); the two forwards are separate, so neither
    bounds the other"""
    if student_block is None:
        raise ValueError("crepa_block_index must be set when CREPA is enabled.")                                    # crepa.py `attach_to_model`
    if teacher_block is None:
        raise ValueError("CREPA self_flow mode requires crepa_teacher_block_index to be set.")                      # common.py `_validate_crepa_configuration`
    s, t = int(student_block), int(teacher_block)
    for key, i in (("crepa_block_index", s), ("crepa_teacher_block_index", t)):
        if not 0 <= i < n_blocks:
            raise ValueError(f"{key} must be within [0, {n_blocks - 1}], got {i}.")
    return s, t


def self_flow_shapes(D: int):
    return ((D,), (D,), (D, D), (D,))


class SelfFlowHead:
    """The projector's four trainable tensors as fp32 views at the tail of the adapter arena, their gradient views, the [lo, hi) element range of the gradient arena
    they span, and the folded bf16 operands the GEMMs read (ops.self_flow_fold, once per training forward)."""

    def __init__(self, block: int, teacher_block: int, D: int, params, grads, flat_lo: int, flat_hi: int, device):
        self.block, self.teacher_block, self.D = block, teacher_block, D
        self.gamma, self.beta, self.W, self.b = params
        self.g_gamma, self.g_beta, self.g_W, self.g_b = grads
        self.flat_lo, self.flat_hi = flat_lo, flat_hi
        e = lambda *shp: torch.empty(*shp, dtype=BF16, device=device)
        self.Wf, self.WfT, self.c = e(D, D), e(D, D), e(D)

    @property
    def params(self):
        return (self.gamma, self.beta, self.W, self.b)

    @property
    def grads(self):
        return (self.g_gamma, self.g_beta, self.g_W, self.g_b)

    @torch.no_grad()
    def init_reference(self, generator=None):
        """crepa.py `attach_to_model`: nn.LayerNorm's (1, 0) and nn.Linear's default — kaiming_uniform(a = sqrt 5) = U(-1 / sqrt D, 1 / sqrt D) for the weight, the same
        bound for the bias — drawn in fp32, weight first, from the generator given: the adapters' own (seeded by add_lora_adapter's `seed`), behind every A / B draw"""
        bound = 1.0 / math.sqrt(self.D)
        self.gamma.fill_(1.0); self.beta.zero_()
        self.W.uniform_(-bound, bound, generator=generator); self.b.uniform_(-bound, bound, generator=generator)

    def fold(self):
        ops.self_flow_fold(self.gamma, self.beta, self.W, self.b, self.Wf, self.WfT, self.c)


class CaptureTap:
    """The teacher forward's tap (no-grad, works with save=False): `tap(g, view)` at block `block` leaves a compact bf16 copy of its image-token rows [B, rows, D] in
    `output`.  `stop`: the forward may end behind that block — nothing else of it is read."""

    key = "crepa_hidden_states"
    stop = True

    def __init__(self, block: int):
        self.block, self.output = block, None

    def tap(self, g: int, view):
        if g == self.block:
            self.output = torch.empty(view.shape, dtype=BF16, device=view.device)
            self.output.copy_(view)

    def finish(self, H: int, W: int):
        if self.output is None:
            raise ValueError(f"CREPA self_flow mode requested teacher layer {self.block} but the teacher forward did not return hidden states.")      # common.py:5359-5362
        return self.output

    def backward(self, d, dx_view, accumulate: bool = False, sync=None):
        raise RuntimeError("CaptureTap: the teacher forward has no backward")


class SelfFlowTap:
    """One per training forward (kept in its ctx).  `tap(g, view)` after the student block of the saving forward — never in the recompute pass of a checkpointed
    segment — folds the current parameters and runs xhat / rstd (ops.self_flow_rows), proj = xhat Wf^T + c (ops.gemm) and the cosine against the teacher features
    handed in (ops.layersync_fwd: `sim` = the mean over all B * rows tokens — the reference's mean of per-sample means, every sample having the same token count —
    and G = d sim / d proj written over proj).  `backward(dsim, dx_view)` right before that block's own backward: P = G^T xhat, db = colsum(G), the four gradient
    views (ops.self_flow_wgrad; dsim, ONE device scalar, carries -weight and the accumulation division), g = G Wf added through the LayerNorm backward into the
    gradient with respect to the block's output (ops.nextlat_ln_bwd_add), then the projector's range goes to `sync`.  `cutoff`: the scheduler's weight is 0 — the
    similarity took no part in the loss: nothing is launched, the gradient views are zeroed."""

    key = "crepa_similarity"

    def __init__(self, head: SelfFlowHead, teacher):
        self.head, self.block, self.teacher = head, head.block, teacher
        self.xhat = self.rstd = self.G = self.cos = self.sim = self.output = None
        self.B = self.rows = 0
        self.cutoff = False

    def tap(self, g: int, view):
        if g != self.block:
            return
        B, rows, D = view.shape
        h, dev, t = self.head, view.device, self.teacher
        if t is None:
            raise ValueError("CREPA self_flow feature mode requires teacher features from the model.")              # crepa.py `compute_loss`
        if t.dim() != 3 or tuple(t.shape) != (B, rows, D):
            raise ValueError(f"CREPA self_flow: teacher features {tuple(t.shape)} do not match the student block's image tokens {(B, rows, D)}")
        M = B * rows
        self.B, self.rows = B, rows
        self.xhat, self.rstd = pad64_empty(M, D, dev), torch.empty(M, dtype=F32, device=dev)
        self.G = pad64_empty(M, D, dev)
        self.cos, self.sim = torch.empty(M, dtype=F32, device=dev), torch.empty((), dtype=F32, device=dev)
        h.fold()
        ops.self_flow_rows(view, self.xhat, self.rstd)
        ops.gemm(self.xhat, h.Wf, bias=h.c, out=self.G)                   # the projection, overwritten with G by the cosine pass
        ops.layersync_fwd(self.G.view(B, rows, D), t.detach(), self.G, self.cos, self.sim)
        self.teacher = None

    def finish(self, H: int, W: int):
        if self.sim is None:
            raise RuntimeError(f"Self-Flow: block {self.block} was never reached by the forward")
        self.output = self.sim
        return self.output

    def backward(self, dsim, dx_view, accumulate: bool = False, sync=None):
        h = self.head
        if dsim is None or self.cutoff:          # the similarity took no part in the loss
            if not accumulate:
                for g in h.grads:
                    g.zero_()
        else:
            M, D, dev = self.B * self.rows, h.D, self.G.device
            s = dsim.detach().to(device=dev, dtype=F32).reshape(1).contiguous()
            db = torch.empty(1, D, dtype=F32, device=dev)
            ops.colsum_prod(self.G, db)
            ops.self_flow_wgrad(ops.gemm_tn(pad64(self.G), pad64(self.xhat)), db.view(D), h.gamma, h.beta, h.W, s, *h.grads, accumulate=accumulate)
            if dx_view is not None:
                g = torch.empty(M, D, dtype=BF16, device=dev)
                ops.gemm(self.G, h.WfT, out=g)                            # g = G Wf
                ops.nextlat_ln_bwd_add(g, self.xhat, self.rstd, s, dx_view)
        if sync is not None:
            sync.ready(h.flat_lo, h.flat_hi)
        self.xhat = self.rstd = self.G = None


# ------------------------------------------------------------------------------------------------
# Self-Transcendence (helpers/distillation/self_transcendence/distiller.py): a projector Linear(D -> Hp) -> SiLU -> Linear(Hp -> Hp) -> SiLU -> Linear(Hp -> D) of one
# shallow block's image-token output, trained by a masked per-sample MSE to the patchified diffusion target (stage `vae`) or to the frozen teacher's feature-space
# CFG target (stage `self`)
# ------------------------------------------------------------------------------------------------
ST_NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")      # under `self_transcendence_projector.`: the reference module's names


def self_transcendence_indices(student_block, teacher_block, n_blocks: int):
    """0-based (student, teacher or None) block indices, used as they are (`layer_{i}` of the hidden-state buffer); the reference finds no `layer_{i}` past the last
    block at the first step — here that is refused when the blocks are named"""
    s = int(student_block)
    t = None if teacher_block is None else int(teacher_block)
    for key, i in (("student_block", s), ("teacher_block", t)):
        if i is not None and not 0 <= i < n_blocks:
            raise ValueError(f"Self-Transcendence {key} must be within [0, {n_blocks - 1}], got {i}.")
    return s, t


def self_transcendence_shapes(D: int, Hp: int):
    return ((Hp, D), (Hp,), (Hp, Hp), (Hp,), (D, Hp), (D,))


def self_transcendence_grid(source_shape, token_count: int):
    """distiller.py `_factor_grid` for a 2-D latent: the shape itself when it holds exactly the tokens (patch 1), else the divisor pair (gh, gw) with gh | H, gw | W
    and gh gw == token_count whose aspect ratio is closest to H / W (the first such pair on a tie)"""
    H, W = (int(v) for v in source_shape)
    token_count = int(token_count)
    if H * W == token_count:
        return (H, W)
    cands = [(f, token_count // f) for f in range(1, token_count + 1) if token_count % f == 0 and H % f == 0 and W % (token_count // f) == 0]
    if not cands:
        raise ValueError(f"Self-Transcendence could not map {token_count} tokens onto latent spatial shape {(H, W)}.")
    return min(cands, key=lambda p: abs((p[0] / p[1]) - (H / W)))


class SelfTranscendenceHead:
    """The projector's six trainable tensors as fp32 views at the tail of the adapter arena, their gradient views, the [lo, hi) element range of the gradient arena
    they span, and the bf16 operands the GEMMs read (ops.st_fold, once per training forward; the last Linear's as wide as the columns that are read)."""

    def __init__(self, block: int, D: int, Hp: int, params, grads, flat_lo: int, flat_hi: int, device):
        self.block, self.D, self.Hp = block, D, Hp
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = params
        self.g_W1, self.g_b1, self.g_W2, self.g_b2, self.g_W3, self.g_b3 = grads
        self.flat_lo, self.flat_hi = flat_lo, flat_hi
        e = lambda *shp: torch.empty(*shp, dtype=BF16, device=device)
        self.W1h, self.W1T, self.b1h = e(Hp, D), e(D, Hp), e(Hp)
        self.W2h, self.W2T, self.b2h = e(Hp, Hp), e(Hp, Hp), e(Hp)
        self.W3h, self.W3T, self.b3h = e(D, Hp), None, e(D)

    @property
    def params(self):
        return (self.W1, self.b1, self.W2, self.b2, self.W3, self.b3)

    @property
    def grads(self):
        return (self.g_W1, self.g_b1, self.g_W2, self.g_b2, self.g_W3, self.g_b3)

    @torch.no_grad()
    def init_reference(self, generator=None):
        """nn.Linear's default for the three layers — kaiming_uniform(a = sqrt 5) = U(-1 / sqrt fan_in, 1 / sqrt fan_in) for the weight, the same bound for the bias —
        drawn in fp32, layer by layer, weight first, from the generator given: the adapters' own, behind every A / B draw"""
        for W, b in ((self.W1, self.b1), (self.W2, self.b2), (self.W3, self.b3)):
            bound = 1.0 / math.sqrt(W.shape[1])
            W.uniform_(-bound, bound, generator=generator); b.uniform_(-bound, bound, generator=generator)

    def fold(self, P3: int):
        if self.W3T is None or self.W3T.shape[1] != P3:
            self.W3T = torch.empty(self.Hp, P3, dtype=BF16, device=self.W3h.device)
        ops.st_fold(*self.params, self.W1h, self.W1T, self.b1h, self.W2h, self.W2T, self.b2h, self.W3h, self.W3T, self.b3h)


class SelfTranscendenceTap:
    """One per training forward (kept in its ctx).  `tap(g, view)` after the student block of the saving forward — never in the recompute pass of a checkpointed
    segment — folds the current parameters and runs the projector on the block's image-token rows [B, S, D]: X (a compact copy) -> U1 = X W1^T + b1 -> A1 = silu ->
    U2 = A1 W2^T + b2 -> A2 = silu -> pred = A2 W3[:P]^T + b3[:P] (ops.gemm / ops.silu; P = the columns that are read: the patch size of the diffusion target in
    stage `vae` — a thin GEMM, the reference computes all D columns and discards the rest — and D in stage `self`), then the masked per-sample MSE (ops.st_vae_loss
    against `target` [B, C, H, W] read in place / ops.st_cfg_loss against the teacher's [2B, S, D] capture): `stats` = (guide loss, active count, 1 / (count S P)) on
    the device, G = d (sum of the active samples' squared errors) / d pred written over pred.  `backward(d, dx_view)` right before that block's own backward: the
    chain is linear in G, so ONE device scalar s = d * stats[2] carries the upstream gradient (the weight, the accumulation division) and the normaliser; the three
    Linears' gradients from gemm_tn / colsum_prod through ops.st_wgrad, dX = dU1 W1 added into the gradient with respect to the block's output (ops.st_dx_add;
    dx_view None: the block lies below the first one that trains), then the projector's range goes to `sync`.  `off`: the weight is 0 (stop_step reached) — nothing
    is launched, the output is a constant 0 and the gradient views are zeroed."""

    key = "self_transcendence_guide_loss"

    def __init__(self, head: SelfTranscendenceHead, stage: str, target, sigmas, tmin: float, tmax: float, cfg_scale: float = 1.0, off: bool = False):
        self.head, self.block, self.stage, self.off = head, head.block, stage, off
        self.target, self.sigmas, self.tmin, self.tmax, self.cfg_scale = target, sigmas, float(tmin), float(tmax), float(cfg_scale)
        self.X = self.U1 = self.A1 = self.U2 = self.A2 = self.G = self.stats = self.per_sample = self.output = None
        self.B = self.rows = self.P = 0

    def tap(self, g: int, view):
        if g != self.block or self.off:
            return
        B, S, D = view.shape
        h, dev, t = self.head, view.device, self.target
        if t is None or self.sigmas is None:
            raise ValueError("Self-Transcendence: the training forward needs `self_transcendence_target` and `self_transcendence_sigmas`")
        if self.stage == "vae":
            if t.dim() != 4 or t.shape[0] != B:
                raise ValueError(f"Self-Transcendence VAE guidance does not support latent shape {tuple(t.shape)}.")       # distiller.py `_vae_target_tokens`
            grid = self_transcendence_grid(t.shape[2:], S)
            P = t.shape[1] * (t.shape[2] // grid[0]) * (t.shape[3] // grid[1])
            if P > D:
                raise ValueError(f"Self-Transcendence: the diffusion target has {P} values per token, the projector's output only {D}")
        else:
            if t.dim() != 3 or tuple(t.shape) != (2 * B, S, D):
                raise ValueError(f"Self-Transcendence student and teacher shapes differ: student={(B, S, D)}, teacher={tuple(t.shape)}.")
            P = D
        if D % 64 or h.Hp % 64 or P % 64:
            raise NotImplementedError(f"distillation_method=self_transcendence: D, projector_hidden_dim and the target's values per token must be multiples of 64, the "
                                      f"contraction granule of the GEMMs (got {D}, {h.Hp}, {P}); not built on the st355 path")
        M = B * S
        self.B, self.rows, self.P = B, S, P
        self.X = pad64_empty(M, D, dev)
        self.X.view(B, S, D).copy_(view)
        self.U1, self.U2 = torch.empty(M, h.Hp, dtype=BF16, device=dev), torch.empty(M, h.Hp, dtype=BF16, device=dev)
        self.G = pad64_empty(M, P, dev)
        self.stats, self.per_sample = torch.empty(3, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev)
        sig = self.sigmas.detach().to(device=dev, dtype=F32).reshape(B, -1)[:, 0].contiguous()
        h.fold(P)
        ops.gemm(self.X, h.W1h, bias=h.b1h, out=self.U1)
        self.A1 = ops.silu(self.U1)
        ops.gemm(self.A1, h.W2h, bias=h.b2h, out=self.U2)
        self.A2 = ops.silu(self.U2)
        ops.gemm(self.A2, h.W3h[:P], bias=h.b3h[:P], out=self.G)          # the prediction, overwritten with G by the loss
        if self.stage == "vae":
            ops.st_vae_loss(self.G, t.detach(), grid, sig, self.tmin, self.tmax, self.per_sample, self.stats)
        else:
            ops.st_cfg_loss(self.G, t.detach(), self.cfg_scale, sig, self.tmin, self.tmax, self.per_sample, self.stats)
        self.target = self.sigmas = None

    def finish(self, H: int, W: int):
        if self.off:
            self.output = torch.zeros((), dtype=F32, device=self.head.W1.device)
        elif self.stats is None:
            raise RuntimeError(f"Self-Transcendence: block {self.block} was never reached by the forward")
        else:
            self.output = self.stats[0]
        return self.output

    def backward(self, d, dx_view, accumulate: bool = False, sync=None):
        h = self.head
        if d is None or self.off:                # the guide loss took no part in the loss
            if not accumulate:
                for g in h.grads:
                    g.zero_()
        else:
            M, D, Hp, P, dev = self.B * self.rows, h.D, h.Hp, self.P, self.G.device
            s = (d.detach().to(device=dev, dtype=F32).reshape(1) * self.stats[2:3]).contiguous()
            db = torch.empty(1, P + 2 * Hp, dtype=F32, device=dev)
            db3, db2, db1 = db[:, :P], db[:, P:P + Hp], db[:, P + Hp:]
            ops.colsum_prod(self.G, db3)
            ops.st_wgrad(ops.gemm_tn(pad64(self.G), pad64(self.A2)), db3.view(P), s, h.g_W3[:P], h.g_b3[:P], accumulate=accumulate)
            if P < D and not accumulate:         # the columns that are not read: the reference computes and discards them, their gradients are zero
                h.g_W3[P:].zero_(); h.g_b3[P:].zero_()
            dU2 = ops.silu_bwd(self.U2, ops.gemm(self.G, h.W3T))              # dA2 = G W3[:P]
            ops.colsum_prod(dU2, db2)
            ops.st_wgrad(ops.gemm_tn(pad64(dU2), pad64(self.A1)), db2.view(Hp), s, h.g_W2, h.g_b2, accumulate=accumulate)
            dU1 = ops.silu_bwd(self.U1, ops.gemm(dU2, h.W2T))                 # dA1 = dU2 W2
            ops.colsum_prod(dU1, db1)
            ops.st_wgrad(ops.gemm_tn(pad64(dU1), pad64(self.X)), db1.view(Hp), s, h.g_W1, h.g_b1, accumulate=accumulate)
            if dx_view is not None:
                ops.st_dx_add(ops.gemm(dU1, h.W1T), s, dx_view)               # dX = dU1 W1
        if sync is not None:
            sync.ready(h.flat_lo, h.flat_hi)
        self.X = self.U1 = self.A1 = self.U2 = self.A2 = self.G = None


def sincos_2d_hw(embed_dim: int, h: int, w: int, base_size: int, interpolation_scale: float) -> torch.Tensor:
    """diffusers get_2d_sincos_pos_embed on a (h, w) grid: [h * w, embed_dim] fp32 (first half from the w coordinate, which varies fastest; sin then cos)"""
    gh = (torch.arange(h, dtype=torch.float32) / (h / base_size) / interpolation_scale).double()
    gw = (torch.arange(w, dtype=torch.float32) / (w / base_size) / interpolation_scale).double()
    cw = gw[None, :].expand(h, w).reshape(-1)
    chh = gh[:, None].expand(h, w).reshape(-1)

    def one_d(dim, pos):
        omega = 1.0 / 10000 ** (torch.arange(dim // 2, dtype=torch.float64) / (dim / 2.0))
        out = pos[:, None] * omega[None, :]
        return torch.cat([out.sin(), out.cos()], dim=1)

    return torch.cat([one_d(embed_dim // 2, cw), one_d(embed_dim // 2, chh)], dim=1).float()


# ------------------------------------------------------------------------------------------------
# one bf16 arena under every base parameter
# ------------------------------------------------------------------------------------------------
class ArenaModule(nn.Module):
    """Every weight / bias / norm weight / modulation row is a view of ONE bf16 arena (allocation order = arena order): full-rank training then has a gradient
    arena of the same layout, ONE fused optimizer launch and contiguous slices for the gradient exchange.  The subclass's `_build()` allocates through
    `_alloc` and names parameters through `_reg`; it runs twice — pass 1 counts on meta tensors, pass 2 hands out the views.  Hooks: `_extra_state()` (checkpoint
    entries that are no parameters), `_weights_changed()` (drop what was derived from the weights), `_all_linears()`."""

    def _build_arena(self, dev):
        self._arena_numel, self._counting = 0, True
        self._build()
        self.arena = torch.zeros(self._arena_numel, dtype=BF16, device=dev)
        self._arena_numel, self._counting = 0, False
        self._build()

    def _alloc(self, *shape):
        n = 1
        for d in shape:
            n *= d
        off = self._arena_numel
        self._arena_numel += (n + 7) // 8 * 8               # every tensor starts 16-byte aligned inside the arena
        if self._counting:
            return torch.empty(*shape, dtype=BF16, device="meta")
        return self.arena[off:off + n].view(*shape)

    def _reg(self, name, param):
        if not self._counting:
            attach(self, name, param)

    def _extra_state(self) -> Dict[str, torch.Tensor]:
        return {}

    def _weights_changed(self):
        self._prepared = False

    @torch.no_grad()
    def load_flat_state(self, state: Dict[str, torch.Tensor]):
        """copy a {checkpoint name: tensor} dict into the fused buffers (names = diffusers state-dict keys)"""
        own = dict(self.named_parameters())
        # (an Internal Guidance head / a NextLat predictor is optional in a file: without one it keeps the reference's initial values)
        missing = [k for k in own if k not in state and ".lora_" not in k and ".lokr_" not in k and not k.startswith(("internal_guidance_head.", "nextlat_predictor.", "crepa_projector.", "self_transcendence_projector."))]
        if missing:
            raise KeyError(f"missing weights: {missing[:5]} ... ({len(missing)})")
        own.update(self._extra_state())
        for k, v in state.items():
            if k in own:
                own[k].data.copy_(v.to(device=own[k].device, dtype=own[k].dtype))
        self._weights_changed()

    def load_diffusers_state(self, state: Dict[str, torch.Tensor]):
        self.load_flat_state(state)

    def diffusers_state_dict(self) -> Dict[str, torch.Tensor]:
        """{diffusers checkpoint key: tensor} of the base parameters (the parameter names ARE the checkpoint keys) + `_extra_state()`: what `save_pretrained`
        writes (training/trainer.py save_state)"""
        sd = {k: v.detach() for k, v in self.named_parameters() if ".lora_" not in k and ".lokr_" not in k}
        sd.update({k: v.detach() for k, v in self._extra_state().items()})
        return sd

    @torch.no_grad()
    def init_synthetic(self, seed: int = 42):
        """seed-deterministic random init on device, same distribution family as the oracle's init_params (benchmarks)."""
        g = torch.Generator(device=self.device_).manual_seed(seed)
        for name, p in self.named_parameters():
            if ".lora_" in name or ".lokr_" in name:
                continue
            if "norm_q" in name or "norm_k" in name or "norm_added" in name:
                p.data.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device=self.device_))
            elif name.endswith(".bias"):
                p.data.copy_(0.02 * torch.randn(p.shape, generator=g, device=self.device_))
            else:
                p.data.copy_(torch.randn(p.shape, generator=g, device=self.device_, dtype=BF16) * (1.0 / math.sqrt(p[0].numel())))      # fan-in
        self._weights_changed()

    def trainable_parameters(self):
        return list(self._full_params) if self.full else list(self._lora_params)

    # ---- adapters off / on (peft's names: the reference's distillers call them on the trained component) ----
    def disable_lora(self):
        """Take every LoRA group off its site: the engine forward then launches exactly the base model's sequence (no down projection, an empty K-extension, the
        block-level entry points get NULL adapter operands) and, with no group left, neither packs nor drops.  Meant for no-grad forwards between training
        forwards (Flow-DPO's reference model); `enable_lora()` puts the same groups back.  DoRA and LoKr fold their adapters into the weights and are refused."""
        if getattr(self, "_lora_off", None) is not None:
            return
        if getattr(self, "lora_dora", False) or getattr(self, "lora_lokr", False):
            raise NotImplementedError("disable_lora: switching a DoRA / LoKr adapter off (its fold lives in the weights) is not built on the st355 path")
        sites = [(l, l.lora) for l in self._all_linears() if getattr(l, "lora", None) is not None]
        mod = getattr(self, "mod_lora", None)
        if len(sites) + (mod is not None) != len(self.lora_groups):
            raise RuntimeError(f"disable_lora: {len(self.lora_groups)} adapter groups but {len(sites) + (mod is not None)} sites found")
        self._lora_off = (sites, self.lora_groups, mod, getattr(self, "lora_dropout", None))
        for l, _ in sites:
            l.lora = None
        self.lora_groups = []
        if mod is not None:
            self.mod_lora = None
        if hasattr(self, "lora_dropout"):
            self.lora_dropout = None

    def enable_lora(self):
        off, self._lora_off = getattr(self, "_lora_off", None), None
        if off is None:
            return
        sites, groups, mod, drop = off
        for l, g in sites:
            l.lora = g
        self.lora_groups = groups
        if mod is not None:
            self.mod_lora = mod
        if hasattr(self, "lora_dropout"):
            self.lora_dropout = drop

    @contextmanager
    def lora_disabled(self):
        self.disable_lora()
        try:
            yield self
        finally:
            self.enable_lora()

    @contextmanager
    def teacher_values(self, flat):
        """Inside: the adapters' GEMM operands (LoraGroup.pack) are built from `flat` — an fp32 buffer laid out like `lora_flat`, e.g. the EMA's `shadow_flat` —
        instead of the masters: every group's A / B lists point at the same offsets of `flat`, and every forward packs from what they point at.  On exit the lists
        point at the masters again and the operands are rebuilt from them.  The masters are never written (no store / copy_to / restore round trip).  Standard LoRA
        groups only: DoRA, LoKr and T-LoRA fold further state into their operands and are refused."""
        groups = list(getattr(self, "lora_groups", None) or [])
        if not groups or getattr(self, "lora_flat", None) is None:
            raise RuntimeError("teacher_values: the component has no adapter arena (add_lora_adapter() first)")
        if getattr(self, "lora_dora", False) or getattr(self, "lora_lokr", False) or getattr(self, "lora_tlora", None) is not None or not all(type(g) is LoraGroup for g in groups):
            raise NotImplementedError("teacher_values: only standard LoRA groups pack from a flat buffer (DoRA / LoKr / T-LoRA fold further state) on the st355 path")
        base = self.lora_flat
        if flat.dtype != F32 or flat.device != base.device or flat.dim() != 1 or not flat.is_contiguous():
            raise ValueError("teacher_values: expected a contiguous 1-D fp32 buffer on the adapters' device")
        view = lambda t: flat[(t.data_ptr() - base.data_ptr()) // 4:][:t.numel()].view(t.shape)
        if max(g.flat_hi for g in groups) > flat.numel():
            raise ValueError(f"teacher_values: the buffer holds {flat.numel()} elements, the adapters end at {max(g.flat_hi for g in groups)}")
        kept = [(g.A, g.B) for g in groups]
        try:
            for g in groups:
                g.A, g.B = [view(t) for t in g.A], [view(t) for t in g.B]
            yield self
        finally:
            for g, (A, B) in zip(groups, kept):
                g.A, g.B = A, B
                g.pack()

    def _refresh_transposed(self):
        """W^T follows the weights (2 B read + 2 B write per parameter per step: ~12 ms for Flux.1-dev's 12 B parameters, ~1 ms for SD3-Medium)"""
        for l in self._all_linears():
            if getattr(l, "wT", None) is not None:
                ops.transpose(l.w, out=l.wT)


def mod_grads(D: int, dn, x_in, rows: int, k_shift: int, k_scale: int, dm, xhat=None):
    """d shift = sum_t dY, d scale = sum_t dY * LN(x) of one AdaLN instance, per sample, into chunks k_shift / k_scale of its slice `dm` of the modulation-row
    gradient.  x_in = the LayerNorm's input (LN(x) is recomputed: recovering it from the saved modulated output divides by 1 + scale, singular where a scale
    entry is -1), or xhat = LN(x) when the caller already has it."""
    ops.colsum_prod(dn, dm[:, k_shift * D:(k_shift + 1) * D], rows_per_batch=rows)
    ops.colsum_prod(dn, dm[:, k_scale * D:(k_scale + 1) * D], b=ops.layer_norm_xhat(x_in) if xhat is None else xhat, rows_per_batch=rows)


# ------------------------------------------------------------------------------------------------
# the backward of the one autograd node per network (_FluxFn / _FluxFullFn, _SD3Fn / _SD3FullFn, _PixArtLoraFn / _CtrlFn, _UNetFn)
# ------------------------------------------------------------------------------------------------
def node_backward(fctx, full: bool, *d_outs, run=None, whole: bool = False, covered: bool = False, cut=None):
    """Runs the model's hand-written backward on the node's kept context between the gradient exchange's begin / finish, then hands autograd a private flat
    copy (one copy per step) so that .grad never aliases the arena the next backward overwrites; the per-parameter gradients returned stay views of ONE
    contiguous buffer, which the fused optimizer / RCCL all-reduce exploit.  full: the bf16 gradient arena and `_full_params`, else the adapters' fp32 one.
    run: what runs the backward on (context, *d_outs), the model's `_engine_backward[_full]` by default.  whole: the arena is handed to the exchange in one piece
    after the backward (nothing reported itself ready).  covered: refuse an exchange that did not take every element.  cut: the (parameters, [(offset, n)]) the
    flat gradient is cut by, else `_full_params` / `_lora_params` and their offsets."""
    model = fctx.model
    sync = model.grad_sync
    if sync is not None:
        sync.begin()
    (run or (model._engine_backward_full if full else model._engine_backward))(fctx.ectx, *d_outs)
    fctx.ectx = None
    arena = model.grad_arena if full else model.lora_grad_flat
    if sync is not None:
        if whole:
            sync.ready(0, arena.numel())
        model.grad_scale_from_sync = sync.finish()   # every slice reduced (SUM over replicas); the optimizer folds 1/world
        if covered and (sent := sum(hi - lo for lo, hi in sync.launched_slices)) != arena.numel():
            raise RuntimeError(f"gradient sync covered {sent} of {arena.numel()} elements: a parameter's gradient was never reported ready")
    from .training.grad_sync import hand_over_gradients
    model._last_grad_flat = gflat = hand_over_gradients(model, arena)
    params, offsets = cut or ((model._full_params, model._full_offsets) if full else (model._lora_params, model._lora_offsets))
    return tuple(gflat[off:off + n].view_as(p) for (off, n), p in zip(offsets, params))


# ------------------------------------------------------------------------------------------------
# full-rank training: what one backward shares between the families
# ------------------------------------------------------------------------------------------------
class FullGrads:
    """One per backward of full-rank training.  Owns d loss / d (modulation Linear output) `dmod` [B, mod_total] fp32, the per-width bias temporaries and the
    zero-padded silu(temb) `st_p`.  Reads `lin.gw` / `lin.gb` / `model.g_mod_*` at call time (SD3 re-points them between its two gradient arenas).
    `front_hi`: the arena offset below which the fused modulation matrix must lie for its rows to be handed to `sync` block by block."""

    def __init__(self, model, B: int, dev, sync, front_hi: int, st):
        self.model, self.B, self.dev, self.sync = model, B, dev, sync
        self.Bp = (B + 63) // 64 * 64
        self.dmod = torch.zeros(B, model.mod_total, dtype=F32, device=dev)
        self.st_p = self._pad_batch(st)
        self._tmp_b = {}
        self.mw_lo = (model.mod_w.data_ptr() - model.arena.data_ptr()) // model.arena.element_size()
        self.mw_hi = self.mw_lo + model.mod_total * model.D
        self.mod_in_front = 0 <= self.mw_lo and self.mw_hi <= front_hi
        self.mod_rows_lo = model.mod_total                # rows [mod_rows_lo, mod_total) of dW_mod are written (and handed over)

    def _pad_batch(self, t):
        """[B, C] -> bf16 [Bp, C], zero rows up to the TN GEMM's granule"""
        o = torch.zeros(self.Bp, t.shape[1], dtype=BF16, device=self.dev)
        o[:self.B] = t
        return o

    def bgrad(self, lin, dy):
        N = dy.shape[1]
        t = self._tmp_b.get(N)
        if t is None:
            t = self._tmp_b[N] = torch.empty(1, N, dtype=F32, device=self.dev)
        ops.colsum_prod(dy, t)
        lin.gb.copy_(t[0])

    def wgrad(self, lin, dy, x, bias: bool = True):
        """dW = dY^T X ; db = colsum(dY)   (into the gradient arena views of `lin`; bias=False: the bias gradient was already taken by a fused pass)"""
        ops.gemm_tn(pad64(dy), pad64(x), out=lin.gw)
        if bias:
            self.bgrad(lin, dy)

    def mod_grads(self, dn, x_in, rows, k_shift, k_scale, dm, xhat=None):
        mod_grads(self.model.D, dn, x_in, rows, k_shift, k_scale, dm, xhat)

    def mod_rows_grad(self, r0: int):
        """The fused modulation matrix gets its gradient rows block by block: dW_mod[r0:r1] = dmod[:, r0:r1]^T silu(temb) as soon as the block that owns rows
        [r0, r1) has run, so that the exchange takes them behind the backward instead of as one exposed region after it.  Same arithmetic per row (one 64-deep
        contraction over the zero-padded batch): bit-equal to the one-product form."""
        m, r1 = self.model, self.mod_rows_lo
        if r1 <= r0:
            return
        ops.gemm_tn(self._pad_batch(self.dmod[:, r0:r1]), self.st_p, out=m.g_mod_w[r0:r1])
        self.mod_rows_lo = r0
        if self.sync is not None and self.mod_in_front:
            self.sync.ready(self.mw_lo + r0 * m.D, self.mw_lo + r1 * m.D)

    def mod_linear_bwd(self, temb):
        """modulation Linear mod = silu(temb) W_mod^T + b: the rows of dW_mod not handed over yet, db, and d temb"""
        m, B, dev = self.model, self.B, self.dev
        D = m.D
        dmod_p = self._pad_batch(self.dmod)
        self.mod_rows_grad(0)
        tb = torch.empty(1, m.mod_total, dtype=F32, device=dev)
        ops.colsum_prod(dmod_p, tb)
        m.g_mod_b.copy_(tb[0])
        # d silu(temb) = dmod @ W_mod -> [B, D], as (W_mod^T dmod^T)^T with the TN GEMM.  The contraction runs over the mod_total rows of W_mod (1.06 M for
        # Flux.1-dev): walked in row blocks that stay inside the TN GEMM's 2 GiB operand window, accumulated into one [D, B8] output
        B8 = 8 * ((B + 7) // 8)
        dmod_t = ops.transpose(dmod_p[:B8])                                   # [mod_total, B8]
        blk_rows = max(64, (getattr(m, "_tn_window_bytes", (1 << 31) - 1) // (2 * max(D, B8))) // 64 * 64)        # (attribute: tests shrink the window)
        acc = torch.empty(D, B8, dtype=BF16, device=dev)
        for i, r0 in enumerate(range(0, m.mod_total, blk_rows)):
            r1 = min(m.mod_total, r0 + blk_rows)
            ops.gemm_tn(m.mod_w[r0:r1], dmod_t[r0:r1], out=acc, accumulate=i > 0)
        return ops.silu_bwd(temb, ops.transpose(acc)[:B].contiguous())

    def mlp_bwd(self, l1, l2, x_in, pre1, act1, dy):
        """TimestepEmbedding / guidance / pooled-text projection: y = l2(silu(l1(x)))"""
        dyp = self._pad_batch(dy)
        ops.gemm_tn(dyp, self._pad_batch(act1), out=l2.gw)
        self.bgrad(l2, dyp)
        d1p = self._pad_batch(ops.silu_bwd(pre1, ops.gemm(dy, l2.wT)))
        ops.gemm_tn(d1p, self._pad_batch(x_in), out=l1.gw)
        self.bgrad(l1, d1p)

    def ready_front(self, hi: int):
        """hand over what lies around the modulation matrix's rows below arena offset `hi` (embedders, the modulation bias)"""
        if self.sync is None:
            return
        if self.mod_in_front:
            self.sync.ready(self.mw_hi, hi)
            self.sync.ready(0, self.mw_lo)
        else:
            self.sync.ready(0, hi)

"""The slab-level gradient checker behind tests/test_engine_algebra_cpu.py (wide arithmetic, CPU) and tests/test_engine_parity_gpu.py (bf16 kernels, MI355X)
— TEST INFRASTRUCTURE ONLY.

Unit of comparison: the SLAB.  Every parameter tensor (or LoRA / DoRA / LoKr factor) is one slab; a tensor whose leading dimension is k * D with k > 1 (the
fused modulation matrices and biases, fused projections; D the model width of that stream) is split into its k row slabs of D.  No tensor is skipped.

CPU rule (wide arithmetic, `check_wide`): per slab  err = ||g_engine - g_ref64||,  noise = ||g_oracle_fp32 - g_ref64||  (the oracle run a second time in fp32), and

    err <= 16 * noise + 1e-6 * ||g_ref64 slab|| + 1e-7 * gmax / sqrt(number of slabs)

with gmax the largest tensor gradient norm of the case.  The allowance is measured on the reference side alone.  16: the engine's operation order and count differ
from autograd's (fused epilogues, chunked sums, recomputation); the two floors are fp32 roundoff for slabs that cancel (an all-zero reference slab is held by the
last floor — nothing divides by a slab norm).  The prediction (one slab) and the loss follow the same rule.

Device rule (`check_device`): the engines run bf16 kernels, so the yardstick is rounding noise, taken from the reference side: the kernel-contract emulator at bf16.
Per slab (slabs of fewer than 1024 elements pooled per block and kind until they reach 1024)  E_gpu = ||g_gpu - g_ref64||,  E_emu = ||g_emu - g_ref64||  and

    E_gpu <= 3 * E_emu + 1/2 ulp_bf16(||slab||_inf) * sqrt(n)."""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, field

import torch

NOISE_FACTOR, REL_FLOOR, ABS_FLOOR = 16.0, 1e-6, 1e-7            # the CPU rule's constants (see the module docstring)
DEVICE_FACTOR, POOL_MIN = 3.0, 1024                               # the device rule's


def split_slabs(name: str, t: torch.Tensor, width: int):
    """[(slab name, tensor)]: `t` itself, or its k row slabs of `width` when its leading dimension is k * width with k > 1"""
    if t.dim() >= 1 and width and t.shape[0] > width and t.shape[0] % width == 0:
        k = t.shape[0] // width
        return [(f"{name}[{i}/{k}]", t[i * width:(i + 1) * width]) for i in range(k)]
    return [(name, t)]


def family(name: str) -> str:
    """the row of the report a slab belongs to"""
    base = name.split("[")[0]
    if base in ("prediction", "loss"):
        return base
    for tag, fam in ((".lora_A.", "adapter A"), (".lora_B.", "adapter B"), (".lokr_", "LoKr factor"), ("lora_magnitude", "DoRA magnitude"), (".magnitude", "DoRA magnitude")):
        if tag in base:
            return fam
    if re.search(r"norm(_added)?_[qk]\d?\.", base) or re.search(r"\.norm_[qk]\d?\.", base):
        return "q/k norm weight"
    kind = "bias" if base.endswith("bias") else "weight"
    if re.search(r"norm\w*\.linear\.|adaLN|scale_shift_table|norm_out\.linear\.", base):
        return "modulation " + kind
    if re.search(r"(^|\.)(norm\d*|group_norm|conv_norm_out|norm_\w+)\.(weight|bias)$", base):
        return "norm " + kind
    return kind


def block_of(name: str) -> str:
    m = re.search(r"((?:single_)?transformer_blocks|joint_blocks|blocks|down_blocks|up_blocks|mid_block|controlnet_blocks)\.(\d+)", name)
    return f"{m.group(1)}.{m.group(2)}" if m else "trunk"


@dataclass
class Row:
    name: str
    err: float
    allow: float
    ref: float
    n: int
    noise: float = 0.0
    fam: str = ""

    @property
    def ratio(self):
        return self.err / self.allow if self.allow > 0 else (0.0 if self.err == 0 else math.inf)


@dataclass
class Report:
    case: str
    rows: list = field(default_factory=list)

    def over(self):
        return [r for r in self.rows if not r.err <= r.allow]

    def worst(self):
        return max(self.rows, key=lambda r: r.ratio)

    def by_family(self):
        fam = {}
        for r in self.rows:
            fam.setdefault(r.fam or family(r.name), []).append(r)
        return {k: (len(v), max(v, key=lambda r: r.ratio), sorted(x.ratio for x in v)[len(v) // 2]) for k, v in sorted(fam.items())}

    def table(self):
        lines = [f"[{self.case}] {len(self.rows)} slabs"]
        for k, (n, w, med) in self.by_family().items():
            lines.append(f"  {k:18s} {n:5d} slabs  worst err/allow {w.ratio:9.3e}  median {med:9.3e}  at {w.name}")
        return "\n".join(lines)

    def record(self):
        """print the per-family table; append it to $ENGINE_PARITY_REPORT (one `case|family|slabs|worst|median|slab` line each) when that is set — how profiles/engine_parity.md is made"""
        print(self.table())
        path = os.environ.get("ENGINE_PARITY_REPORT")
        if path:
            with open(path, "a") as f:
                for k, (n, w, med) in self.by_family().items():
                    f.write(f"{self.case}|{k}|{n}|{w.ratio:.3e}|{med:.3e}|{w.name}\n")
        return self

    def assert_ok(self):
        bad = sorted(self.over(), key=lambda r: -r.ratio)
        assert not bad, f"[{self.case}] {len(bad)} of {len(self.rows)} slabs over their allowance; worst: " + "; ".join(
            f"{r.name}: err {r.err:.3e} > allow {r.allow:.3e} (noise {r.noise:.3e}, |ref| {r.ref:.3e})" for r in bad[:6])
        return self


def _d(t):
    return t.detach().to("cpu", torch.float64)


def _slab_list(grads: dict, width):
    out = []
    for name, t in grads.items():
        out += split_slabs(name, t, width(name, t) if callable(width) else width)
    return out


def check_wide(case: str, engine: dict, ref64: dict, ref32: dict, width, scalars: dict | None = None) -> Report:
    """the CPU rule.  `engine` / `ref64` / `ref32`: {parameter name: gradient} with the same keys (a missing or None engine gradient counts as zeros: nothing
    is skipped); `width`: D, or f(name, tensor) -> D; `scalars`: {"prediction" | "loss": (engine, ref64, ref32)} held to the same rule as one slab each."""
    assert set(ref64) == set(ref32), sorted(set(ref64) ^ set(ref32))
    missing = set(ref64) - set(engine)
    assert not missing, f"[{case}] the engine returned no gradient entry for {sorted(missing)[:5]}"
    assert not (set(engine) - set(ref64)), f"[{case}] no reference gradient for {sorted(set(engine) - set(ref64))[:5]}"
    r64 = {k: _d(v) for k, v in ref64.items()}
    gmax = max(v.norm().item() for v in r64.values())
    s64 = _slab_list(r64, width)
    s32 = _slab_list({k: _d(ref32[k]) for k in r64}, width)
    sen = _slab_list({k: (torch.zeros_like(r64[k]) if engine[k] is None else _d(engine[k]).reshape(r64[k].shape)) for k in r64}, width)
    floor = ABS_FLOOR * gmax / math.sqrt(len(s64))
    rep = Report(case)
    for (name, g64), (_, g32), (_, ge) in zip(s64, s32, sen):
        assert torch.isfinite(ge).all(), f"[{case}] {name}: non-finite engine gradient"
        noise, ref = (g32 - g64).norm().item(), g64.norm().item()
        rep.rows.append(Row(name, (ge - g64).norm().item(), NOISE_FACTOR * noise + REL_FLOOR * ref + floor, ref, g64.numel(), noise))
    for name, (e, a, b) in (scalars or {}).items():
        e, a, b = _d(torch.as_tensor(e)), _d(torch.as_tensor(a)), _d(torch.as_tensor(b))
        noise, ref = (b - a).norm().item(), a.norm().item()
        rep.rows.append(Row(name, (e.reshape(a.shape) - a).norm().item(), NOISE_FACTOR * noise + REL_FLOOR * ref + floor, ref, a.numel(), noise))
    return rep


def check_equal_wide(case: str, a: dict, b: dict, ref64: dict, ref32: dict, width) -> Report:
    """recomputation: wide-mode gradients with (`a`) and without (`b`) recomputation are equal to the same per-slab allowance"""
    rep = check_wide(case, a, ref64, ref32, width)
    sa = _slab_list({k: _d(a[k]) for k in ref64}, width)
    sb = _slab_list({k: _d(b[k]) for k in ref64}, width)
    for row, (_, x), (_, y) in zip(rep.rows, sa, sb):
        row.err = (x - y).norm().item()
    return rep


def ulp_bf16(x: float) -> float:
    """spacing of bf16 numbers at magnitude x (8 significant bits); the smallest normal's spacing below it"""
    x = max(abs(float(x)), 2.0 ** -126)
    return 2.0 ** (math.floor(math.log2(x)) - 7)


def pool_small(slabs, min_elems=POOL_MIN):
    """[(name, [tensors])]: slabs of fewer than `min_elems` elements pooled per (block, kind) — in order, a pool closes once it reaches `min_elems`"""
    out, open_ = [], {}
    for name, t in slabs:
        if t.numel() >= min_elems:
            out.append((name, [name]))
            continue
        key = (block_of(name), family(name))
        p = open_.setdefault(key, [f"pool:{key[0]}:{key[1]}#{sum(1 for n, _ in out if n.startswith(f'pool:{key[0]}:{key[1]}#'))}", [], 0])
        p[1].append(name); p[2] += t.numel()
        if p[2] >= min_elems:
            out.append((p[0], p[1])); del open_[key]
    for p in open_.values():
        out.append((p[0], p[1]))
    return out


def check_device(case: str, gpu: dict, emu: dict, ref64: dict, width, scalars: dict | None = None) -> Report:
    """the device rule.  Row.noise carries E_emu, Row.err E_gpu; `ratio` is err / allowance, `Row.err / Row.noise` the recorded E_gpu / E_emu"""
    assert set(gpu) == set(emu) == set(ref64), (sorted(set(gpu) ^ set(ref64))[:5], sorted(set(emu) ^ set(ref64))[:5])
    r64 = {k: _d(v) for k, v in ref64.items()}
    by = lambda d: dict(_slab_list({k: (torch.zeros_like(r64[k]) if d[k] is None else _d(d[k]).reshape(r64[k].shape)) for k in r64}, width))
    s64, sg, se = dict(_slab_list(r64, width)), by(gpu), by(emu)
    rep = Report(case)
    cat = lambda d, names: torch.cat([d[n].reshape(-1) for n in names])
    groups = pool_small(list(s64.items()))
    for name, (g, e, r) in (scalars or {}).items():
        s64[name], sg[name], se[name] = _d(r), _d(g).reshape(r.shape), _d(e).reshape(r.shape)
        groups.append((name, [name]))
    for gname, names in groups:
        r, g, e = cat(s64, names), cat(sg, names), cat(se, names)
        assert torch.isfinite(g).all(), f"[{case}] {gname}: non-finite device gradient"
        e_emu = (e - r).norm().item()
        allow = DEVICE_FACTOR * e_emu + 0.5 * ulp_bf16(r.abs().max().item()) * math.sqrt(r.numel())
        rep.rows.append(Row(gname, (g - r).norm().item(), allow, r.norm().item(), r.numel(), e_emu, family(names[0])))
    return rep


def device_ratios(rep: Report):
    """[(family, slabs, worst E_gpu / E_emu, median, slabs whose E_emu is exactly zero)] — what profiles/engine_parity.md records for the device"""
    fam = {}
    for r in rep.rows:
        fam.setdefault(r.fam or family(r.name), []).append(r)
    out = []
    for k, v in sorted(fam.items()):
        q = sorted(r.err / r.noise for r in v if r.noise > 0)
        out.append((k, len(v), q[-1] if q else float("nan"), q[len(q) // 2] if q else float("nan"), len(v) - len(q)))
    return out


def record_device(rep: Report):
    """print worst / median E_gpu / E_emu per family; append `case|family|slabs|worst|median|zero-noise slabs` lines to $ENGINE_PARITY_REPORT when that is set"""
    rows = device_ratios(rep)
    print(f"[{rep.case}] {len(rep.rows)} slabs (small ones pooled); worst err/allowance {rep.worst().ratio:.3f} at {rep.worst().name}")
    for k, n, w, med, z in rows:
        print(f"  {k:18s} {n:5d} slabs  E_gpu/E_emu worst {w:7.3f}  median {med:7.3f}" + (f"  ({z} with E_emu = 0)" if z else ""))
    path = os.environ.get("ENGINE_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            for k, n, w, med, z in rows:
                f.write(f"{rep.case}|{k}|{n}|{w:.3f}|{med:.3f}|{z}\n")
    return rep

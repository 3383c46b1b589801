#!/usr/bin/env python3
"""Generate tests/golden/adapter_arena_layout.json: the lay-out and the initial values of the fp32 adapter arena (`lora_flat`) of every adapter builder, on the CPU.

Every variant below is built at the tiny architectures of the host-sequencing tests with rank 4, seed 7 and init_b_std 0.0 / 0.02, and recorded as

  entries           the ordered (parameter name, offset in lora_flat, shape) of `_lora_params`; with `sha256` of the bytes where the initial value is a scaled draw
                    or a constant (lora_A / lora_B / lokr_w1, and lokr_w2 without init_norm) — DoRA magnitudes, an init_norm w2 and the heads' values come out of
                    reductions and are held by their own tests
  numel             lora_flat.numel()
  groups / dora / heads   every (flat_lo, flat_hi)
  named_parameters  SHA-256 over name, shape, dtype and requires_grad of everything named_parameters() yields, in its order

tests/test_adapter_arena_cpu.py rebuilds every variant through `build` / `snapshot` below and compares exactly.  Run it at the commit whose lay-out is to be held:

    python tools/gen_adapter_arena_golden.py
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

OUT = ROOT / "tests" / "golden" / "adapter_arena_layout.json"
RANK, SEED, B_STDS = 4, 7, (0.0, 0.02)


def _flux(targets, single=1):
    def make(b_std):
        from simpletuner_amd.flux.transformer import FluxTransformer2DModel
        from tests import parity_utils as PU
        m = FluxTransformer2DModel(device="cpu", **PU.small_flux_cfg(layers=1, single=single))
        m.add_lora_adapter(rank=RANK, seed=SEED, init_b_std=b_std, targets=targets)
        return m
    return make


def _sd3(lokr=None, sd35=False, heads=(), **kw):
    def make(b_std):
        from simpletuner_amd.sd3.transformer import SD3Transformer2DModel
        from tests.test_sd3_host_sequencing_cpu import _arch
        m = SD3Transformer2DModel(device="cpu", **_arch(2, **(dict(qk_norm="rms_norm", dual=(0,)) if sd35 else {})))
        m.init_synthetic(5)
        if heads == ("ig",):
            m.set_internal_guidance(1)
        elif heads == ("nextlat",):
            m.set_nextlat(1)
        elif heads:          # both heads at once: the public setters refuse the pair, the builder lays both out (IG, then NextLat from its 8-element boundary)
            m._ig_block = m._nl_block = 1
        if lokr is not None:
            m.add_lokr_adapter(seed=SEED, **lokr)
        else:
            m.add_lora_adapter(rank=RANK, seed=SEED, init_b_std=b_std, **kw)
        return m
    return make


def _pixart(b_std):
    from simpletuner_amd.pixart.transformer import PixArtTransformer2DModel
    from tests.test_pixart_host_sequencing_cpu import ARCH
    m = PixArtTransformer2DModel(device="cpu", **ARCH)
    m.add_lora_adapter(rank=RANK, seed=SEED, init_b_std=b_std)
    return m


def _unet(b_std):
    from simpletuner_amd.unet.unet import UNet2DConditionModel
    from tests.test_unet_host_sequencing_cpu import SMALL
    m = UNet2DConditionModel(device="cpu", **SMALL)
    m.add_lora_adapter(rank=RANK, seed=SEED, init_b_std=b_std)
    return m


LOKR = dict(factors={"Attention": 2, "FeedForward": 2})          # D = 128: 2 x 64 on every side (the builder's own default factors need a wider model)
VARIANTS = {
    "flux/default": _flux("default"), "flux/all+ffs": _flux("all+ffs"), "flux/all+ffs+embedder": _flux("all+ffs+embedder"), "flux/ai-toolkit": _flux("ai-toolkit"),
    "flux/nano": _flux("nano", single=9),
    "sd3/default": _sd3(), "sd3/all": _sd3(targets="all"), "sd3/dual": _sd3(sd35=True), "sd3/dora": _sd3(dora=True), "sd3/ig": _sd3(heads=("ig",)),
    "sd3/nextlat": _sd3(heads=("nextlat",)), "sd3/ig+nextlat": _sd3(heads=("ig", "nextlat")), "sd3/lokr": _sd3(lokr=LOKR), "sd3/lokr+init_norm": _sd3(lokr=dict(LOKR, init_norm=1e-3)),
    "pixart/lora": _pixart, "unet/lora": _unet,
}


def cases():
    """(key, variant, init_b_std): the LoKr builder takes no init_b_std, so it is built once"""
    return [(f"{v}@b_std={b}", v, b) for v in VARIANTS for b in B_STDS if not (v.startswith("sd3/lokr") and b)]


def build(variant: str, b_std: float, monkeypatch):
    """the model of one variant, on the ops emulator (DoRA's first fold, the UNet's K-major copies and LoKr's refusal checks launch)"""
    from tests import lokr_ref
    lokr_ref.install(monkeypatch)
    return VARIANTS[variant](b_std)


def offset_of(model, p) -> int:
    flat = model.lora_flat
    return (p.data_ptr() - flat.data_ptr()) // flat.element_size()


def snapshot(model, variant: str) -> dict:
    name_of = {id(p): n for n, p in model.named_parameters()}
    hashed = (".lora_A.", ".lora_B.", ".lokr_w1") + ((".lokr_w2",) if "init_norm" not in variant else ())
    entries = []
    for p in model._lora_params:
        e = {"name": name_of[id(p)], "offset": offset_of(model, p), "shape": list(p.shape)}
        if any(h in e["name"] for h in hashed):
            e["sha256"] = hashlib.sha256(p.detach().contiguous().numpy().tobytes()).hexdigest()
        entries.append(e)
    named = "\n".join(f"{n} {list(p.shape)} {p.dtype} {p.requires_grad}" for n, p in model.named_parameters())
    return {"entries": entries, "numel": model.lora_flat.numel(), "grad_numel": model.lora_grad_flat.numel(),
            "groups": [[g.flat_lo, g.flat_hi] for g in model.lora_groups],
            "dora": [[g.dora.flat_lo, g.dora.flat_hi] for g in model.lora_groups if g.dora is not None],
            "heads": {k: [h.flat_lo, h.flat_hi] for k in ("_ig", "_nl") if (h := getattr(model, k, None)) is not None},
            "named_parameters": hashlib.sha256(named.encode()).hexdigest()}


def main():
    import pytest
    out = {}
    for key, variant, b_std in cases():
        mp = pytest.MonkeyPatch()
        try:
            out[key] = snapshot(build(variant, b_std, mp), variant)
        finally:
            mp.undo()
        print(f"{key}: {len(out[key]['entries'])} entries, {out[key]['numel']} elements")
    OUT.write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()

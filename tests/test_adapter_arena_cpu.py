"""The fp32 adapter arena (engine.AdapterArena / engine.lora_pairs) and the one node backward that cuts its gradient (engine.node_backward), on the CPU.

(a) every adapter builder — Flux, SD3 (LoRA, dual attention, DoRA, the heads, LoKr), PixArt, UNet — against tests/golden/adapter_arena_layout.json, recorded by
    tools/gen_adapter_arena_golden.py from the hand-rolled builders these replaced: names, order, offsets, shapes, the total, every flat_lo / flat_hi and the bytes of
    every drawn or constant entry, exactly;
(b) `_lora_offsets` is where each parameter lies, and PixArt's pad lanes start at zero;
(c) an arena with a gap (an odd-sized entry before an 8-aligned one): the gradients `node_backward` returns are cut by `_lora_offsets`, not by running numel() sums."""
import json
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tools import gen_adapter_arena_golden as GEN

GOLDEN = json.loads((Path(__file__).parent / "golden" / "adapter_arena_layout.json").read_text())


def test_the_fixture_holds_every_variant():
    assert sorted(GOLDEN) == sorted(key for key, _, _ in GEN.cases())


@pytest.mark.parametrize("key,variant,b_std", GEN.cases(), ids=[c[0] for c in GEN.cases()])
def test_builder_reproduces_the_recorded_arena(monkeypatch, key, variant, b_std):
    model = GEN.build(variant, b_std, monkeypatch)
    assert GEN.snapshot(model, variant) == GOLDEN[key]
    # (b) the offsets the node's backward cuts by are the parameters' places in the arena, one per parameter, inside the arena
    assert len(model._lora_offsets) == len(model._lora_params) > 0
    for (lo, n), p in zip(model._lora_offsets, model._lora_params):
        assert lo == GEN.offset_of(model, p) and n == p.numel() and 0 <= lo and lo + n <= model.lora_flat.numel()
    if variant == "pixart/lora":
        from simpletuner_amd.pixart.transformer import HP
        H, hd = model.H, model.hd
        pad = torch.zeros(H, HP, dtype=torch.bool); pad[:, hd:] = True
        pad, seen = pad.reshape(-1), {"A": 0, "B": 0}
        for name, p in model.named_parameters():
            if ".lora_A." in name and p.shape[1] == H * HP:
                assert not p[:, pad].any() and p[:, ~pad].abs().min() > 0; seen["A"] += 1
            if ".lora_B." in name and p.shape[0] == H * HP:
                assert not p[pad].any() and (b_std == 0 or p[~pad].abs().min() > 0); seen["B"] += 1
        assert seen == {"A": 2 * len(model.blocks), "B": 6 * len(model.blocks)}          # to_out.0 of attn1 / attn2; to_q, to_k, to_v of both


def test_node_backward_cuts_an_arena_with_a_gap_by_its_offsets():
    """an odd-sized entry, then an 8-aligned one: elements [15, 16) belong to nobody, and running numel() sums would hand the later entries shifted data"""
    from simpletuner_amd.engine import AdapterArena, node_backward
    model = torch.nn.Module()
    arena = AdapterArena(model, "cpu")
    slots = [arena.add("a.weight", (3, 5)), arena.add("b.weight", (4, 2), align=8), arena.add("c.weight", (7,)), arena.add("d.weight", (2, 3), align=8)]
    assert [(s.lo, s.hi) for s in slots] == [(0, 15), (16, 24), (24, 31), (32, 38)]
    arena.build(0)
    assert model.lora_flat.numel() == model.lora_grad_flat.numel() == 40 and model._lora_offsets == [(0, 15), (16, 8), (24, 7), (32, 6)]
    assert [n for n, _ in model.named_parameters()] == ["a.weight", "b.weight", "c.weight", "d.weight"]
    model.grad_sync = None
    model.lora_grad_flat.fill_(-1.0)                       # what the gaps hold must reach nobody

    def backward(ectx, dout):
        assert ectx == "kept" and dout == "dout"
        for k, s in enumerate(slots):
            s.g.fill_(float(k + 1))

    model._engine_backward = backward
    fctx = SimpleNamespace(model=model, ectx="kept")
    grads = node_backward(fctx, False, "dout")
    assert fctx.ectx is None and len(grads) == 4
    flat = model._last_grad_flat
    assert flat.data_ptr() != model.lora_grad_flat.data_ptr() and torch.equal(flat, model.lora_grad_flat)
    for k, (g, p, (lo, n)) in enumerate(zip(grads, model._lora_params, model._lora_offsets)):
        assert g.shape == p.shape and torch.equal(g, torch.full_like(p, float(k + 1)))
        assert g.data_ptr() == flat.data_ptr() + lo * flat.element_size() and g._base is flat

"""8-bit block-wise AdamW (`ao-adamw8bit`), host side: the codebooks, the segment table, the registry entry, the refusals and the state-dict round trip.  No GPU."""
from __future__ import annotations

import types

import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from simpletuner_amd.training.optimizer import OPTIMIZER_CHOICE, St355AdamW8bit, optimizer_settings
from tests import adamw8bit_ref as R

SIZES = (4096, 3072, 4104, 8192, 64)      # eligible, below 4096, not a multiple of 256, eligible, tiny


def arena_params(dtype=torch.float32, device="cpu", seed=0):
    flat = (0.05 * torch.randn(sum(SIZES), generator=torch.Generator().manual_seed(seed))).to(dtype).to(device)
    return flat, [torch.nn.Parameter(t) for t in flat.split(list(SIZES))]


@pytest.mark.parametrize("which, per_decade", [(0, [2 ** i for i in range(7)]), (1, [2 ** (i + 1) for i in range(7)])])
def test_codebooks(which, per_decade):
    cb, ref = ops.adamw8bit_codebooks()[which], R.codebooks()[which]
    assert cb.dtype == torch.float32 and cb.numel() == 256 and bool((cb[1:] > cb[:-1]).all())
    assert torch.equal(cb.double(), ref)                                   # the product's table is the recipe's, bit for bit
    assert cb[-1] == 1.0 and int((cb == 0).sum()) == 1
    pos = cb[(cb > 0) & (cb < 1)].double()
    counts = [int(((pos > 10.0 ** (i - 7)) & (pos < 10.0 ** (i - 6))).sum()) for i in range(7)]
    assert counts == per_decade
    if which == 0:
        assert torch.equal(cb[:127], -cb[128:255].flip(0)) and cb[127] == 0
    pts = ops.adamw8bit_books()[512 + 256 * which:][:255].double()        # decision points: never above the exact midpoint, and the next fp32 is
    mid = (ref[:-1] + ref[1:]) / 2
    assert bool((pts <= mid).all()) and bool((torch.nextafter(pts.float(), torch.tensor(float("inf"))).double() > mid).all())


def test_segment_table():
    _, ps = arena_params()
    plan = ops.Adamw8bitPlan([sum(SIZES[:i]) for i in range(len(SIZES))], list(SIZES), "cpu")
    rec = plan.host.view(-1, 8).tolist()
    assert [r[2] for r in rec] == [int(R.eligible(n)) for n in SIZES] == [1, 0, 0, 1, 0]
    codes = scales = plain = items = 0
    for (start, count, kind, co, so, po, first, n_items), n in zip(rec, SIZES):
        assert (count, first, n_items) == (n, items, -(-n // 256))
        if kind:
            assert count % 256 == 0 and (co, so) == (codes, scales)        # whole blocks inside one tensor; codes and scales packed tensor after tensor
            codes, scales = codes + n, scales + n // 256
        else:
            assert po == plain and po % 4 == 0
            plain += -(-n // 4) * 4
        items += n_items
    assert (plan.n_codes, plan.n_scales, plan.n_plain, plan.n_items) == (codes, scales, plain, items) == (12288, 48, 7240, 78)
    with pytest.raises(St355Error, match="overlaps"):
        ops.Adamw8bitPlan([0, 10], [4096, 64], "cpu")


def test_registry():
    e = OPTIMIZER_CHOICE["ao-adamw8bit"]
    assert e["class"] is St355AdamW8bit and e["precision"] == "any" and e["gradient_precision"] == "bf16"
    assert e["default_settings"] == {"betas": (0.9, 0.999), "weight_decay": 1e-2, "eps": 1e-6}
    cfg = types.SimpleNamespace(optimizer_config="eps=1e-7,weight_decay=0.0", optimizer_beta1=None, optimizer_beta2=None)
    assert optimizer_settings("ao-adamw8bit", cfg) == {"betas": (0.9, 0.999), "weight_decay": 0.0, "eps": 1e-7}
    assert not {"ao-adamw4bit", "ao-adamfp8", "ao-adamwfp8"} & set(OPTIMIZER_CHOICE)
    assert St355AdamW8bit.fuses_ema is False


@pytest.mark.parametrize("kw, text", [(dict(amsgrad=True), "amsgrad=True"), (dict(bf16_stochastic_round=True), "bf16_stochastic_round=True"),
                                      (dict(block_size=128), "block_size=128")])
def test_constructor_refusals(kw, text):
    with pytest.raises(NotImplementedError, match=f"ao-adamw8bit: {text}"):
        St355AdamW8bit(arena_params()[1], **kw)


def test_refuses_scattered_parameters_and_cpu_arena():
    ps = [torch.nn.Parameter(torch.zeros(4096)), torch.nn.Parameter(torch.zeros(64))]
    opt = St355AdamW8bit(ps)
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(NotImplementedError, match="one contiguous run"):
        opt.step()
    flat, ps = arena_params()
    opt = St355AdamW8bit(ps)
    gflat = torch.zeros_like(flat)
    for p, g in zip(ps, gflat.split(list(SIZES))):
        p.grad = g
    with pytest.raises(St355Error, match="pflat: expected a device tensor"):     # a precondition, by name, before the library is even loaded
        opt.step()


def test_trainer_refuses_the_other_torchao_names():
    from simpletuner_amd.training.trainer import Trainer
    comp = types.SimpleNamespace(trainable_parameters=lambda: arena_params()[1])
    plugin = types.SimpleNamespace(get_trained_component=lambda: comp, accelerator=None)
    for name in ("ao-adamw4bit", "ao-adamfp8", "ao-adamwfp8"):
        with pytest.raises(NotImplementedError, match=f"optimizer '{name}' is not built"):
            Trainer(types.SimpleNamespace(optimizer=name), plugin)


def test_state_dict_round_trip():
    _, ps = arena_params()
    a = St355AdamW8bit(ps, lr=2e-3)
    st = a._group_flat(0, a.param_groups[0])
    gen = torch.Generator().manual_seed(1)
    for k in ("m_codes", "v_codes"):
        st[k].copy_(torch.randint(0, 256, st[k].shape, generator=gen, dtype=torch.uint8))
    for k in ("m_scale", "v_scale", "m_plain", "v_plain"):
        st[k].copy_(torch.rand(st[k].shape, generator=gen))
    st["step"] = 7
    st["step_t"].fill_(7.0)
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg_codes", "exp_avg_scale", "exp_avg_sq_codes", "exp_avg_sq_scale"}
    assert set(sd["state"][1]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["state"][0]["exp_avg_codes"].dtype == torch.uint8 and sd["state"][0]["exp_avg_scale"].shape == (16,)
    b = St355AdamW8bit(arena_params(seed=3)[1])
    b.load_state_dict(sd)
    sb = b._flat[0]
    for k in ("m_codes", "v_codes", "m_scale", "v_scale", "m_plain", "v_plain"):
        assert sb[k].dtype == st[k].dtype and torch.equal(sb[k], st[k]), k
    assert sb["step"] == 7 and float(b.state[b.param_groups[0]["params"][3]]["step"]) == 7.0 and b.param_groups[0]["lr"] == 2e-3

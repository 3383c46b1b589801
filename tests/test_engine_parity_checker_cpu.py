"""The slab checker proves its power: three modelled host-sequencing defects, each injected by wrapping one emulated wrapper through monkeypatch, each run
twice on the SD3.5 full fine-tune of the bf16 case table (3 blocks, dual attention on 0 and 1, q/k RMSNorm weights, B 2, 16x24 latents, text 33):

  * at bf16 under the PRESENT criterion — tests/test_sd3_host_sequencing_cpu.py::test_full_finetune_gradients_of_every_parameter_match_the_oracle, its
    constants quoted in `present_criterion` below — which must PASS (that is the gap);
  * in wide arithmetic under the slab rule of tests/engine_parity.py, which must FAIL on the slab concerned (and only where the defect can reach).

Plus the slab splitter, the pooling of small slabs, the bf16 ulp, and an all-zero reference slab held by the floors rather than by a division."""
import math

import pytest
import torch

from tests import engine_parity as EP
from tests import parity_utils as PU
from tests import test_engine_algebra_cpu as ALG
from tests import test_sd3_host_sequencing_cpu as S3
from tests import wide_arith as W

F32, F64 = torch.float32, torch.float64
CASE = (3, 2, 16, 24, 33, True)               # layers, B, lat_h, lat_w, S_txt, sd35: a row of the present test's table


def present_criterion(model, out, loss, d):
    """tests/test_sd3_host_sequencing_cpu.py:104-119, constants as stated there: prediction rel-L2 < 2e-2, |loss - ref| < 2e-3 * max(1, ref); per tensor, a reference
    gradient norm below 1e-3 * gmax only has to "stay small" (< 3e-3 * gmax), every other tensor rel-L2 < 6e-2 and cosine > 0.998.  Returns the failures."""
    o_out, o_loss, P, _ = S3._oracle_side(model, d, True)
    bad = []
    if not (PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())):
        bad.append("prediction / loss")
    gmax = max(v.grad.norm().item() for k, v in P.items() if k != "pos_embed.pos_embed")
    skipped = []
    for name, p in model.named_parameters():
        ref = P[name].grad
        if ref.norm().item() < 1e-3 * gmax:
            skipped.append(name)
            if not p.grad.float().norm().item() < 3e-3 * gmax:
                bad.append(name)
            continue
        if not (PU.rel_l2(p.grad, ref) < 6e-2 and PU.cos_sim(p.grad, ref) > 0.998):
            bad.append(name)
    return bad, skipped


# ---- the defects: each wraps ONE emulated wrapper of simpletuner_amd.ops after the emulator is installed ----
# SD3.5, 3 blocks, the backward's calls of ops.ln_modulate_bwd_stats in order (sd3/transformer.py, host-sequenced block backward): block 2 (last, single attention)
# #0 MLP / #1 attention, image / #2 attention, text; block 1 (dual) #3 MLP image / #4 MLP text / #5 attention image (d shift_msa, d scale_msa; dres = the image
# stream's residual) / #6 attn2 / #7 attention text; block 0: #8 ...
CALL = 5
SHIFT_SLABS = ("transformer_blocks.1.norm1.linear.weight[0/9]", "transformer_blocks.1.norm1.linear.bias[0/9]")
SMALL_TENSOR = "transformer_blocks.0.attn.norm_added_q.weight"          # under the present "small stays small" rule (|ref| = 3.4e-4 vs gmax 1.26)


def _nth_call(monkeypatch, name, n, before=None, after=None):
    from simpletuner_amd import ops
    real, count = getattr(ops, name), [0]

    def wrapped(*a, **k):
        i, count[0] = count[0], count[0] + 1
        if i == n and before is not None:
            a, k = before(list(a), dict(k))
        r = real(*a, **k)
        if i == n and after is not None:
            after(a, k, r)
        return r
    monkeypatch.setattr(ops, name, wrapped)
    return count


def shift_gradient_scaled(monkeypatch, model):
    """one modulation slab's shift gradient x 1.01 in one block (d_shift is the 5th positional operand)"""
    return _nth_call(monkeypatch, "ln_modulate_bwd_stats", CALL, after=lambda a, k, r: a[4].mul_(1.01))


def residual_scaled(monkeypatch, model):
    """the residual (dres) contribution of one block x 0.999"""
    def before(a, k):
        k["dres"] = (k["dres"].float() * 0.999).to(k["dres"].dtype)
        return a, k
    return _nth_call(monkeypatch, "ln_modulate_bwd_stats", CALL, before=before)


def small_tensor_zeroed(monkeypatch, model):
    """the gradient of one tensor under the present skip replaced by zeros: whatever the q/k RMSNorm backward writes into that tensor's gradient view is dropped"""
    from simpletuner_amd import ops
    blk = model.blocks[0]
    ptrs = {v.data_ptr() for views in model._grad_views for (owner, attr, v) in views if owner is blk and attr == "g_norm_added_q"}
    assert len(ptrs) == 2                     # one view per gradient arena
    real, hits = ops.qk_norm_rope_bwd_wgrad, [0]

    def wrapped(*a, **k):
        r = real(*a, **k)
        for t in list(a) + list(k.values()):
            if torch.is_tensor(t) and t.data_ptr() in ptrs and t.numel() == blk.norm_added_q.numel():
                t.zero_(); hits[0] += 1
        return r
    monkeypatch.setattr(ops, "qk_norm_rope_bwd_wgrad", wrapped)
    return hits


def _run(monkeypatch, defect, wide):
    layers, B, lat_h, lat_w, S_txt, sd35 = CASE
    if wide:
        W.install(monkeypatch)
    model = S3._model(monkeypatch, layers, sd35)
    model.enable_full_finetune()
    counter = defect(monkeypatch, model) if defect is not None else None
    d = S3._inputs(B, lat_h, lat_w, S_txt)
    if wide:
        d = ALG._wide(d)
        out, loss, eng = ALG._sd3_engine(model, d)
        assert counter is None or counter[0] > (CALL if defect is not small_tensor_zeroed else 0)          # the defect really was injected
        o64, l64, g64 = ALG._sd3_oracle(model, d, F64)
        o32, l32, g32 = ALG._sd3_oracle(model, d, F32)
        return EP.check_wide("defect", eng, g64, g32, model.D, {"prediction": (out, o64, o32), "loss": (loss, l64, l32)})
    out, loss = S3._hip_side(model, d)
    assert counter is None or counter[0] > (CALL if defect is not small_tensor_zeroed else 0)
    return present_criterion(model, out, loss, d)


def _block(name):
    return EP.block_of(name)


def test_without_a_defect_both_criteria_pass(monkeypatch):
    bad, skipped = _run(monkeypatch, None, wide=False)
    assert not bad and SMALL_TENSOR in skipped and len(skipped) == 9          # 9 of 126 tensors are under the skip at this shape
    monkeypatch.undo()
    rep = _run(monkeypatch, None, wide=True)
    assert not rep.over() and rep.worst().ratio < 0.5
    assert {r.name for r in rep.rows} >= set(SHIFT_SLABS) | {SMALL_TENSOR}


def test_a_shift_gradient_off_by_one_percent_passes_today_and_fails_on_its_slab(monkeypatch):
    bad, _ = _run(monkeypatch, shift_gradient_scaled, wide=False)
    assert not bad, bad
    monkeypatch.undo()
    rep = _run(monkeypatch, shift_gradient_scaled, wide=True)
    over = {r.name: r for r in rep.over()}
    assert set(SHIFT_SLABS) <= set(over), sorted(over)
    for s in SHIFT_SLABS:                                      # ... by the size of the defect: 1 % of the slab against an allowance of ~1e-6 of it
        assert 0.009 < over[s].err / over[s].ref < 0.011 and over[s].ratio > 1e3, over[s]
    # d(modulation rows) also feeds the timestep / pooled-text embedders below the modulation Linear: the defect may show there, and nowhere else
    assert all(n in SHIFT_SLABS or _block(n) == "trunk" for n in over), sorted(over)
    assert sorted(rep.rows, key=lambda r: -r.ratio)[0].name in SHIFT_SLABS


def test_a_zeroed_small_gradient_passes_today_and_fails_on_its_slab(monkeypatch):
    bad, skipped = _run(monkeypatch, small_tensor_zeroed, wide=False)
    assert not bad and SMALL_TENSOR in skipped
    monkeypatch.undo()
    rep = _run(monkeypatch, small_tensor_zeroed, wide=True)
    over = rep.over()
    assert [r.name for r in over] == [SMALL_TENSOR], [r.name for r in over]
    assert over[0].err == pytest.approx(over[0].ref) and over[0].ref > 0 and over[0].ratio > 1e3


def test_a_residual_term_off_by_a_tenth_of_a_percent_passes_today_and_fails_upstream_of_it(monkeypatch):
    bad, _ = _run(monkeypatch, residual_scaled, wide=False)
    assert not bad, bad
    monkeypatch.undo()
    rep = _run(monkeypatch, residual_scaled, wide=True)
    over = {r.name for r in rep.over()}
    # block 1's residual feeds block 0 and everything below it; blocks 1 and 2 and the head were differentiated before the defect
    assert over and all(_block(n) in ("transformer_blocks.0", "trunk") for n in over), sorted(over)
    in_b0 = [r for r in rep.rows if _block(r.name) == "transformer_blocks.0" and r.ref > 0]
    assert sum(r.name in over for r in in_b0) > 0.5 * len(in_b0)
    assert "transformer_blocks.0.attn.to_q.weight" in over and "pos_embed.proj.weight" in over


# ---- the checker's own parts ----
def test_the_slab_splitter():
    D = 8
    t = torch.arange(6 * D * 3.0).view(6 * D, 3)
    s = EP.split_slabs("m.weight", t, D)
    assert [n for n, _ in s] == [f"m.weight[{i}/6]" for i in range(6)] and all(torch.equal(x, t[i * D:(i + 1) * D]) for i, (_, x) in enumerate(s))
    assert torch.equal(torch.cat([x for _, x in s]), t)                                # a partition: nothing dropped, nothing twice
    assert [n for n, _ in EP.split_slabs("b", torch.zeros(3 * D), D)] == ["b[0/3]", "b[1/3]", "b[2/3]"]          # biases too
    assert [n for n, _ in EP.split_slabs("w", torch.zeros(D, 4 * D), D)] == ["w"]     # k = 1: one slab (the trailing dimension does not split)
    assert [n for n, _ in EP.split_slabs("w", torch.zeros(D + 4, D), D)] == ["w"]     # not a multiple of the width
    assert [n for n, _ in EP.split_slabs("A", torch.zeros(4, D), D)] == ["A"]         # a rank-4 factor
    assert [n for n, _ in EP.split_slabs("s", torch.zeros(()), D)] == ["s"]


def test_an_all_zero_reference_slab_is_held_by_the_floors():
    D = 4
    g = torch.Generator().manual_seed(0)
    ref = {"a.weight": torch.randn(2 * D, D, generator=g, dtype=F64), "dead.weight": torch.zeros(D, D, dtype=F64)}
    ref32 = {k: v.float() for k, v in ref.items()}
    gmax = ref["a.weight"].norm().item()
    floor = EP.ABS_FLOOR * gmax / math.sqrt(3)
    ok = EP.check_wide("zero", {"a.weight": ref["a.weight"].float(), "dead.weight": torch.zeros(D, D)}, ref, ref32, D)
    assert len(ok.rows) == 3 and not ok.over()
    dead = next(r for r in ok.rows if r.name == "dead.weight")
    assert dead.ref == 0 and dead.noise == 0 and dead.allow == pytest.approx(floor) and dead.ratio == 0 and math.isfinite(dead.ratio)
    # the engine writing roundoff-sized values where the truth is zero passes; anything visible does not; a missing gradient counts as zeros
    tiny = EP.check_wide("zero", {"a.weight": ref["a.weight"].float(), "dead.weight": torch.full((D, D), 0.1 * floor / D)}, ref, ref32, D)
    assert not tiny.over()
    loud = EP.check_wide("zero", {"a.weight": ref["a.weight"].float(), "dead.weight": torch.full((D, D), 1e-4 * gmax)}, ref, ref32, D)
    assert [r.name for r in loud.over()] == ["dead.weight"]
    with pytest.raises(AssertionError, match="dead.weight"):
        loud.assert_ok()
    none = EP.check_wide("zero", {"a.weight": None, "dead.weight": None}, ref, ref32, D)
    assert [r.name for r in none.over()] == ["a.weight[0/2]", "a.weight[1/2]"]
    with pytest.raises(AssertionError, match="no gradient entry"):
        EP.check_wide("zero", {"a.weight": ref["a.weight"]}, ref, ref32, D)


def test_the_allowance_is_measured_on_the_reference_side_alone():
    D = 4
    ref = {"w": torch.ones(D, D, dtype=F64)}
    r32 = {"w": torch.ones(D, D) * (1 + 2.0 ** -20)}
    noise = (r32["w"].double() - ref["w"]).norm().item()
    a = EP.check_wide("x", {"w": torch.ones(D, D)}, ref, r32, D).rows[0]
    b = EP.check_wide("x", {"w": torch.ones(D, D) * 1.5}, ref, r32, D).rows[0]
    assert a.allow == b.allow == pytest.approx(16 * noise + 1e-6 * ref["w"].norm().item() + 1e-7 * ref["w"].norm().item())
    assert a.err == 0 and b.err == pytest.approx(0.5 * 4) and b.ratio > 1


def test_families_blocks_and_the_bf16_ulp():
    fam = EP.family
    assert fam("transformer_blocks.1.norm1.linear.weight[3/9]") == "modulation weight" and fam("transformer_blocks.0.norm1_context.linear.bias[0/6]") == "modulation bias"
    assert fam("transformer_blocks.0.attn.norm_added_q.weight") == "q/k norm weight" and fam("single_transformer_blocks.1.attn.norm_k.weight") == "q/k norm weight"
    assert fam("transformer_blocks.0.attn.to_q.lora_A.default.weight") == "adapter A" and fam("x.lora_B.default.weight[1/4]") == "adapter B"
    assert fam("transformer_blocks.0.ff.net.2.bias") == "bias" and fam("transformer_blocks.0.ff.net.2.weight") == "weight" and fam("prediction") == "prediction"
    assert EP.block_of("single_transformer_blocks.11.proj_out.weight") == "single_transformer_blocks.11" and EP.block_of("time_text_embed.timestep_embedder.linear_1.bias") == "trunk"
    for x in (1.0, 1.5, 0.3, 3e-5, 700.0):
        b = torch.tensor(x).to(torch.bfloat16)
        nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
        assert EP.ulp_bf16(x) == (nxt.float() - b.float()).item(), x
    assert EP.ulp_bf16(0.0) > 0


def test_small_slabs_pool_per_block_and_kind_until_they_reach_1024_elements():
    mk = lambda n: torch.zeros(n)
    slabs = [("blocks.0.a.bias", mk(512)), ("blocks.0.w.weight", torch.zeros(64, 64)), ("blocks.0.b.bias", mk(512)), ("blocks.0.c.bias", mk(128)),
             ("blocks.1.a.bias", mk(128)), ("blocks.0.norm_q.weight", mk(64))]
    pools = dict(EP.pool_small(slabs))
    assert pools["blocks.0.w.weight"] == ["blocks.0.w.weight"]                       # big enough: on its own
    assert ["blocks.0.a.bias", "blocks.0.b.bias"] in pools.values()                   # closed at 1024
    assert ["blocks.0.c.bias"] in pools.values() and ["blocks.1.a.bias"] in pools.values() and ["blocks.0.norm_q.weight"] in pools.values()      # the remainders, never across block or kind
    assert sorted(n for v in pools.values() for n in v) == sorted(n for n, _ in slabs)


def test_the_device_rule_on_synthetic_gradients():
    g = torch.Generator().manual_seed(1)
    ref = {"blocks.0.w.weight": torch.randn(64, 64, generator=g, dtype=F64)}
    e1 = 2e-2 * torch.randn(64, 64, generator=g, dtype=F64)
    e2 = 2e-2 * torch.randn(64, 64, generator=g, dtype=F64)
    emu = {"blocks.0.w.weight": ref["blocks.0.w.weight"] + e1}
    same = EP.check_device("d", {"blocks.0.w.weight": ref["blocks.0.w.weight"] + e2}, emu, ref, 0)          # an independent draw of the same noise
    assert not same.over() and 0.8 < same.rows[0].err / same.rows[0].noise < 1.25
    big = EP.check_device("d", {"blocks.0.w.weight": ref["blocks.0.w.weight"] + 5 * e2}, emu, ref, 0)
    assert len(big.over()) == 1
    r = same.rows[0]
    assert r.allow == pytest.approx(3 * e1.norm().item() + 0.5 * EP.ulp_bf16(ref["blocks.0.w.weight"].abs().max().item()) * 64)

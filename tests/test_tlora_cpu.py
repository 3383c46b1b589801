"""T-LoRA (`lora_type=lycoris`, `"algo": "tlora"`): the rank rule, the mask stand-in, the SD3 engine on the stand-ins against an fp64 autograd oracle with the explicit
per-sample mask, the plugin and the trainer.  The kernel itself: tests/test_tlora_gpu.py."""
import json
import os
from decimal import Decimal, getcontext
from types import SimpleNamespace

import pytest
import torch

from oracle import sd3 as OS
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests import tlora_ref as TR

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------
# (1) the rank table
# ------------------------------------------------------------------------------------------------
def test_the_documented_alpha_one_rows_are_known_answers():
    """documentation/experimental/T_LORA.md, the alpha = 1 table (R = 64, Rmin = 1): t = 0 / 250 / 500 / 750 / 999 -> 64 / 48 / 32 / 16 / 1"""
    from simpletuner_amd.engine import TLora, tlora_active_rank
    for t, want in ((0, 64), (250, 48), (500, 32), (750, 16), (999, 1)):
        assert tlora_active_rank(t, 1000, 64, 1, 1.0) == want
    st = TLora(64, 1, 1.0, 1000, "cpu")
    assert st.table.dtype == torch.int32 and st.table.shape == (1001,)
    assert [int(st.table[t]) for t in (0, 250, 500, 750, 999)] == [64, 48, 32, 16, 1]


@pytest.mark.parametrize("R,Rmin,alpha", [(64, 1, 1.0), (64, 1, 2.0), (64, 1, 0.5), (16, 4, 1.0), (128, 1, 3.0), (4, 1, 0.5)])
def test_end_points_and_monotonicity(R, Rmin, alpha):
    from simpletuner_amd.engine import TLora
    ranks = TLora(R, Rmin, alpha, 1000, "cpu").ranks
    assert len(ranks) == 1001 and ranks[1000] == Rmin and ranks[0] == R
    assert all(a >= b for a, b in zip(ranks, ranks[1:])) and all(Rmin <= r <= R for r in ranks)


def test_min_rank_equal_to_the_rank_keeps_every_column():
    from simpletuner_amd.engine import TLora
    assert set(TLora(16, 16, 1.0, 1000, "cpu").ranks) == {16}
    assert set(TLora(16, 16, 0.5, 1000, "cpu").ranks) == {16}


def test_alpha_two_and_one_half_follow_the_formula_not_the_documented_tables():
    """alpha = 2 against exact rational arithmetic, alpha = 1/2 against an exact integer square-root comparison and against 50-digit decimals; where the float
    expression sits within an ulp of an integer the exact value may differ, so such timesteps are held to the float rule itself (evaluated here, in the
    documented order) and counted.  The documentation's own alpha = 2 table does not follow its formula: t = 250 gives 36, the table says 60."""
    from simpletuner_amd.engine import tlora_active_rank
    assert tlora_active_rank(250, 1000, 64, 1, 2.0) == 36 == TR.active_rank_exact(250, 1000, 64, 1, 2) != 60
    getcontext().prec = 50
    for alpha, exact_alpha in ((2.0, 2), (0.5, 0.5)):
        off = 0
        for t in range(1001):
            got = tlora_active_rank(t, 1000, 64, 1, alpha)
            assert got == min(64, int(((1000 - t) / 1000) ** alpha * 63) + 1)          # the rule in Python floats, in this order
            exact = TR.active_rank_exact(t, 1000, 64, 1, exact_alpha)
            if alpha == 0.5:
                dec = min(64, int((Decimal(1000 - t) / Decimal(1000)).sqrt() * 63) + 1)
                assert dec == exact
            off += got != exact
            assert abs(got - exact) <= 1
        assert off <= 2, (alpha, off)          # (float rounding at an exact integer: at most a boundary or two over the thousand steps)


def test_the_state_refuses_settings_outside_their_ranges():
    from simpletuner_amd.engine import TLora
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match=r"tlora_min_rank must lie in \[1, linear_dim = 16\]"):
            TLora(16, bad, 1.0, 1000, "cpu")
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="tlora_alpha must be positive"):
            TLora(16, 1, bad, 1000, "cpu")


# ------------------------------------------------------------------------------------------------
# (2) the mask stand-in against the dense restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", TR.MASK_LAYOUTS)
@pytest.mark.parametrize("G,rank", TR.MASK_SHAPES)
def test_the_stand_in_equals_the_dense_restatement_bit_for_bit(G, rank, layout):
    dead = 0
    for rows in TR.MASK_ROWS:
        for ts in TR.MASK_TIMESTEPS:
            for dt in TR.MASK_DTYPES:
                _, n = TR.check_mask_case(TR.tlora_mask, "cpu", layout, rows, G, rank, ts, dt, seed=rows + G)
                dead += n
    assert dead > 0


def test_timesteps_are_truncated_as_their_dtype_holds_them():
    """int(0.99) = 0, int(499.5) = 499 and int(999.9) = 999 in fp32; bf16 holds 499.5 as 500 and 999.9 as 1000; values outside [0, T] read the table's ends"""
    f = torch.tensor([0.0, 0.99, 499.5, 999.9, 1000.0, -3.0, 2000.0])
    assert TR.timestep_index(f, 1000).tolist() == [0, 0, 499, 999, 1000, 0, 1000]
    assert TR.timestep_index(f.to(BF16), 1000).tolist() == [0, 0, 500, 1000, 1000, 0, 1000]
    assert TR.timestep_index(torch.tensor([0, 499, 1000, -1, 5000]), 1000).tolist() == [0, 499, 1000, 0, 1000]


# ------------------------------------------------------------------------------------------------
# (3) the SD3 engine on the stand-ins
# ------------------------------------------------------------------------------------------------
R, T_TRAIN = 16, 1000
BOTH = ["Attention", "FeedForward"]


def _perturb(model, seed=3, std=0.02):
    """move `up` off zero, so that the adapter does something and `down` gets a gradient"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(TR.UP):
                p.copy_((std * torch.randn(p.shape, generator=g)).to(p.device))


def _model(monkeypatch, layers, sd35=False, classes=BOTH, rank=R, min_rank=1, alpha=1.0, linear_alpha=None, multiplier=1, perturb=True):
    TR.install(monkeypatch)
    model = SH._model(monkeypatch, layers, sd35)
    TR.install(monkeypatch)                       # (SH._model installs the plain emulator again)
    model.add_tlora_adapter(classes=classes, linear_dim=rank, linear_alpha=rank if linear_alpha is None else linear_alpha, multiplier=multiplier, min_rank=min_rank,
                            alpha=alpha, num_train_timesteps=T_TRAIN, seed=7)
    model.prepare_for_training()
    model.train()
    if perturb:
        _perturb(model)
    return model


def _ranks(model, t):
    st = model.lora_tlora
    return [TR.active_rank(int(v), st.T, st.R, st.Rmin, st.alpha) for v in t.tolist()]


def _oracle(monkeypatch, model, d, ranks, scale=1.0, tread=None):
    """fp64 autograd through the oracle with the explicit per-sample mask (ranks None: the same adapter without any mask)"""
    facs = {k: (a.requires_grad_(True), b.requires_grad_(True)) for k, (a, b) in TR.factors_of(model).items()}
    monkeypatch.setattr(OS, "linear", TR.masked_linear(facs, scale, ranks))
    P = {k: v.detach().cpu().to(F64) for k, v in model.named_parameters() if ".lora_" not in k}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().cpu().to(F64)
    kw = {} if tread is None else dict(tread=tread)
    out = OS.sd3_forward(P, SH._ocfg(model), d["lat"].to(F64), d["prompt"].to(F64), d["pooled"].to(F64), d["t"].to(F64), **kw)
    loss = ((out - d["target"].to(F64)) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), facs


def _ref_grad(name, facs):
    return facs[name[:-len(TR.DOWN)]][0].grad if name.endswith(TR.DOWN) else facs[name[:-len(TR.UP)]][1].grad


def _worst(model, facs):
    worst = 0.0
    for name, p in model.named_parameters():
        if ".lora_" in name:
            ref = _ref_grad(name, facs)
            if float(ref.abs().max()) == 0.0:          # (the context_pre_only block's text queries reach nothing)
                assert float(p.grad.abs().max()) == 0.0, name
                continue
            worst = max(worst, PU.rel_l2(p.grad.cpu(), ref.float()))
    return worst


PLANS = {"plain": (False, None, None), "per-block": (True, None, None), "segmented": (True, 2, None), "stride": (True, 2, 3)}


def _plan(model, ckpt):
    model.gradient_checkpointing, model.gradient_checkpointing_interval, model.gradient_checkpointing_segment_stride = PLANS[ckpt]


def _inputs3(seed=5):
    """batch 3 with three timesteps, so that three different ranks are live in one step"""
    d = SH._inputs(3, 16, 24, 33, seed=seed)
    d["t"] = torch.tensor([100.0, 500.5, 900.0])
    return d


@pytest.mark.parametrize("ckpt", list(PLANS))
@pytest.mark.parametrize("classes", [["Attention"], ["FeedForward"], BOTH], ids=["attention", "feed-forward", "both"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_engine_with_tlora_matches_autograd_through_the_masked_oracle(monkeypatch, sd35, classes, ckpt):
    """the tolerances of tests/test_lora_dropout_cpu.py::test_sd3_engine_with_lora_dropout_matches_autograd_through_the_masked_oracle (prediction rel-L2 2e-2, loss
    2e-3, every adapter gradient rel-L2 5e-2): a per-sample truncated LoRA is a standard LoRA of lower rank, nothing wider is justified"""
    model = _model(monkeypatch, 4 if ckpt == "stride" else 3, sd35, classes)
    _plan(model, ckpt)
    d = _inputs3()
    ranks = _ranks(model, d["t"])
    assert ranks == [14, 8, 2]
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, facs = _oracle(monkeypatch, model, d, ranks)
    assert PU.rel_l2(out, o_out.float()) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, facs)
    assert worst < 5e-2, worst
    names = [n for n, _ in model.named_parameters() if n.endswith(TR.DOWN)]
    assert ("Attention" in classes) == any(".attn.add_q_proj" in n for n in names) == any(".attn.to_out.0" in n for n in names)
    assert ("FeedForward" in classes) == any(".ff.net.0.proj" in n for n in names) == any(".ff_context.net.2" in n for n in names)
    assert (not sd35) or ("Attention" not in classes) or any(".attn2.to_out.0" in n for n in names)
    # ... and a reference that forgets the mask is far outside the same tolerances
    _, _, nfacs = _oracle(monkeypatch, model, d, None)
    plain = _worst(model, nfacs)
    assert plain > 0.25, plain
    print(f"[emu] sd3{'.5' if sd35 else ''} T-LoRA {classes} {ckpt}: worst adapter gradient rel-L2 {worst:.3e} with the mask, {plain:.3e} against a reference without it")


@pytest.mark.parametrize("ckpt", ["plain", "per-block"])          # (under routing every plan is the per-block one, as in the reference)
def test_sd3_engine_with_tlora_under_tread(monkeypatch, ckpt):
    from simpletuner_amd.training.tread import ReplayRouter
    d = SH._inputs(2, 16, 16, 24)
    d["t"] = torch.tensor([250.0, 875.0])
    B, Si = 2, 64
    g = torch.Generator().manual_seed(11)
    perm = torch.stack([torch.randperm(Si, generator=g) for _ in range(B)])
    Kk = Si - int(round(Si * 0.5))
    rec = {"mask": torch.ones(B, Si, dtype=torch.bool).scatter_(1, perm[:, :Kk], False), "ids_keep": perm[:, :Kk], "ids_mask": perm[:, Kk:], "ids_shuffle": perm,
           "ids_restore": torch.argsort(perm, dim=1)}
    routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]
    model = _model(monkeypatch, 4, True)
    model.set_router(ReplayRouter([rec]), routes)
    _plan(model, ckpt)
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, facs = _oracle(monkeypatch, model, d, _ranks(model, d["t"]), tread={"routes": routes, "mask_infos": [rec]})
    assert PU.rel_l2(out, o_out.float()) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    assert _worst(model, facs) < 5e-2


def test_layersync_trains_beside_the_mask(monkeypatch):
    """the regulariser's tap and its injected gradient run on a T-LoRA component: the step's adapter gradients are finite and the extra output is there"""
    model = _model(monkeypatch, 3)
    model.set_layersync(0, 1)
    d = _inputs3()
    out = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    assert len(out) == 2
    (((out[0].float() - d["target"].float()) ** 2).mean() - 0.1 * out[1].float().mean()).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in model.named_parameters() if ".lora_" in n)


def test_gradient_accumulation_adds_the_second_micro_step(monkeypatch):
    model = _model(monkeypatch, 3, True)
    d1, d2 = _inputs3(5), _inputs3(6)
    d2["t"] = torch.tensor([700.0, 10.0, 333.0])
    grads = lambda: {n: p.grad.clone() for n, p in model.named_parameters() if ".lora_" in n}
    SH._hip_side(model, d2)
    g2 = grads()
    for p in model.parameters():
        p.grad = None
    SH._hip_side(model, d1)
    g1 = grads()
    model.accumulate_lora_grads = True
    for p in model.parameters():
        p.grad = None                            # the engine's flat gradient arena keeps the first micro-step's values
    SH._hip_side(model, d2)
    got = grads()
    for n in got:
        assert (got[n] - (g1[n] + g2[n])).abs().max().item() <= 1e-6 * max((g1[n].abs() + g2[n].abs()).max().item(), 1e-30), n


# ------------------------------------------------------------------------------------------------
# (4) the exact-zero property
# ------------------------------------------------------------------------------------------------
def test_inactive_ranks_get_exactly_zero_gradient(monkeypatch):
    """batch 1 at t = 999 (Rmin = 1, R = 16): one rank is live, so rows 1 .. 15 of every d down and columns 1 .. 15 of every d up are exactly 0.0 — the masked T and
    U carry exact zeros into both products — and row / column 0 is not"""
    model = _model(monkeypatch, 3, True)
    d = SH._inputs(1, 16, 24, 33)
    d["t"] = torch.tensor([999.0])
    assert _ranks(model, d["t"]) == [1]
    SH._hip_side(model, d)
    dead = "transformer_blocks.2.attn.add_q_proj."          # the context_pre_only block drops its text rows: the text queries reach nothing
    seen = 0
    for n, p in model.named_parameters():
        if n.endswith(TR.DOWN):
            assert bool((p.grad[1:] == 0).all()), n
            assert n.startswith(dead) or float(p.grad[0].abs().max()) > 0, n
            seen += 1
        if n.endswith(TR.UP):
            assert bool((p.grad[:, 1:] == 0).all()), n
            assert n.startswith(dead) or float(p.grad[:, 0].abs().max()) > 0, n
            seen += 1
    assert seen == 2 * sum(len(g.targets) for g in model.lora_groups) > 0


# ------------------------------------------------------------------------------------------------
# (5) equivalences
# ------------------------------------------------------------------------------------------------
def _run(m, d):
    return m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()


def test_min_rank_equal_to_the_rank_is_the_unmasked_adapter_bit_for_bit(monkeypatch):
    from simpletuner_amd import ops
    d = _inputs3()
    model = _model(monkeypatch, 3, True, min_rank=R)
    calls = []
    real = ops.tlora_mask
    monkeypatch.setattr(ops, "tlora_mask", lambda t, *a, **k: (calls.append(1), real(t, *a, **k))[1])
    out, loss = SH._hip_side(model, d)
    assert calls                                             # every sample at the full rank: the mask still runs (no branch on device data)
    g = model.lora_grad_flat.clone()
    n_calls = len(calls)
    model2 = _model(monkeypatch, 3, True, min_rank=R)
    monkeypatch.setattr(ops, "tlora_mask", lambda t, *a, **k: t)          # the mask call stubbed to a no-op
    out2, loss2 = SH._hip_side(model2, d)
    assert torch.equal(out, out2) and torch.equal(loss, loss2) and torch.equal(g, model2.lora_grad_flat) and bool(g.abs().max() > 0)
    # ... while with Rmin = 1 the stubbed run is another computation
    model3 = _model(monkeypatch, 3, True)
    monkeypatch.setattr(ops, "tlora_mask", real)
    out3, _ = SH._hip_side(model3, d)
    assert not torch.equal(out3, out2) and n_calls > 0


def test_the_fresh_adapter_is_the_base_model_and_eval_applies_the_mask_and_the_validation_strength(monkeypatch):
    from simpletuner_amd import ops
    from simpletuner_amd.sd3 import transformer as T
    d = _inputs3()
    model = _model(monkeypatch, 3, True, perturb=False)
    for n, p in model.named_parameters():
        if n.endswith(TR.UP):
            assert bool((p == 0).all())
        if n.endswith(TR.DOWN):
            assert 0 < p.abs().max().item() <= 1.0 / p.shape[1] ** 0.5          # U(-1 / sqrt(in), 1 / sqrt(in))
    a = _run(model, d)
    monkeypatch.setattr(T, "_BLOCK_ABI", False)          # the base model, host-sequenced like T-LoRA
    base = SH._model(monkeypatch, 3, True)
    TR.install(monkeypatch)
    monkeypatch.setattr(T, "_BLOCK_ABI", False)
    with torch.no_grad():
        assert torch.equal(a, _run(base, d))
    # eval() and no-grad forwards apply the mask, scaled by the validation strength there
    _perturb(model)
    train_out = _run(model, d)
    assert not torch.equal(train_out, a)
    model.eval()
    with torch.no_grad():
        assert torch.equal(_run(model, d), train_out)                      # strength 1: the training forward's computation, mask included
        real = ops.tlora_mask
        monkeypatch.setattr(ops, "tlora_mask", lambda t, *a_, **k: t)
        assert not torch.equal(_run(model, d), train_out)                  # ... which a forward without the mask is not
        monkeypatch.setattr(ops, "tlora_mask", real)
        model.lokr_validation_strength = 0.5
        half = _run(model, d)
        assert not torch.equal(half, train_out) and all(g.scale == 0.5 * g.tlora_scale for g in model.lora_groups)
        model.lokr_validation_strength = 0.0
        assert torch.equal(_run(model, d), a)
    model.train()
    assert torch.equal(_run(model, d), train_out)                          # training forwards never take the validation strength


def test_multiplier_and_alpha_go_through_int_and_scale_the_adapter(monkeypatch):
    model = _model(monkeypatch, 2, linear_alpha=8.9, multiplier=2.7)
    assert model.tlora_multiplier == 2 and model.tlora_linear_alpha == 8 and all(g.tlora_scale == 8 / R and g.scale == 2 * 8 / R for g in model.lora_groups)


# ------------------------------------------------------------------------------------------------
# (6) the launch stream of the other adapters
# ------------------------------------------------------------------------------------------------
def test_lokr_and_standard_lora_never_reach_the_mask_and_tlora_leaves_the_block_entries(monkeypatch):
    """on ONE commit: a standard LoRA and a LoKr component issue no `tlora_mask` (and the standard LoRA still goes through the block-level entry points), a T-LoRA
    component issues it and runs host-sequenced.  That those streams — every launch with its operands' dtypes, shapes and strides — equal the parent commit's is
    shown with tools/launch_trace.py over the host-sequencing and LoKr engine tests at both commits (CHANGELOG.md)."""
    from simpletuner_amd import ops
    d = _inputs3()

    def trace(build):
        TR.install(monkeypatch)
        model = SH._model(monkeypatch, 3, True if build != "lora" else False)
        TR.install(monkeypatch)
        names = []
        for nm in ("gemm", "gemm_grouped", "skinny_tn", "skinny_tn_multi", "block_sd3_joint_fwd", "block_sd3_joint_bwd", "tlora_mask", "lokr_fold"):
            fn = getattr(ops, nm)
            monkeypatch.setattr(ops, nm, (lambda f, n: (lambda *a, **k: (names.append(n), f(*a, **k))[1]))(fn, nm))
        if build == "lora":
            model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
        elif build == "lokr":
            model.add_lokr_adapter(factors={"Attention": 2, "FeedForward": 2})
        else:
            model.add_tlora_adapter(linear_dim=16, linear_alpha=16)
        model.prepare_for_training()
        model.train()
        SH._hip_side(model, d)
        return names

    lora, lokr, tl = trace("lora"), trace("lokr"), trace("tlora")
    assert "tlora_mask" not in lora and "block_sd3_joint_fwd" in lora and "block_sd3_joint_bwd" in lora
    assert "tlora_mask" not in lokr and "lokr_fold" in lokr
    assert "tlora_mask" in tl and "block_sd3_joint_fwd" not in tl and "block_sd3_joint_bwd" not in tl
    # two masks per adapter site and step: one on T in the forward, one on U in the backward (block 0 included: its U feeds d down)
    model_sites = 3 * 10 - 2 + 2 * 2          # 3 blocks x (qkv, add_qkv, to_out, to_add_out, ff1, ff2, ffc1, ffc2) less the last block's (to_add_out, ffc1, ffc2) + 2 dual x (qkv2, to_out2)
    assert tl.count("tlora_mask") == 2 * (3 * 8 - 3 + 2 * 2), (tl.count("tlora_mask"), model_sites)


# ------------------------------------------------------------------------------------------------
# (7) the plugin and the trainer
# ------------------------------------------------------------------------------------------------
LYCORIS = {"algo": "tlora", "multiplier": 1.0, "linear_dim": 8, "linear_alpha": 8, "tlora_min_rank": 2, "tlora_alpha": 1.0,
           "apply_preset": {"target_module": ["Attention", "FeedForward"]}}


def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, lycoris=LYCORIS, tmp_path=None, lora_type="lycoris", **cfg_kw):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    TR.install(monkeypatch)
    cfg = default_config(model_family="sd3", train_batch_size=2, seed=3, lora_rank=8, **cfg_kw)
    cfg.lora_type = lora_type
    if tmp_path is not None:          # through the file, as `lycoris_config` names it
        path = tmp_path / "lycoris_config.json"
        path.write_text(json.dumps(lycoris))
        cfg.lycoris_config = str(path)
    else:
        cfg.lycoris_config = dict(lycoris)
    plugin = SD3(cfg, _acc())
    plugin.load_model(**SH._arch(2))
    return plugin


def _trainer(monkeypatch, lycoris=LYCORIS, lora_type="lycoris", **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, lycoris=lycoris, lora_type=lora_type, learning_rate=1e-3, **cfg_kw)
    if lora_type == "standard":
        plugin.config.lora_init_b_std = 0.02
    plugin.add_lora_adapter()
    if lora_type == "lycoris" and lycoris.get("algo") == "tlora":
        _perturb(plugin.get_trained_component())
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


@pytest.mark.parametrize("through", ["dict", "file"])
def test_the_plugin_builds_tlora_pairs_from_the_lycoris_config(monkeypatch, tmp_path, through):
    plugin = _plugin(monkeypatch, tmp_path=tmp_path if through == "file" else None, validation_lycoris_strength=0.5)
    plugin.add_lora_adapter()
    comp = plugin.get_trained_component()
    names = [n for n, p in comp.named_parameters() if p.requires_grad]
    assert names and all(n.endswith((TR.DOWN, TR.UP)) for n in names)
    assert "transformer_blocks.0.attn.to_q.lora_down.weight" in names and "transformer_blocks.0.ff.net.0.proj.lora_up.weight" in names
    assert not any("lora_A" in n or "lora_B" in n or ".lokr_" in n for n, _ in comp.named_parameters())
    st = comp.lora_tlora
    assert (st.R, st.Rmin, st.alpha, st.T) == (8, 2, 1.0, 1000) and not comp.lora_lokr and comp.lokr_validation_strength == 0.5
    assert dict(comp.named_parameters())["transformer_blocks.0.ff.net.2.lora_down.weight"].shape == (8, 512)
    assert plugin.lycoris["algo"] == "tlora" and plugin.lycoris["multiplier"] == 1 and isinstance(plugin.lycoris["multiplier"], int)
    # defaults of the mask settings, and the class selection
    p2 = _plugin(monkeypatch, lycoris={"algo": "tlora", "linear_dim": 4, "apply_preset": {"target_module": ["Attention"]}})
    p2.add_lora_adapter()
    c2 = p2.get_trained_component()
    assert (c2.lora_tlora.Rmin, c2.lora_tlora.alpha, c2.tlora_linear_alpha) == (1, 1.0, 1) and not any(".ff" in n for n, _ in c2.named_parameters() if ".lora_" in n)


def test_lokr_still_parses_as_before(monkeypatch):
    plugin = _plugin(monkeypatch, lycoris={"algo": "lokr", "multiplier": 1.0, "linear_dim": 10000, "linear_alpha": 1, "factor": 2})
    plugin.add_lora_adapter()
    comp = plugin.get_trained_component()
    assert comp.lora_lokr and comp.lora_tlora is None and any(n.endswith(".lokr_w1") for n, _ in comp.named_parameters())


def test_refusals_by_their_exact_texts(monkeypatch):
    def err(exc, **kw):
        with pytest.raises(exc) as ei:
            _plugin(monkeypatch, **kw).add_lora_adapter()
        return str(ei.value)

    assert err(ValueError, lycoris=dict(LYCORIS, tlora_min_rank=0)) == \
        'lycoris_config tlora_min_rank=0: must lie in [1, linear_dim = 8]; set "tlora_min_rank" inside that range'
    assert err(ValueError, lycoris=dict(LYCORIS, tlora_min_rank=9)) == \
        'lycoris_config tlora_min_rank=9: must lie in [1, linear_dim = 8]; set "tlora_min_rank" inside that range'
    assert err(ValueError, lycoris=dict(LYCORIS, tlora_alpha=0)) == 'lycoris_config tlora_alpha=0.0: must be positive; set "tlora_alpha" above 0'
    assert err(ValueError, lycoris=dict(LYCORIS, tlora_alpha=-2)) == 'lycoris_config tlora_alpha=-2.0: must be positive; set "tlora_alpha" above 0'
    mixed = dict(LYCORIS, apply_preset={"target_module": ["Attention", "FeedForward"], "module_algo_map": {"FeedForward": {"algo": "lokr", "factor": 2}}})
    assert err(NotImplementedError, lycoris=mixed) == ("lycoris_config apply_preset.module_algo_map.FeedForward.algo=lokr beside algo=tlora: one component that mixes lokr "
                                                       "and tlora adapters is not built on the st355 path; set the same algo for every module class")
    mixed2 = {"algo": "lokr", "factor": 2, "linear_dim": 10000, "apply_preset": {"target_module": ["Attention"], "module_algo_map": {"Attention": {"algo": "tlora"}}}}
    assert err(NotImplementedError, lycoris=mixed2) == ("lycoris_config apply_preset.module_algo_map.Attention.algo=tlora beside algo=lokr: one component that mixes lokr "
                                                        "and tlora adapters is not built on the st355 path; set the same algo for every module class")
    assert err(NotImplementedError, lycoris=dict(LYCORIS, linear_dim=256, tlora_min_rank=1)) == \
        'lycoris_config linear_dim=256: the rank-space kernels of the st355 path take 1 <= linear_dim <= 128; set "linear_dim" inside that range'
    per_class = dict(LYCORIS, apply_preset={"target_module": ["Attention"], "module_algo_map": {"Attention": {"linear_dim": 4}}})
    assert err(NotImplementedError, lycoris=per_class) == ("lycoris_config apply_preset.module_algo_map.Attention.linear_dim=4: a per-class linear_dim is not built on the "
                                                           'st355 path (one rank table per component); set "linear_dim" at the top level only')
    # what was refused before keeps its text
    assert err(NotImplementedError, lycoris=dict(LYCORIS, algo="loha")) == ("lycoris_config algo=loha: not built on the st355 path (built: algo=lokr with both factors "
                                                                            'full, merged-weight forward); set "algo": "lokr"')
    assert err(NotImplementedError, lycoris=dict(LYCORIS, rank_dropout=0.2)).startswith("lycoris_config rank_dropout=0.2: not built on the st355 path")
    assert err(NotImplementedError, lycoris=dict(LYCORIS, apply_preset={"target_module": ["Attention", "ResnetBlock2D"]})).startswith(
        "lycoris_config apply_preset.target_module entry 'ResnetBlock2D': not built for Stable Diffusion 3.x on the st355 path")
    assert err(ValueError, internal_guidance_enabled=True) == "Internal Guidance requires standard PEFT LoRA or full-model training so its auxiliary head is optimized and saved."
    assert err(ValueError, nextlat_enabled=True, nextlat_weight=0.3) == "NextLat requires standard PEFT LoRA or full-model training so its predictor is optimized and saved."


def test_tokenwise_timesteps_scheduled_sampling_and_xm_are_refused_by_name(monkeypatch):
    from simpletuner_amd.training.trainer import Trainer
    model = _model(monkeypatch, 2)
    d = SH._inputs(2, 16, 24, 33)
    with pytest.raises(NotImplementedError) as ei:
        model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"][:, None].expand(2, 96).contiguous(),
              return_dict=False)
    assert str(ei.value) == ("lycoris tlora with tokenwise timesteps: the active rank is a function of ONE timestep per sample (the reference's int(t) over a [B, S] "
                             "list fails too); not built on the st355 path")
    for kw, flag in ((dict(scheduled_sampling_max_step_offset=3), "scheduled_sampling_max_step_offset=3"), (dict(scheduled_sampling_reflexflow=True), "scheduled_sampling_reflexflow")):
        plugin = _plugin(monkeypatch, **kw)
        plugin.add_lora_adapter()
        plugin.post_model_load_setup()
        with pytest.raises(NotImplementedError) as ei:
            Trainer(plugin.config, plugin, plugin.accelerator)
        assert str(ei.value) == (f"{flag} with lycoris algo=tlora: the reference's rollout forwards run without the timestep rank mask, which every forward of a T-LoRA "
                                 "component of the st355 path applies; not built")
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    plugin.xm_config = SimpleNamespace(enabled=True)
    with pytest.raises(NotImplementedError) as ei:
        Trainer(plugin.config, plugin, plugin.accelerator)
    assert str(ei.value) == ("lycoris algo=tlora with XM noise candidates: the candidate forwards would need the rank mask of the candidate's own timestep; not built on "
                             "the st355 path")


@pytest.mark.parametrize("opt", ["st355-adamw", "adamw_bf16", "optimi-lion", "soap", "torch-adafactor"])          # (muon: refused for the SD3 family whatever the adapter, below)
def test_two_train_steps_move_the_loss_and_the_pairs(monkeypatch, opt):
    extra = {}
    if opt == "soap":          # (soap preconditions the rank side only: rank <= max_precond_dim < in_features; its stand-ins are its own module's)
        from tests import soap_ref
        soap_ref.install(monkeypatch)
        extra = dict(optimizer_config="max_precond_dim=8")
    plugin, trainer, batch = _trainer(monkeypatch, optimizer=opt, **extra)
    comp = plugin.get_trained_component()
    before = {n: p.detach().clone() for n, p in comp.named_parameters() if ".lora_" in n}
    l1 = trainer.train_step(dict(batch))
    if opt == "soap":
        trainer.train_step(dict(batch))          # (SOAP's first step only starts its preconditioner: the values move from the second on)
    l2 = trainer.train_step(dict(batch))
    assert torch.isfinite(l1) and torch.isfinite(l2) and l1.item() != l2.item()
    moved = {n for n, p in comp.named_parameters() if ".lora_" in n and not torch.equal(p.detach(), before[n])}
    assert any(n.endswith(TR.DOWN) for n in moved) and any(n.endswith(TR.UP) for n in moved) and any(".ff." in n for n in moved)


def test_muon_keeps_its_refusal_for_the_family(monkeypatch):
    with pytest.raises(ValueError, match="Optimizer 'muon' is not supported by model family sd3"):
        _trainer(monkeypatch, optimizer="muon")


def test_ema_follows_the_pairs(monkeypatch):
    plugin, trainer, batch = _trainer(monkeypatch, use_ema=True)
    assert trainer.ema_model is not None
    l1 = trainer.train_step(dict(batch))
    l2 = trainer.train_step(dict(batch))
    assert torch.isfinite(l1) and torch.isfinite(l2) and l1.item() != l2.item()


def test_adapter_file_round_trip_and_the_mismatch_errors(monkeypatch, tmp_path):
    from safetensors.torch import load_file, save_file
    plugin, trainer, batch = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    comp = plugin.get_trained_component()
    path = plugin.save_lora_weights(str(tmp_path / "a"))
    flat = load_file(path)
    n_targets = sum(len(g.targets) for g in comp.lora_groups)
    assert len(flat) == 3 * n_targets and all(k.startswith("lycoris_transformer_blocks_") for k in flat)
    named = dict(comp.named_parameters())
    assert torch.equal(flat["lycoris_transformer_blocks_0_attn_to_out_0.lora_down.weight"], named["transformer_blocks.0.attn.to_out.0.lora_down.weight"].detach())
    assert torch.equal(flat["lycoris_transformer_blocks_1_ff_net_2.lora_up.weight"], named["transformer_blocks.1.ff.net.2.lora_up.weight"].detach())
    al = flat["lycoris_transformer_blocks_0_ff_net_0_proj.alpha"]
    assert al.dim() == 0 and al.dtype == F32 and al.item() == 8.0
    want = comp.lora_flat.clone()
    plugin2, _, _ = _trainer(monkeypatch)
    assert not torch.equal(plugin2.get_trained_component().lora_flat, want)
    plugin2.load_lora_weights(input_dir=str(tmp_path / "a"))
    assert torch.equal(plugin2.get_trained_component().lora_flat, want)
    # strict: a missing tensor, a tensor too many, another rank's shape, another alpha — each names the lycoris_config key to change
    k0 = "lycoris_transformer_blocks_1_attn_to_q.lora_up.weight"
    for name, mutate, exc, pat in (("b", lambda f: f.pop(k0), KeyError, "LyCORIS checkpoint is missing 1 adapter tensors"),
                                   ("c", lambda f: f.update({"lycoris_other.lora_down.weight": torch.zeros(2, 2)}), KeyError, "holds 1 tensors the adapter has no place for"),
                                   ("d", lambda f: f.update({k0: torch.zeros(128, 4)}), ValueError,
                                    r"has shape \(128, 4\), the adapter's is \(128, 8\): the lycoris_config linear_dim must match"),
                                   ("e", lambda f: f.update({k0[:-len(".lora_up.weight")] + ".alpha": torch.tensor(4.0)}), ValueError,
                                    "alpha 4.0 .* differs from the configured linear_alpha 8.0; set linear_alpha to match the file")):
        f = dict(flat)
        mutate(f)
        os.makedirs(tmp_path / name)
        save_file(f, str(tmp_path / name / plugin.LORA_WEIGHT_NAME))
        with pytest.raises(exc, match=pat):
            plugin2.load_lora_weights(input_dir=str(tmp_path / name))
    # a LoKr file into a T-LoRA adapter and the reverse; a T-LoRA file into a standard adapter and the reverse
    lokr, _, _ = _trainer(monkeypatch, lycoris={"algo": "lokr", "multiplier": 1.0, "linear_dim": 10000, "linear_alpha": 1, "factor": 2})
    lokr.save_lora_weights(str(tmp_path / "k"))
    with pytest.raises(ValueError) as ei:
        plugin2.load_lora_weights(input_dir=str(tmp_path / "k"))
    assert str(ei.value) == ('lycoris_config algo=tlora is set but the checkpoint carries LyCORIS LoKr factors (lokr_w1 / lokr_w2): set "algo": "lokr" in the '
                             "lycoris_config to load it")
    with pytest.raises(ValueError) as ei:
        lokr.load_lora_weights(input_dir=str(tmp_path / "a"))
    assert str(ei.value) == ("lycoris_config algo=lokr is set but the checkpoint carries LyCORIS low-rank pairs (lora_down / lora_up: a T-LoRA file): set "
                             '"algo": "tlora" in the lycoris_config to load it')
    plain, _, _ = _trainer(monkeypatch, lora_type="standard")
    with pytest.raises(ValueError, match=r"carries LyCORIS low-rank pairs .* but the adapter was built as a standard LoRA: set --lora_type=lycoris"):
        plain.load_lora_weights(input_dir=str(tmp_path / "a"))
    plain.save_lora_weights(str(tmp_path / "p"))
    with pytest.raises(ValueError, match="lycoris_config algo=tlora is set but the checkpoint carries no LyCORIS low-rank pairs"):
        plugin2.load_lora_weights(input_dir=str(tmp_path / "p"))
    plugin.config.lora_format = "comfyui"
    with pytest.raises(NotImplementedError, match="lora_type=lycoris with lora_format=comfyui: the ComfyUI export of a T-LoRA adapter"):
        plugin.save_lora_weights(str(tmp_path / "q"))


def test_resume_equals_the_uninterrupted_run_and_holds_the_mask_settings(monkeypatch, tmp_path):
    plugin, trainer, batch = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    trainer.save_state(str(tmp_path / "ck"))
    assert json.load(open(tmp_path / "ck" / "training_state.json"))["tlora"] == {"min_rank": 2, "alpha": 1.0, "num_train_timesteps": 1000}
    want = trainer.train_step(dict(batch))
    want_w = plugin.get_trained_component().lora_flat.clone()
    plugin2, trainer2, _ = _trainer(monkeypatch)
    trainer2.load_state(str(tmp_path / "ck"))
    got = trainer2.train_step(dict(batch))
    assert got.item() == want.item() and torch.equal(plugin2.get_trained_component().lora_flat, want_w)
    _, trainer3, _ = _trainer(monkeypatch, lycoris=dict(LYCORIS, tlora_min_rank=4, tlora_alpha=2.0))
    with pytest.raises(ValueError, match=r"other T-LoRA mask settings \(min_rank: checkpoint 2, configured 4; alpha: checkpoint 1.0, configured 2.0\): set tlora_min_rank / tlora_alpha"):
        trainer3.load_state(str(tmp_path / "ck"))

"""LyCORIS LoKr (`lora_type=lycoris`, `algo: lokr`) on the CPU: the factor rule, the fp64 restatement against autograd through torch.kron, `init_lokr_norm` against
the reference's function (recorded), the stand-ins inside the kernels' derived bounds, the SD3 engine on the kernel-contract emulator against autograd through the
oracle with the merged-weight linear, the arena lay-out, the plugin / trainer surface, the adapter files and every refusal.  The LyCORIS package is not installed:
the rule is pinned to the issue's statement as tests/lokr_ref.py restates it, not to executed LyCORIS code."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from oracle import sd3 as OS
from tests import lokr_bounds as LB
from tests import lokr_ref as LR
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.lokr_checks import ROWS, W1_SIDES, check_dw1, check_dw2, check_fold, check_mix, run_fold

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAND = SimpleNamespace(**LR.STAND_INS)


# ------------------------------------------------------------------------------------------------
# (a) the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,factor,want", [(1536, 10, (8, 192)), (1536, 4, (4, 384)), (6144, 4, (4, 1536)), (1536, 16, (16, 96)), (3072, 10, (8, 384)),
                                             (64, 10, (8, 8)), (24, 10, (4, 6)), (56, 16, (7, 8)), (1536, -1, (32, 48)), (2432, 10, (8, 304))])
def test_factorization_table(dim, factor, want):
    from simpletuner_amd.engine import lokr_factorization
    assert lokr_factorization(dim, factor) == want


def _problem(M=37, ol=3, ok=8, im=2, in_=5, seed=0, bias=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    N, K = ol * ok, im * in_
    return dict(x=rn(M, K), W=rn(N, K) / K ** 0.5, b=rn(N) if bias else None, w1=rn(ol, im), w2=0.3 * rn(ok, in_), s=0.7, dy=rn(M, N))


@pytest.mark.parametrize("bias", [True, False])
def test_restatement_equals_autograd_through_kron(bias):
    p = _problem(bias=bias)
    leaves = {k: p[k].clone().requires_grad_(True) for k in ("x", "w1", "w2")}
    y = LR.lokr_autograd(leaves["x"], p["W"], p["b"], leaves["w1"], leaves["w2"], p["s"])
    y.backward(p["dy"])
    y64, dx, dw1, dw2 = LR.lokr64(p["x"], p["W"], p["b"], p["w1"], p["w2"], p["s"], p["dy"])
    for name, got, want in (("y", y64, y.detach()), ("dx", dx, leaves["x"].grad), ("dw1", dw1, leaves["w1"].grad), ("dw2", dw2, leaves["w2"].grad)):
        err = (got - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-13, (name, err)          # fp64 rounding of sums of at most a few hundred terms
    # the element rule: dW[i ok + k, j in + l] = s w1[i, j] w2[k, l]
    dW = LR.merged(torch.zeros_like(p["W"]), p["w1"], p["w2"], p["s"])
    assert dW[1 * 8 + 3, 1 * 5 + 2].item() == pytest.approx(p["s"] * p["w1"][1, 1].item() * p["w2"][3, 2].item(), rel=1e-15)


def test_init_lokr_norm_equals_the_reference_function_under_the_same_seed():
    """tests/golden/lokr_vectors.pt: `approximate_normal_tensor` of the reference executed on the CPU (tools/gen_lokr_golden.py)"""
    from simpletuner_amd.engine import lokr_init_norm
    cases = torch.load(os.path.join(ROOT, "tests", "golden", "lokr_vectors.pt"))["init_lokr_norm"]
    assert len(cases) == 2
    for c in cases:
        w2 = torch.zeros_like(c["w2"])
        torch.manual_seed(c["seed"])
        lokr_init_norm(c["weight"], w2, c["scale"])
        assert torch.equal(w2, c["w2"])


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins inside the kernels' bounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ol,im,ok,in_", [(2, 2, 8, 8), (8, 4, 24, 40), (16, 16, 64, 64)])
def test_stand_ins_are_inside_the_derived_bounds(ol, im, ok, in_, G):
    check_fold(STAND, "cpu", ol, im, ok, in_, G)
    r = run_fold(STAND, "cpu", ol, im, ok, in_, G, 0.0)
    assert torch.equal(r.Wf[0], r.W)                       # s = 0: the identity
    for kind, B, rows in ROWS:
        check_mix(STAND, "cpu", kind, B, rows, ol, im, ok, G)
        for acc in (False, True):
            check_dw2(STAND, "cpu", kind, B, rows, im, ok, in_, acc)
            check_dw1(STAND, "cpu", kind, B, rows, ol, im, ok, G, acc)


def test_the_emulated_gemm_keeps_p_inside_its_bound(monkeypatch):
    ops = LR.install(monkeypatch)
    g = torch.Generator().manual_seed(1)
    M, im, ok, in_ = 37, 4, 24, 64
    x, w2b = torch.randn(M, im * in_, generator=g).to(BF16), (0.05 * torch.randn(ok, in_, generator=g)).to(BF16)
    P = torch.empty(M, im * ok, dtype=BF16)
    ops.gemm(x.view(M * im, in_), w2b, out=P.view(M * im, ok))
    assert LB.inside(P, *LB.p_ref(x, w2b, im))[0]


# ------------------------------------------------------------------------------------------------
# (c) the SD3 engine on the emulator
# ------------------------------------------------------------------------------------------------
FACTORS = {"Attention": 2, "FeedForward": 2}          # D = 128: 2 x 64 on every side


def _perturb(model, seed=3, std=0.02):
    """move w2 off zero, so that the delta is there and dw1 is a gradient of something"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(LR.K2):
                p.copy_((std * torch.randn(p.shape, generator=g)).to(p.device))


def _model(monkeypatch, layers, sd35=False, factors=FACTORS, arch=None, **kw):
    LR.install(monkeypatch)
    if arch is None:
        model = SH._model(monkeypatch, layers, sd35)
    else:
        from simpletuner_amd.sd3 import transformer as T
        model = T.SD3Transformer2DModel(device="cpu", **arch)
        model.init_synthetic(5)
    LR.install(monkeypatch)                       # (SH._model installs the plain emulator again)
    model.add_lokr_adapter(factors=dict(factors), **kw)
    model.prepare_for_training()
    model.train()
    return model


def _oracle(monkeypatch, model, d, s=1.0, lokr=True, tread=None):
    facs = {k: (a.requires_grad_(True), b.requires_grad_(True)) for k, (a, b) in LR.factors_of(model).items()}
    monkeypatch.setattr(OS, "linear", LR.lokr_linear(facs if lokr else {}, s))
    P = {k: v.detach().float() for k, v in model.named_parameters() if ".lokr_" not in k}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    kw = {} if tread is None else dict(tread=tread)
    out = OS.sd3_forward(P, SH._ocfg(model), d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], **kw)
    loss = ((out - d["target"].float()) ** 2).mean()
    if lokr:
        loss.backward()
    return out.detach(), loss.detach(), facs


def _ref_grad(name, facs):
    key, which = name.rsplit(".lokr_", 1)
    return facs[key][0 if which == "w1" else 1].grad


def _worst(model, facs):
    worst = {"w1": 0.0, "w2": 0.0}
    for name, p in model.named_parameters():
        if ".lokr_" in name:
            which = name.rsplit(".lokr_", 1)[1]
            worst[which] = max(worst[which], PU.rel_l2(p.grad, _ref_grad(name, facs)))
    return worst


PLANS = {"plain": (False, None, None), "per-block": (True, None, None), "segmented": (True, 2, None), "stride": (True, 2, 3)}


def _plan(model, ckpt):
    model.gradient_checkpointing, model.gradient_checkpointing_interval, model.gradient_checkpointing_segment_stride = PLANS[ckpt]


@pytest.mark.parametrize("ckpt", list(PLANS))
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_engine_with_lokr_matches_autograd_through_the_merged_weight_oracle(monkeypatch, sd35, ckpt):
    """the tolerances of tests/test_dora_cpu.py for the same comparison (prediction rel-L2 2e-2, loss 2e-3, every gradient rel-L2 5e-2).  The oracle multiplies with
    the merged weight ROUNDED to bf16, as the rule defines the forward, so the fold's rounding is no error of the comparison; the gradient operands the engine
    recomputes for the FeedForward sites (the modulated LayerNorm rows, gelu of the kept bf16 pre-activation) carry one bf16 rounding each, as every activation does."""
    model = _model(monkeypatch, 4, sd35)
    _perturb(model)
    _plan(model, ckpt)
    d = SH._inputs(2, 16, 24, 33)
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, facs = _oracle(monkeypatch, model, d)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, facs)
    assert max(worst.values()) < 5e-2, worst
    names = [n for n, _ in model.named_parameters() if n.endswith(LR.K1)]
    assert any(".ff.net.0.proj" in n for n in names) and any(".ff_context.net.2" in n for n in names) and any(".attn.add_q_proj" in n for n in names)
    assert (not sd35) or any(".attn2.to_out.0" in n for n in names)
    dead = "transformer_blocks.3.attn.add_q_proj."          # the context_pre_only block drops its text rows: the text queries reach nothing
    assert all((p.grad.abs().max() > 0) != n.startswith(dead) for n, p in model.named_parameters() if ".lokr_" in n)
    # ... and a reference without the delta is far outside the same tolerances
    monkeypatch.undo()
    LR.install(monkeypatch)
    n_out, _, _ = _oracle(monkeypatch, model, d, lokr=False)
    assert PU.rel_l2(out, n_out) > 2e-2
    print(f"[emu] sd3{'.5' if sd35 else ''} LoKr {ckpt}: worst gradient rel-L2 {worst}")


def test_sd3_engine_with_lokr_at_eight_heads_and_factor_eight(monkeypatch):
    """D = 512: factor 8 gives w1 [8, 8] and w2 [64, 64] on the attention sites, [256, 64] / [64, 256] on the feed-forward ones"""
    model = _model(monkeypatch, 2, factors={"Attention": 8, "FeedForward": 8}, arch=SH._arch(2, heads=8))
    assert model.blocks[0].qkv.lora.shapes[0] == (8, 64, 8, 64) and model.blocks[0].ff1.lora.shapes[0] == (8, 256, 8, 64)
    _perturb(model, std=0.01)
    d = SH._inputs(1, 16, 16, 20)
    d["prompt"] = d["prompt"][..., :128]
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, facs = _oracle(monkeypatch, model, d)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, facs)
    assert max(worst.values()) < 5e-2, worst


@pytest.mark.parametrize("ckpt", ["plain", "per-block"])          # (under routing every plan is the per-block one, as in the reference)
def test_sd3_engine_with_lokr_under_tread(monkeypatch, ckpt):
    from simpletuner_amd.training.tread import ReplayRouter
    d = SH._inputs(2, 16, 16, 24)
    B, Si = 2, 64
    g = torch.Generator().manual_seed(11)
    perm = torch.stack([torch.randperm(Si, generator=g) for _ in range(B)])
    Kk = Si - int(round(Si * 0.5))
    rec = {"mask": torch.ones(B, Si, dtype=torch.bool).scatter_(1, perm[:, :Kk], False), "ids_keep": perm[:, :Kk], "ids_mask": perm[:, Kk:], "ids_shuffle": perm,
           "ids_restore": torch.argsort(perm, dim=1)}
    routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]
    model = _model(monkeypatch, 4, True)
    _perturb(model)
    model.set_router(ReplayRouter([rec]), routes)
    _plan(model, ckpt)
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, facs = _oracle(monkeypatch, model, d, tread={"routes": routes, "mask_infos": [rec]})
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, facs)
    assert max(worst.values()) < 5e-2, worst


def test_gradient_accumulation_adds_the_second_micro_step(monkeypatch):
    """each micro-step's gradient holds to the 5e-2 rel-L2 of the single-step test; the triangle inequality then bounds the accumulated sum's error by
    5e-2 (|r1| + |r2|) — NOT by 5e-2 |r1 + r2|: a w1 is as small as 2 x 2 here and the two micro-steps' gradients of one nearly cancel.  The accumulation itself is
    held much tighter: the accumulated arena equals the sum of the two single-step arenas up to the fp32 rounding of the kernels' one add per element."""
    model = _model(monkeypatch, 3, True)
    _perturb(model)
    d1, d2 = SH._inputs(2, 16, 24, 33, seed=5), SH._inputs(2, 16, 24, 33, seed=6)
    lokr = lambda: {n: p.grad.clone() for n, p in model.named_parameters() if ".lokr_" in n}
    SH._hip_side(model, d2)
    g2 = lokr()
    for p in model.parameters():
        p.grad = None
    SH._hip_side(model, d1)
    g1 = lokr()
    model.accumulate_lora_grads = True
    for p in model.parameters():
        p.grad = None                            # the engine's flat gradient arena keeps the first micro-step's values
    SH._hip_side(model, d2)
    got = lokr()
    refs = []
    for d in (d1, d2):
        _, _, facs = _oracle(monkeypatch, model, d)
        refs.append({n: _ref_grad(n, facs) for n in got})
    for n in got:
        assert (got[n] - (g1[n] + g2[n])).abs().max().item() <= 1e-6 * (g1[n].abs() + g2[n].abs()).max().item(), n
        assert (got[n] - (refs[0][n] + refs[1][n])).norm().item() <= 5e-2 * (refs[0][n].norm() + refs[1][n].norm()).item(), n


def test_the_fresh_adapter_is_the_base_model_bit_for_bit_and_the_multiplier_scales_the_delta(monkeypatch):
    d = SH._inputs(2, 16, 24, 33)
    run = lambda m: m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()
    model = _model(monkeypatch, 3, True)
    assert all(bool((p == 0).all()) for n, p in model.named_parameters() if n.endswith(LR.K2))
    for n, p in model.named_parameters():
        if n.endswith(LR.K1):
            assert p.abs().max().item() <= 1.0 / p.shape[1] ** 0.5 and p.abs().max().item() > 0          # U(-1 / sqrt(im), 1 / sqrt(im))
    a = run(model)
    assert all(torch.equal(g.Wf, g.lin.w) and torch.equal(g.WfT, g.lin.w.t()) for g in model.lora_groups)
    from simpletuner_amd.sd3 import transformer as T
    monkeypatch.setattr(T, "_BLOCK_ABI", False)          # the base model, host-sequenced like LoKr
    base = SH._model(monkeypatch, 3, True)
    LR.install(monkeypatch)
    monkeypatch.setattr(T, "_BLOCK_ABI", False)
    with torch.no_grad():
        assert torch.equal(a, run(base))
    # LoKr is part of the weight: eval() and no-grad forwards apply it, scaled by the validation strength there
    _perturb(model)
    model.eval()
    with torch.no_grad():
        full = run(model)
        assert not torch.equal(full, a)
        model.lokr_validation_strength = 0.0
        assert torch.equal(run(model), a)
        assert all(g.s == 0.0 for g in model.lora_groups)


# ------------------------------------------------------------------------------------------------
# (d) the arena
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["none", "layersync"])
def test_parameters_and_gradients_are_one_run_w1_then_w2_in_target_order(monkeypatch, extra):
    from simpletuner_amd.training.optimizer import flat_view
    model = _model(monkeypatch, 3, True)
    if extra == "layersync":
        model.set_layersync(0, 1)
    _perturb(model)
    params = model.trainable_parameters()
    names = {id(p): n for n, p in model.named_parameters()}
    order = [names[id(p)] for p in params]
    assert all(a.endswith(LR.K1) and b == a[:-len(LR.K1)] + LR.K2 for a, b in zip(order[0::2], order[1::2]))
    assert len(order) == 2 * sum(len(g.targets) for g in model.lora_groups) and not any(".lora_" in n for n, _ in model.named_parameters())
    fv = flat_view(params)
    assert fv is not None and fv.data_ptr() == model.lora_flat.data_ptr() and fv.numel() == sum(p.numel() for p in params)
    off = 0
    for p in params:
        assert p.dtype == F32 and p.data_ptr() == model.lora_flat.data_ptr() + 4 * off
        off += p.numel()
    for g in model.lora_groups:
        assert g.w1[0].data_ptr() == model.lora_flat.data_ptr() + 4 * g.flat_lo and g.g1[0].data_ptr() == model.lora_grad_flat.data_ptr() + 4 * g.flat_lo
    d = SH._inputs(2, 16, 24, 33)
    out = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    loss = ((out[0].float() - d["target"].float()) ** 2).mean()
    for extra_out in out[1:]:
        loss = loss + extra_out.float().mean()
    loss.backward()
    gv = flat_view([p.grad for p in params])
    assert gv is not None and gv.numel() == fv.numel()


# ------------------------------------------------------------------------------------------------
# (e) the plugin and the trainer
# ------------------------------------------------------------------------------------------------
LYCORIS = {"algo": "lokr", "multiplier": 1.0, "linear_dim": 10000, "linear_alpha": 1, "factor": 2,
           "apply_preset": {"target_module": ["Attention", "FeedForward"], "module_algo_map": {"Attention": {"factor": 2}, "FeedForward": {"factor": 2}}}}


def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, lycoris=LYCORIS, tmp_path=None, **cfg_kw):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    LR.install(monkeypatch)
    cfg = default_config(model_family="sd3", train_batch_size=2, seed=3, lora_rank=8, **cfg_kw)
    cfg.lora_type = "lycoris"
    if tmp_path is not None:          # through the file, as `lycoris_config` names it
        path = tmp_path / "lycoris_config.json"
        path.write_text(json.dumps(lycoris))
        cfg.lycoris_config = str(path)
    else:
        cfg.lycoris_config = dict(lycoris)
    plugin = SD3(cfg, _acc())
    plugin.load_model(**SH._arch(2))
    return plugin


def _trainer(monkeypatch, lokr=True, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, learning_rate=1e-3, **cfg_kw)
    if not lokr:
        plugin.config.lora_type, plugin.config.lora_init_b_std = "standard", 0.02
    plugin.add_lora_adapter()
    if lokr:
        _perturb(plugin.get_trained_component())
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


def test_the_plugin_under_lora_type_lycoris_registers_lokr_factors_and_no_lora_matrices(monkeypatch, tmp_path):
    """fails without the feature: the flag used to be ignored and a standard LoRA was built"""
    plugin = _plugin(monkeypatch, tmp_path=tmp_path)
    plugin.add_lora_adapter()
    names = [n for n, p in plugin.get_trained_component().named_parameters() if p.requires_grad]
    assert names and all(n.endswith((LR.K1, LR.K2)) for n in names)
    assert "transformer_blocks.0.attn.to_q.lokr_w1" in names and "transformer_blocks.0.ff.net.0.proj.lokr_w2" in names
    assert not any("lora_A" in n or "lora_B" in n for n, _ in plugin.get_trained_component().named_parameters())
    comp = plugin.get_trained_component()
    assert comp.lora_lokr and comp.lokr_multiplier == 1.0 and comp.blocks[0].qkv.lora.shapes == [(2, 64, 2, 64)] * 3
    # per-class factors and the class selection come from the file
    only_attn = dict(LYCORIS, apply_preset={"target_module": ["Attention"]})
    p2 = _plugin(monkeypatch, lycoris=only_attn)
    p2.add_lora_adapter()
    assert not any(".ff" in n for n, p in p2.get_trained_component().named_parameters() if ".lokr_" in n)
    # lora_dropout and use_dora are ignored under lycoris, as in the reference
    p3 = _plugin(monkeypatch, lora_dropout=0.1)
    p3.config.use_dora = True
    p3.add_lora_adapter()
    assert p3.get_trained_component().lora_dropout is None and not p3.get_trained_component().lora_dora


@pytest.mark.parametrize("opt", ["st355-adamw", "optimi-lion"])
def test_one_train_step_moves_w1_and_w2(monkeypatch, opt):
    plugin, trainer, batch = _trainer(monkeypatch, optimizer=opt)
    comp = plugin.get_trained_component()
    before = {n: p.detach().clone() for n, p in comp.named_parameters() if ".lokr_" in n}
    assert before
    trainer.train_step(dict(batch))
    moved = {n for n, p in comp.named_parameters() if ".lokr_" in n and not torch.equal(p.detach(), before[n])}
    dead = "transformer_blocks.1.attn.add_q_proj."          # the context_pre_only block drops its text rows: zero gradient (Lion leaves it, AdamW's decay moves it)
    assert moved >= {n for n in before if not n.startswith(dead)} and any(n.endswith(LR.K1) for n in moved) and any(n.endswith(LR.K2) for n in moved)


def test_validation_lycoris_strength_reaches_the_component(monkeypatch):
    plugin = _plugin(monkeypatch, validation_lycoris_strength=0.5)
    plugin.add_lora_adapter()
    assert plugin.get_trained_component().lokr_validation_strength == 0.5


def test_init_lokr_norm_through_the_plugin(monkeypatch):
    plugin = _plugin(monkeypatch, init_lokr_norm=1e-3)
    plugin.add_lora_adapter()
    comp = plugin.get_trained_component()
    for n, p in comp.named_parameters():
        if n.endswith(LR.K1):
            assert bool((p == 1).all())
        if n.endswith(LR.K2):
            assert p.abs().max().item() > 0
    g = comp.blocks[0].to_out.lora
    W = g.lin.w.float()
    assert g.w2[0].mean().item() == pytest.approx(1e-3 * W.mean().item(), rel=1e-3, abs=1e-9) and g.w2[0].std().item() == pytest.approx(1e-3 * W.std().item(), rel=1e-3)


# ------------------------------------------------------------------------------------------------
# (f) refusals, by name
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_path", ["simpletuner_amd.flux.model.Flux", "simpletuner_amd.pixart.model.PixartSigma", "simpletuner_amd.sdxl.model.SDXL",
                                      "simpletuner_amd.sd1x.model.StableDiffusion1"])
def test_families_without_the_fold_refuse_the_flag_by_name(cls_path):
    import importlib
    mod, cls = cls_path.rsplit(".", 1)
    Plug = getattr(importlib.import_module(mod), cls)
    plug = Plug.__new__(Plug)
    plug.config = SimpleNamespace(model_type="lora", lora_type="lycoris", lycoris_config=dict(LYCORIS), lora_rank=8)
    plug.controlnet, plug.model = None, None
    for call in (plug.lycoris_value, plug.add_lora_adapter):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert str(ei.value) == f"lora_type=lycoris: LyCORIS adapters are not built for {Plug.NAME} on the st355 path (built: SD3); set --lora_type=standard"
    for cfg in (SimpleNamespace(model_type="lora", lora_type="standard"), SimpleNamespace(model_type="lora"), SimpleNamespace(model_type="full", lora_type="lycoris")):
        plug.config = cfg
        assert plug.lycoris_value() is None


REFUSED = [
    (dict(algo="loha"), r"lycoris_config algo=loha: .* set \"algo\": \"lokr\""),
    (dict(linear_dim=16), r"lycoris_config linear_dim=16: transformer_blocks\.0\.attn\.to_q would get a low-rank w2 \(\[64, 64\] needs linear_dim >= 32\).* set \"linear_dim\": 10000"),
    (dict(decompose_both=True), r"lycoris_config decompose_both=true: .* set \"decompose_both\": false"),
    (dict(use_tucker=True), r"lycoris_config use_tucker=true"),
    (dict(use_scalar=True), r"lycoris_config use_scalar=true"),
    (dict(weight_decompose=True), r"lycoris_config weight_decompose=true"),
    (dict(rs_lora=True), r"lycoris_config rs_lora=true"),
    (dict(train_norm=True), r"lycoris_config train_norm=true"),
    (dict(dropout=0.1), r"lycoris_config dropout=0\.1: .* set \"dropout\": 0"),
    (dict(rank_dropout=0.2), r"lycoris_config rank_dropout=0\.2"),
    (dict(module_dropout=0.3), r"lycoris_config module_dropout=0\.3"),
    (dict(bypass_mode=True), r"lycoris_config bypass_mode=true: .* set \"bypass_mode\": false"),
    (dict(apply_preset={"target_module": ["Attention", "ResnetBlock2D"]}), r"lycoris_config apply_preset\.target_module entry 'ResnetBlock2D': .* subset of \['Attention', 'FeedForward'\]"),
    (dict(apply_preset={"target_module": ["Attention"], "module_algo_map": {"Attention": {"factor": 4}}}),
     r"lycoris lokr: factor=4 splits transformer_blocks\.0\.attn\.to_q \[128, 128\] into w2 \[32, 32\]; the gradient route needs ok % 8 == 0 and in % 64 == 0 — choose a factor"),
]


@pytest.mark.parametrize("change,pat", REFUSED, ids=[next(iter(c)) + str(i) for i, (c, _) in enumerate(REFUSED)])
def test_sd3_refuses_what_is_not_built_by_key_and_value(monkeypatch, change, pat):
    plugin = _plugin(monkeypatch, lycoris=dict(LYCORIS, **change))
    with pytest.raises(NotImplementedError, match=pat):
        plugin.add_lora_adapter()


def test_a_w1_side_above_sixteen_is_refused_with_the_factor_to_choose(monkeypatch):
    """D = 512: factor -1 splits the 2048 feed-forward features 32 x 64"""
    with pytest.raises(NotImplementedError, match=r"lycoris lokr: factor=-1 gives transformer_blocks\.0\.ff\.net\.0\.proj a w1 of \[32, 16\]; the kernels take w1 sides "
                                                  r"up to 16 — set factor to a divisor of 2048 and 512 that is at most 16"):
        _model(monkeypatch, 2, factors={"FeedForward": -1}, arch=SH._arch(2, heads=8))


def test_sd3_refuses_the_flag_combinations_by_name(monkeypatch):
    with pytest.raises(NotImplementedError, match="lora_type=lycoris with lora_format=comfyui"):
        _plugin(monkeypatch, lora_format="comfyui").add_lora_adapter()
    with pytest.raises(NotImplementedError, match=r"lora_type=lycoris with init_lora=/some/file\.safetensors"):
        _plugin(monkeypatch, init_lora="/some/file.safetensors").add_lora_adapter()
    # the standard-LoRA-only regularisers: the reference's ValueError, checked first, texts unchanged
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, internal_guidance_enabled=True, lycoris=dict(LYCORIS, algo="loha")).add_lora_adapter()
    assert str(ei.value) == "Internal Guidance requires standard PEFT LoRA or full-model training so its auxiliary head is optimized and saved."
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, lycoris=dict(LYCORIS, algo="loha")).add_lora_adapter()
    assert str(ei.value) == "NextLat requires standard PEFT LoRA or full-model training so its predictor is optimized and saved."
    with pytest.raises(ValueError, match="lora_type=lycoris needs lycoris_config"):
        p = _plugin(monkeypatch)
        p.config.lycoris_config = None
        p.add_lora_adapter()


# ------------------------------------------------------------------------------------------------
# (g) files
# ------------------------------------------------------------------------------------------------
def test_adapter_file_round_trip_and_the_mismatch_errors(monkeypatch, tmp_path):
    from safetensors.torch import load_file, save_file
    plugin, trainer, batch = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    comp = plugin.get_trained_component()
    path = plugin.save_lora_weights(str(tmp_path / "a"))
    flat = load_file(path)
    n_targets = sum(len(g.targets) for g in comp.lora_groups)
    assert len(flat) == 3 * n_targets and all(k.startswith("lycoris_transformer_blocks_") for k in flat)
    assert torch.equal(flat["lycoris_transformer_blocks_0_attn_to_out_0.lokr_w1"], dict(comp.named_parameters())["transformer_blocks.0.attn.to_out.0.lokr_w1"].detach())
    al = flat["lycoris_transformer_blocks_0_ff_net_0_proj.alpha"]
    assert al.dim() == 0 and al.dtype == F32 and al.item() == 10000.0
    want = comp.lora_flat.clone()
    plugin2, _, _ = _trainer(monkeypatch)
    assert not torch.equal(plugin2.get_trained_component().lora_flat, want)
    plugin2.load_lora_weights(input_dir=str(tmp_path / "a"))
    assert torch.equal(plugin2.get_trained_component().lora_flat, want)
    # strict: a missing tensor, a tensor too many, another factor's shape, another linear_dim
    k0 = "lycoris_transformer_blocks_1_attn_to_q.lokr_w2"
    for name, mutate, exc, pat in (("b", lambda f: f.pop(k0), KeyError, "LyCORIS checkpoint is missing 1 adapter tensors"),
                                   ("c", lambda f: f.update({"lycoris_other.lokr_w1": torch.zeros(2, 2)}), KeyError, "holds 1 tensors the adapter has no place for"),
                                   ("d", lambda f: f.update({k0: torch.zeros(32, 32)}), ValueError, r"has shape \(32, 32\), the adapter's is \(64, 64\)"),
                                   ("e", lambda f: f.update({k0[:-len(".lokr_w2")] + ".alpha": torch.tensor(4.0)}), ValueError, "alpha 4.0 .* differs from the configured linear_dim")):
        f = dict(flat)
        mutate(f)
        os.makedirs(tmp_path / name)
        save_file(f, str(tmp_path / name / plugin.LORA_WEIGHT_NAME))
        with pytest.raises(exc, match=pat):
            plugin2.load_lora_weights(input_dir=str(tmp_path / name))
    # a LoKr file into a standard adapter, and the reverse
    plain, _, _ = _trainer(monkeypatch, lokr=False)
    with pytest.raises(ValueError, match=r"carries LyCORIS LoKr factors \(lokr_w1 / lokr_w2\) but the adapter was built as a standard LoRA: set --lora_type=lycoris"):
        plain.load_lora_weights(input_dir=str(tmp_path / "a"))
    plain.save_lora_weights(str(tmp_path / "p"))
    with pytest.raises(ValueError, match="lora_type=lycoris is set but the checkpoint carries no LoKr factors"):
        plugin2.load_lora_weights(input_dir=str(tmp_path / "p"))
    plugin.config.lora_format = "comfyui"
    with pytest.raises(NotImplementedError, match="lora_type=lycoris with lora_format=comfyui"):
        plugin.save_lora_weights(str(tmp_path / "q"))


def test_resume_equals_the_uninterrupted_run(monkeypatch, tmp_path):
    plugin, trainer, batch = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    trainer.save_state(str(tmp_path / "ck"))
    want = trainer.train_step(dict(batch))
    want_w = plugin.get_trained_component().lora_flat.clone()
    plugin2, trainer2, _ = _trainer(monkeypatch)
    trainer2.load_state(str(tmp_path / "ck"))
    got = trainer2.train_step(dict(batch))
    assert got.item() == want.item() and torch.equal(plugin2.get_trained_component().lora_flat, want_w)

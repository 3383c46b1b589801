"""Internal Guidance (helpers/training/internal_guidance.py) on the CPU: the fp64 restatement against the executed reference's golden file, the stand-ins against the
derived bounds, the plugin / trainer / file / sampling surface, and the SD3 engine's host sequencing — where the head's prediction leaves the network's autograd
node and where its gradient enters the hand-written dX chain, under every checkpoint mode — against autograd through the oracle (tests/ops_emulator.py + the
stand-ins of tests/internal_guidance_ref.py)."""
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import internal_guidance_bounds as IB
from tests import internal_guidance_ref as IG
from tests import layersync_ref as LS
from tests import ops_emulator as EMU
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN = Path(__file__).resolve().parent / "golden" / "internal_guidance_vectors.pt"
# the weight of the engine cases: at the reference's default 0.5 on these tiny models the head's share of the adapter gradient sits near the gradient tolerances — a
# dropped or misplaced injection could pass.  8.0 makes the two terms comparable (every case asserts the regulariser's measured share), as LayerSync's lambda = 8
WEIGHT = 8.0
PRE = IG.PREFIX


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=True)


# ------------------------------------------------------------------------------------------------
# (a) the restatement against the executed reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["case", "constant_row", "offset_row"])
def test_restatement_equals_the_executed_reference(golden, case):
    """tokens, prediction, loss, logs and the five gradients of InternalGuidanceRegularizer.compute_loss.  The golden numbers are fp32: a D-term mean and variance, a
    D-term projection, their backward.  The fp64 restatement may differ from them by the reference's own rounding, 5 * D * 2^-24 relative to each tensor's scale,
    times kappa = max(1, max|x| / sqrt(var + eps)) over the rows — the factor by which the fp32 mean's error (u max|x|) enters xhat (1 for ordinary rows, ~50 for
    the row of offset 64, 375 for the constant row with its rstd of 1000)."""
    g, p = golden[case], golden["params"]
    D = g["hidden"].shape[-1]
    x = g["hidden"].double().reshape(-1, D)
    kappa = (x.abs().amax(dim=1) / torch.sqrt(x.var(dim=1, unbiased=False) + 1e-6)).clamp_min(1.0)
    tol, kmax = 5 * D * 2.0 ** -24, kappa.max().item()
    loss, logs, tokens, pred, dh, dgamma, dbeta, dW, db = IG.loss64(g["hidden"], p["gamma"], p["beta"], p["W"], p["b"], g["target"], g["weight"])
    scale_y = g["tokens"].double().abs().max()
    assert ((tokens - g["tokens"].double()).abs().reshape(-1, IG.N) <= tol * kappa[:, None] * scale_y).all()
    assert torch.equal(IG.unpatchify(g["tokens"], 16, *g["target"].shape[2:]), g["prediction"])          # the token layout: (dh, dw, c), SD3's own proj_out order
    assert abs(loss.item() - g["loss"].item()) <= tol * kmax * max(1.0, g["loss"].item())
    for k in ("internal_guidance_loss", "internal_guidance_unweighted_loss"):
        assert abs(logs[k] - g["logs"][k]) <= tol * kmax * max(1.0, g["logs"][k]), k
    assert abs(g["logs"]["internal_guidance_loss"] - g["weight"] * g["logs"]["internal_guidance_unweighted_loss"]) < 1e-6
    ref = g["grad_hidden"].double().reshape(-1, D)
    rows_scale = ref.abs().amax(dim=1, keepdim=True)
    assert ((dh.reshape(-1, D) - ref).abs() <= tol * kappa[:, None] * rows_scale).all()
    for name, mine in (("grad_gamma", dgamma), ("grad_beta", dbeta), ("grad_W", dW), ("grad_b", db)):
        r = g[name].double()
        assert r.abs().max() > 0 and ((mine - r).abs() <= tol * kmax * r.abs().max()).all(), name
    if case == "constant_row":
        b0, r0 = g["row"]
        xh, rs, _ = IG.reference64(g["hidden"], p["gamma"], p["beta"], p["W"], p["b"])
        i = b0 * g["hidden"].shape[1] + r0
        assert xh[i].abs().max() == 0 and abs(rs[i].item() - 1000.0) < 1e-6


def test_patch_shapes_features_defaults_and_guided_prediction_equal_the_executed_reference(golden):
    assert all(v == (2, 2) for v in golden["patch_shapes"].values()) and len(golden["patch_shapes"]) == 7
    assert golden["features"] == IG.N == 64 and golden["default_weight"] == 0.5
    from simpletuner_amd import ops
    assert ops.IG_N == golden["features"]
    g = golden["case"]
    t = g["tokens"].to(BF16)
    assert torch.equal(EMU.unpatchify(t, 16, *g["target"].shape[2:], order=1), IG.unpatchify(t, 16, *g["target"].shape[2:]))
    assert torch.equal(EMU.patchify(g["prediction"].to(BF16), order=1), IG.patchify(g["prediction"].to(BF16)))
    gd = golden["guided"]
    inter = golden["case"]["prediction"]
    assert torch.allclose(inter + gd["scale"] * (gd["final"] - inter), gd["result"], rtol=0, atol=1e-6)
    from simpletuner_amd.foundation import ModelFoundation as MF
    for n, want in golden["default_blocks"].items():
        plug = SimpleNamespace(config=SimpleNamespace())
        assert MF.internal_guidance_block_index(plug, n) == want == max(0, n // 4)


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins (the kernels' contracts in plain torch) against the derived bounds
# ------------------------------------------------------------------------------------------------
def check_fold_fwd_bwd_wgrad(fns, dev, B, rows, D, lead, bf16_params, seed=0):
    """Shared with tests/test_internal_guidance_gpu.py: run fold -> head_fwd -> head_bwd -> wgrad of `fns` (the ops wrappers or the stand-ins) on seeded inputs that
    hold a constant row and a row of large offset, through views with `lead` foreign rows ahead of each sample's rows, and hold EVERY output element to
    tests/internal_guidance_bounds.py.  Returns the outputs (for bit-equality of a second call)."""
    g = torch.Generator().manual_seed(seed + D)
    S, M = lead + rows, B * rows
    joint = torch.randn(B, S, D, generator=g).to(BF16)
    joint[0, lead + 3] = 2.0 ** -7                                                                              # constant row: xhat = 0, rstd = 1000
    joint[B - 1, lead + rows - 2] = (64.0 + torch.randint(-4, 5, (D,), generator=g).float() * 0.5).to(BF16)      # mean 64, bf16-representable spread
    pdt = BF16 if bf16_params else F32
    gamma = (1.0 + 0.25 * torch.randn(D, generator=g)).to(pdt); beta = (0.1 * torch.randn(D, generator=g)).to(pdt)
    W = (torch.randn(IG.N, D, generator=g) / D ** 0.5).to(pdt); b = (0.05 * torch.randn(IG.N, generator=g)).to(pdt)
    dy = (torch.randn(M, IG.N, generator=g) / 64).to(BF16)
    dxj = torch.randn(B, S, D, generator=g).to(BF16)
    joint, gamma, beta, W, b, dy, dxj = (t.to(dev) for t in (joint, gamma, beta, W, b, dy, dxj))
    h, dx = joint[:, lead:], dxj[:, lead:]
    dx0 = dxj.clone()
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)
    Wf, WfT, c, xhat, rstd, y = z(IG.N, D), z(D, IG.N), z(IG.N), z(M, D), z(M, dt=F32), z(M, IG.N)
    grads = [z(D, dt=pdt), z(D, dt=pdt), z(IG.N, D, dt=pdt), z(IG.N, dt=pdt)]
    fns["ig_fold"](gamma, beta, W, b, Wf, WfT, c)
    fns["ig_head_fwd"](h, Wf, c, xhat, rstd, y)
    fns["ig_head_bwd"](xhat, rstd, dy, WfT, dx)
    fns["ig_wgrad"](xhat, dy, gamma, beta, W, *grads)
    cpu = lambda t: t.detach().cpu()
    worst = {}

    def hold(name, got, ref, tol):
        err = (cpu(got).double() - ref).abs()
        assert torch.isfinite(cpu(got).float()).all(), name
        bad = err > tol
        worst[name] = (err / tol.clamp_min(1e-300)).max().item()
        assert not bad.any(), f"{name} D={D} lead={lead}: {int(bad.sum())} elements over the bound, worst err/tol {worst[name]:.3f}"

    Wf64, tWf, c64, tc = IB.fold_bounds(cpu(gamma), cpu(beta), cpu(W), cpu(b))
    hold("Wf", Wf, Wf64, tWf); hold("WfT", WfT, Wf64.t(), tWf.t()); hold("c", c, c64, tc)
    xh64, tx, rs64, trs = IB.fwd_bounds(cpu(h).reshape(M, D))
    hold("xhat", xhat, xh64, tx); hold("rstd", rstd, rs64, trs)
    assert cpu(xhat)[3].abs().max().item() <= tx[3].max().item() and abs(cpu(rstd)[3].item() - 1000.0) <= trs[3].item()
    y64, ty = IB.tokens_bounds(cpu(xhat), cpu(Wf), cpu(c))
    hold("y", y, y64, ty)
    o64, to = IB.bwd_bounds(cpu(xhat), cpu(rstd), cpu(dy), cpu(WfT), cpu(dx0)[:, lead:].reshape(M, D))
    hold("dx", dx.reshape(M, D), o64, to)
    assert torch.equal(cpu(dxj)[:, :lead], cpu(dx0)[:, :lead])                                  # rows outside the view: untouched bit for bit
    assert (cpu(dxj)[:, lead:] != cpu(dx0)[:, lead:]).any()
    for name, got in zip(("g_gamma", "g_beta", "g_W", "g_b"), grads):
        ref, tol = IB.wgrad_bounds(cpu(xhat), cpu(dy), cpu(gamma), cpu(beta), cpu(W), bf16_params)[name]
        hold(name, got, ref, tol)
    # accumulate adds to what the gradient tensors hold
    if not bf16_params:
        twice = [t.clone() for t in grads]
        fns["ig_wgrad"](xhat, dy, gamma, beta, W, *twice, accumulate=True)
        for a, t in zip(grads, twice):
            assert torch.allclose(cpu(t), 2 * cpu(a), rtol=1e-6, atol=0)
    print(f"[ig] D={D} lead={lead} {'bf16' if bf16_params else 'fp32'} params: worst err/bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    return [cpu(t) for t in (Wf, WfT, c, xhat, rstd, y, dxj, *grads)]


@pytest.mark.parametrize("bf16_params", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,lead", [(64, 0), (64, 8), (1536, 8)])
def test_stand_ins_stay_inside_the_derived_bounds(D, lead, bf16_params):
    check_fold_fwd_bwd_wgrad(IG.STAND_INS, "cpu", 2, 35, D, lead, bf16_params)


def test_stand_ins_reproduce_the_executed_reference_end_to_end(golden):
    """unchained: bf16 stand-ins from the fixture's fp32 inputs against the executed reference — the head's tokens within two bf16 roundings of their scale, the
    hidden-state gradient within 2 % rel-L2 (bf16 xhat, bf16 folded weights, bf16 dy)"""
    g, p = golden["case"], golden["params"]
    B, S, D = g["hidden"].shape
    h = g["hidden"].to(BF16)
    Wf, WfT, c = torch.zeros(IG.N, D, dtype=BF16), torch.zeros(D, IG.N, dtype=BF16), torch.zeros(IG.N, dtype=BF16)
    xhat, rstd, y = torch.zeros(B * S, D, dtype=BF16), torch.zeros(B * S), torch.zeros(B * S, IG.N, dtype=BF16)
    IG.ig_fold(p["gamma"], p["beta"], p["W"], p["b"], Wf, WfT, c)
    IG.ig_head_fwd(h, Wf, c, xhat, rstd, y)
    assert PU.rel_l2(y.view(B, S, IG.N), g["tokens"]) < 2 * 2.0 ** -8 * 2
    diff = IG.unpatchify(y.view(B, S, IG.N).float(), 16, *g["target"].shape[2:]) - g["target"]
    dy = IG.patchify(2.0 * g["weight"] * diff / diff.numel()).reshape(-1, IG.N).to(BF16)
    dx = torch.zeros(B, S, D, dtype=BF16)
    IG.ig_head_bwd(xhat, rstd, dy, WfT, dx)
    assert PU.rel_l2(dx, g["grad_hidden"]) < 2e-2
    gr = [torch.zeros(D), torch.zeros(D), torch.zeros(IG.N, D), torch.zeros(IG.N)]
    IG.ig_wgrad(xhat, dy, p["gamma"], p["beta"], p["W"], *gr)
    for t, k in zip(gr, ("grad_gamma", "grad_beta", "grad_W", "grad_b")):
        assert PU.rel_l2(t, g[k]) < 2e-2, k


# ------------------------------------------------------------------------------------------------
# (c) plugin / trainer surface
# ------------------------------------------------------------------------------------------------
def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family="sd3", layers=3, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    IG.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=2, single=2))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(layers))
    return plugin


def test_post_model_load_setup_accepts_internal_guidance_for_sd3(monkeypatch, golden):
    plugin = _plugin(monkeypatch, internal_guidance_enabled=True)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    assert comp._ig_block == 0 == golden["default_blocks"][3] and plugin.internal_guidance.weight == 0.5 and plugin.internal_guidance.block_index == 0
    own = dict(comp.named_parameters())
    assert [tuple(own[PRE + nm].shape) for nm in IG.NAMES] == [(comp.D,), (comp.D,), (64, comp.D), (64,)]
    # the reference's initial values: LayerNorm affine (1, 0), zero projection
    assert (own[PRE + "norm.weight"] == 1).all() and all((own[PRE + nm] == 0).all() for nm in IG.NAMES[1:])
    assert all(own[PRE + nm].requires_grad and own[PRE + nm].dtype == F32 for nm in IG.NAMES)          # LoRA: fp32 masters
    plugin.freeze_components()
    assert all(own[PRE + nm].requires_grad for nm in IG.NAMES)
    # the index is used as it is (0-based, no idx - 1 rule)
    plugin = _plugin(monkeypatch, internal_guidance_enabled=True, internal_guidance_block_index=2, internal_guidance_loss_weight=0.25)
    plugin.add_lora_adapter(); plugin.post_model_load_setup()
    assert plugin.get_trained_component()._ig_block == 2 and plugin.internal_guidance.weight == 0.25
    e = golden["errors"]
    for kw, text in ((dict(internal_guidance_loss_weight=-0.5), e["bad_weight"]), (dict(internal_guidance_loss_weight=0), e["zero_weight"])):
        with pytest.raises(ValueError) as ei:
            _plugin(monkeypatch, internal_guidance_enabled=True, **kw).post_model_load_setup()
        assert str(ei.value) == text
    for idx, text in ((3, e["index_high"]), (-1, e["index_negative"])):
        with pytest.raises(ValueError) as ei:
            _plugin(monkeypatch, internal_guidance_enabled=True, internal_guidance_block_index=idx)
        assert str(ei.value) == text
        with pytest.raises(ValueError) as ei:
            comp.set_internal_guidance(idx)
        assert str(ei.value) == text
    # (the three texts below are common.py:5170-5178's, typed out: that module does not load on its own, so the fixture cannot record them)
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, internal_guidance_enabled=True, lora_type="lycoris").post_model_load_setup()
    assert str(ei.value) == "Internal Guidance requires standard PEFT LoRA or full-model training so its auxiliary head is optimized and saved."
    auto = _plugin(monkeypatch, internal_guidance_enabled=True)
    auto.PREDICTION_TYPE = SimpleNamespace(name="AUTOREGRESSIVE_NEXT_TOKEN", value="autoregressive_next_token")          # an autoregressive prediction type
    with pytest.raises(ValueError) as ei:
        auto.post_model_load_setup()
    assert str(ei.value) == "Internal Guidance is not defined for autoregressive next-token models."
    # off: nothing is laid out, the forward returns one output, auxiliary_loss passes the loss through
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter(); plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    assert plugin.internal_guidance is None and comp._ig_block is None and comp._ig is None and not any(n.startswith(PRE) for n, _ in comp.named_parameters())
    loss = torch.tensor(1.5)
    assert plugin.auxiliary_loss({"model_prediction": None}, {}, loss) == (loss, None)


def test_refusals_by_name(monkeypatch):
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import Trainer
    from tests import test_unet_host_sequencing_cpu as UH
    with pytest.raises(NotImplementedError, match="internal_guidance_enabled.*built: SD3"):          # Flux: the follow-up
        _plugin(monkeypatch, "flux", internal_guidance_enabled=True).post_model_load_setup()
    unet, _ = UH._unet(monkeypatch, "sdxl_small", 3)
    plug = SDXL.__new__(SDXL)
    plug.config, plug.accelerator, plug.model, plug.controlnet = SimpleNamespace(internal_guidance_enabled=True), _acc(), unet, None
    with pytest.raises(ValueError) as ei:
        plug.post_model_load_setup()
    assert str(ei.value) == "Internal Guidance is only supported for diffusion transformer models."
    for flag in ("nextlat_enabled", "crepa_enabled", "irepa_enabled", "urepa_enabled"):
        with pytest.raises(NotImplementedError, match=flag):
            _plugin(monkeypatch, **{flag: True}).post_model_load_setup()
    routes = {"routes": [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": 2}]}
    with pytest.raises(NotImplementedError, match="internal_guidance_enabled with TREAD routing"):
        _plugin(monkeypatch, internal_guidance_enabled=True, tread_config=routes).post_model_load_setup()
    plugin = _plugin(monkeypatch, internal_guidance_enabled=True)
    plugin.add_lora_adapter(); plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    comp.set_router(object(), routes["routes"])          # a router handed to the component directly: refused by the engine at the training forward
    d = SH._inputs(2, 16, 24, 33)
    with pytest.raises(NotImplementedError, match="Internal Guidance under TREAD routing"):
        comp(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"])
    for kw, text in ((dict(hip_graph=True), "hip_graph: Internal Guidance"), (dict(optimizer="muon"), "optimizer 'muon' with internal_guidance_enabled.*st355-adamw"),
                     (dict(optimizer="soap"), "optimizer 'soap' with internal_guidance_enabled.*optimi-lion")):
        plugin = _plugin(monkeypatch, internal_guidance_enabled=True, **kw)
        plugin.SUPPORTS_MUON_CLIP = True
        plugin.add_lora_adapter()
        with pytest.raises(NotImplementedError, match=text):
            Trainer(plugin.config, plugin, plugin.accelerator)
    # a head cannot join arenas that are already laid out
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter()
    with pytest.raises(RuntimeError, match="before add_lora_adapter"):
        plugin.get_trained_component().set_internal_guidance(1)


# ------------------------------------------------------------------------------------------------
# (d) host sequencing: loss and every trainable gradient against autograd through the oracle
# ------------------------------------------------------------------------------------------------
def _set_ckpt(model, mode):
    if mode != "plain":
        model.enable_gradient_checkpointing()
    if mode == "segmented":
        model.set_gradient_checkpointing_interval(2)


def _sd3_model(monkeypatch, layers, block, full, seed=11):
    """tests/test_sd3_host_sequencing_cpu.py::_model with the head laid out (its values seeded: a zero projection would hide the injection)"""
    IG.install(monkeypatch)
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device="cpu", internal_guidance_block_index=block, **SH._arch(layers))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith(PRE):
                continue
            if name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = model.config
        model.pos_embed.pos_embed.copy_(T.sincos_2d(model.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    IG.seed_head(model)
    return model


def _hip(model, d, weight, lam=None):
    res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=True)
    out, igp = res.sample, res.internal_guidance_prediction
    assert igp.shape == out.shape and igp.dtype == BF16 and igp.requires_grad
    tgt = d["target"].float()
    loss = ((out.float() - tgt) ** 2).mean() + weight * ((igp.float() - tgt) ** 2).mean()
    if lam is not None:
        loss = loss - lam * res.layersync_similarity
    loss.backward()
    return out.detach(), loss.detach(), igp.detach()


def _check(model, out, loss, igp, oracle, full):
    o_out, o_loss, o_igp, P, lp, share, head = oracle
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, abs(o_loss.item()))
    assert PU.rel_l2(igp, o_igp) < 2e-2
    assert share >= 0.1, share          # dropping the injection would miss the gradient tolerances by a wide margin
    if full:
        LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",))          # (walks the head's four tensors too)
    else:
        LS.check_lora_grads(model, lp, 5e-2)
    # the head's four gradients, in the form of layersync_ref.check_full_grads
    own = dict(model.named_parameters())
    for nm in IG.NAMES:
        p, ref = own[PRE + nm], head[PRE + nm].grad
        assert p.grad is not None and ref.norm() > 0, nm
        rg, cg = PU.rel_l2(p.grad, ref), PU.cos_sim(p.grad, ref)
        assert rg < 6e-2 and cg > 0.998, f"{nm}: rel={rg:.3e} cos={cg:.5f}"
    return share


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented"])
@pytest.mark.parametrize("block", [0, 1, 2])          # 3 joint blocks (the last is context_pre_only)
@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_with_internal_guidance_matches_autograd_through_the_oracle(monkeypatch, full, block, ckpt):
    model = _sd3_model(monkeypatch, 3, block, full)
    _set_ckpt(model, ckpt)
    d = SH._inputs(2, 16, 24, 33)
    out, loss, igp = _hip(model, d, WEIGHT)
    _, lora, scale = PU.oracle_state(model)
    oracle = IG.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, block, WEIGHT, full, None if full else lora, scale)
    share = _check(model, out, loss, igp, oracle, full)
    print(f"[emu] sd3 internal guidance {'full' if full else 'lora'} block {block} {ckpt}: regulariser share of the trunk gradient={share:.3e}")


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_with_internal_guidance_and_layersync_together(monkeypatch, full):
    """outputs in the order (out, sim, ig_pred); both gradients enter the dX chain at their blocks"""
    model = _sd3_model(monkeypatch, 3, 1, full)
    model.set_layersync(0, 2)
    d = SH._inputs(2, 16, 24, 33)
    tup = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    assert len(tup) == 3 and tup[1].dim() == 0 and tup[2].shape == tup[0].shape
    out, loss, igp = _hip(model, d, WEIGHT, lam=8.0)
    _, lora, scale = PU.oracle_state(model)
    oracle = IG.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, 1, WEIGHT, full, None if full else lora, scale, layersync=(0, 2, 8.0))
    _check(model, out, loss, igp, oracle, full)


def test_gradient_accumulation_adds_the_head_gradients(monkeypatch):
    """LoRA, two micro-steps with accumulate_lora_grads: the head's gradient views hold the sum, like the adapters'"""
    model = _sd3_model(monkeypatch, 3, 1, False)
    d1, d2 = SH._inputs(2, 16, 24, 33, seed=5), SH._inputs(2, 16, 24, 33, seed=6)
    own = dict(model.named_parameters())
    singles = []
    for d in (d1, d2):
        _hip(model, d, WEIGHT)
        singles.append([own[PRE + nm].grad.clone() for nm in IG.NAMES])
        for p in model.parameters():
            p.grad = None
    _hip(model, d1, WEIGHT)
    model.accumulate_lora_grads = True
    for p in model.parameters():
        p.grad = None                            # the engine's flat gradient arena keeps the first micro-step's values
    _hip(model, d2, WEIGHT)
    for nm, a, b in zip(IG.NAMES, *singles):
        assert torch.allclose(own[PRE + nm].grad, a + b, rtol=1e-5, atol=1e-7 * (a + b).abs().max().item()), nm


def test_tap_below_the_first_trained_block_fills_only_the_head_gradients(monkeypatch, golden):
    """backward(d_pred, None): no dX accumulation (a student block below the first adapter-carrying block), the head's gradients as with it"""
    from simpletuner_amd.engine import InternalGuidanceHead, InternalGuidanceTap
    IG.install(monkeypatch)
    g = torch.Generator().manual_seed(2)
    B, H, W, D = 2, 10, 14, 64
    rows = (H // 2) * (W // 2)
    params = [1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(64, D, generator=g) / 8, 0.05 * torch.randn(64, generator=g)]
    outs = []
    for with_dx in (True, False):
        grads = [torch.zeros_like(p) for p in params]
        ready = []
        head = InternalGuidanceHead(1, D, params, grads, 128, 128 + sum(p.numel() for p in params), "cpu")
        tap = InternalGuidanceTap(head)
        joint = torch.randn(B, rows + 8, D, generator=torch.Generator().manual_seed(3)).to(BF16)
        tap.tap(0, joint[:, 8:])
        assert tap.y is None                      # only at its block
        tap.tap(1, joint[:, 8:])
        pred = tap.prediction(H, W)
        assert pred.shape == (B, 16, H, W)
        with pytest.raises(ValueError) as ei:          # the reference's text, recorded with tokens=34 for the (10, 14) target
            InternalGuidanceTap.prediction(SimpleNamespace(y=tap.y, rows=rows - 1, B=B, channels=16, block=1), H, W)          # (a tap that saw 34 tokens)
        assert str(ei.value) == golden["errors"]["token_mismatch"]
        dx = torch.zeros(B, rows, D, dtype=BF16)
        tap.backward(torch.randn(B, 16, H, W, generator=torch.Generator().manual_seed(4)).to(BF16) / 64, dx if with_dx else None, False,
                     SimpleNamespace(ready=lambda lo, hi: ready.append((lo, hi))))
        assert ready == [(head.flat_lo, head.flat_hi)] and (dx.abs().max() > 0) == with_dx and all(t.abs().max() > 0 for t in grads)
        outs.append(grads)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# (e) arena invariants: one run for the optimizer, EMA, clipping
# ------------------------------------------------------------------------------------------------
def _trainer(monkeypatch, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, internal_guidance_enabled=True, internal_guidance_block_index=1, lora_rank=8, lora_init_b_std=0.02, **cfg_kw)
    if plugin.config.model_type == "lora":
        plugin.add_lora_adapter()
    else:
        plugin.freeze_components()
    plugin.post_model_load_setup()
    IG.seed_head(plugin.get_trained_component())
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


@pytest.mark.parametrize("model_type", ["lora", "full"])
def test_trainable_parameters_and_gradients_stay_one_run_with_the_head(monkeypatch, model_type):
    from simpletuner_amd.training.optimizer import flat_view
    plugin, trainer, batch = _trainer(monkeypatch, model_type=model_type)
    comp = plugin.get_trained_component()
    params = comp.trainable_parameters()
    own = dict(comp.named_parameters())
    head = [own[PRE + nm] for nm in IG.NAMES]
    assert all(any(p is h for p in params) for h in head)
    flat = flat_view([p.data for p in params])
    assert flat is not None and flat.numel() >= sum(p.numel() for p in params)
    assert flat.dtype == (F32 if model_type == "lora" else BF16) and head[0].dtype == flat.dtype
    loss = trainer.model.loss_with_logs
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    total, logs = plugin.auxiliary_loss(pred, prepared, loss(prepared, pred)[0])
    total.backward()
    gflat = flat_view([p.grad for p in params])
    assert gflat is not None and all(h.grad is not None and h.grad.abs().max() > 0 for h in head)


def test_train_step_adds_the_regulariser_keeps_its_logs_and_moves_the_head(monkeypatch, golden):
    """Trainer.train_step: loss = mse + weight * loss(head prediction), the logs as floats in `last_aux_logs`, merged with LayerSync's when both are on"""
    plugin, trainer, batch = _trainer(monkeypatch, learning_rate=1e-3, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=3,
                                      use_ema=True, ema_decay=0.9, max_grad_norm=0.05)
    comp = plugin.get_trained_component()
    own = dict(comp.named_parameters())
    before = [own[PRE + nm].detach().clone() for nm in IG.NAMES]
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    mse, _ = plugin.loss_with_logs(prepared, pred)
    total, logs = plugin.auxiliary_loss(pred, prepared, mse)
    assert set(logs) == {"internal_guidance_loss", "internal_guidance_unweighted_loss", "layersync_loss", "layersync_similarity"} and all(isinstance(v, float) for v in logs.values())
    inter = plugin.loss(prepared, {"model_prediction": pred["internal_guidance_prediction"]}, apply_conditioning_mask=True)
    assert logs["internal_guidance_unweighted_loss"] == inter.item() and abs(logs["internal_guidance_loss"] - 0.5 * inter.item()) < 1e-7
    assert abs(total.item() - (mse.item() + 0.5 * inter.item() + logs["layersync_loss"])) < 1e-5
    # the same micro-step by hand: the gradient norm over adapters + head, and over the adapters alone
    total.backward()
    params = comp.trainable_parameters()
    sq = lambda ps: sum(p.grad.double().pow(2).sum().item() for p in ps) ** 0.5
    norm_all, norm_adapters = sq(params), sq([p for n, p in comp.named_parameters() if ".lora_" in n])
    assert norm_all > 1.01 * norm_adapters                                                              # the head's share is visible in the norm
    for p in params:
        p.grad = None
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - total.item()) < 1e-5 and trainer.last_aux_logs == logs
    assert all(not torch.equal(own[PRE + nm].detach(), b) for nm, b in zip(IG.NAMES, before))          # AdamW moved all four
    # the on-device norm (and with it the clip coefficient) covers the head's range of the arena: it is the norm over adapters + head, not over the adapters
    assert float(trainer.last_grad_norm) > 0.05 and abs(float(trainer.last_grad_norm) - norm_all) <= 1e-4 * norm_all
    sh = getattr(trainer.ema_model, "shadow_flat", None)
    assert sh is not None                         # the trainables are still ONE run: the EMA keeps its flat shadow, which covers the head's range and lags it
    lo, hi = comp._ig.flat_lo, comp._ig.flat_hi
    cur = comp.lora_flat[lo:hi]
    assert sh.numel() >= hi and 0 < (sh[lo:hi].float() - cur).abs().max().item() < (torch.cat([b.reshape(-1) for b in before]) - cur).abs().max().item()
    with torch.no_grad():          # a prediction outside training carries no head output: the regulariser cannot be evaluated on it
        with pytest.raises(ValueError) as ei:
            plugin.auxiliary_loss(plugin.model_predict(prepared), prepared, mse)
        assert str(ei.value) == golden["errors"]["no_buffer"]


@pytest.mark.parametrize("opt", ["adamw_bf16", "optimi-lion"])
@pytest.mark.parametrize("model_type", ["lora", "full"])
def test_the_other_one_launch_optimizers_move_the_head(monkeypatch, model_type, opt):
    from tests import lion_bounds as LB
    # (full fine-tune under Lion: every step moves a bf16 parameter by lr exactly, Kahan-compensated — 1e-2 so that two steps pass the bf16 ulp of gamma ~ 1, 2^-7)
    lr = 1e-3 if model_type == "lora" else (1e-2 if opt == "optimi-lion" else 1e-4)
    plugin, trainer, batch = _trainer(monkeypatch, model_type=model_type, optimizer=opt, learning_rate=lr)
    LB.install(monkeypatch)                       # (the emulated ops.lion_step)
    own = dict(plugin.get_trained_component().named_parameters())
    before = [own[PRE + nm].detach().clone() for nm in IG.NAMES]
    for _ in range(2):
        trainer.train_step(dict(batch))
    moved = [not torch.equal(own[PRE + nm].detach(), b) for nm, b in zip(IG.NAMES, before)]
    assert all(moved), dict(zip(IG.NAMES, moved))


# ------------------------------------------------------------------------------------------------
# (f) files and sampling
# ------------------------------------------------------------------------------------------------
def test_lora_file_round_trip_carries_the_head(monkeypatch, golden, tmp_path):
    from safetensors.torch import load_file
    plugin, _, _ = _trainer(monkeypatch)
    comp = plugin.get_trained_component()
    vals = {n: p.detach().clone() for n, p in comp.named_parameters() if n.startswith(PRE)}
    path = plugin.save_lora_weights(str(tmp_path))
    flat = load_file(path)
    keys = sorted(k for k in flat if "internal_guidance_head" in k)
    assert keys == sorted("transformer." + PRE + s for s in ("norm.weight", "norm.bias", "proj.weight", "proj.bias", "block_index"))
    # the reference's own key layout for the head (its loader, executed on a dict in this layout when the fixture was made)
    assert sorted(k.split(PRE)[1] for k in keys) == sorted(golden["loader"]["head_state"]) and golden["loader"]["block_index"] == 1
    assert all(PRE not in k for k in golden["loader"]["lora_keys"])
    bi = flat["transformer." + PRE + "block_index"]
    assert bi.dtype == torch.int64 and bi.dim() == 0 and bi.item() == 1
    adapter_dtype = next(v.dtype for k, v in flat.items() if ".lora_A." in k)
    assert all(flat["transformer." + PRE + nm].dtype == adapter_dtype for nm in IG.NAMES)
    with torch.no_grad():
        for n, p in comp.named_parameters():
            if n.startswith(PRE) or ".lora_" in n:
                p.add_(0.5)
    plugin.load_lora_weights(input_dir=str(tmp_path))
    for n, p in comp.named_parameters():
        if n.startswith(PRE):
            assert torch.equal(p.detach(), vals[n]), n
    # strict: a file with a head, no head configured
    plain = _plugin(monkeypatch, lora_rank=8)
    plain.add_lora_adapter(); plain.post_model_load_setup()
    with pytest.raises(ValueError, match="carries an Internal Guidance head"):
        plain.load_lora_weights(input_dir=str(tmp_path))
    # ... a ComfyUI-dialect file into a component with a head: refused (that dialect cannot carry the head; it would silently keep its initial values)
    plugin.config.lora_format = "comfyui"
    plugin.save_lora_weights(str(tmp_path / "comfy_in"))
    with pytest.raises(ValueError, match="ComfyUI-format LoRA file cannot carry the Internal Guidance head"):
        plugin.load_lora_weights(input_dir=str(tmp_path / "comfy_in"))
    plugin.config.lora_format = None
    # ... a head configured, a file without one
    plain.save_lora_weights(str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="block index"):
        plugin.load_lora_weights(input_dir=str(tmp_path / "plain"))
    # the ComfyUI export drops the head
    plugin.config.lora_format = "comfyui"
    assert not any("internal_guidance" in k for k in load_file(plugin.save_lora_weights(str(tmp_path / "comfy"))))


def test_full_checkpoint_carries_the_head_through_the_parameter_names(monkeypatch):
    model = _sd3_model(monkeypatch, 2, 0, True)
    sd = model.diffusers_state_dict()
    assert all(PRE + nm in sd and sd[PRE + nm].dtype == BF16 for nm in IG.NAMES)
    other = _sd3_model(monkeypatch, 2, 0, True, seed=12)
    with torch.no_grad():
        for nm in IG.NAMES:
            dict(other.named_parameters())[PRE + nm].zero_()
    other.load_flat_state(sd)
    assert all(torch.equal(dict(other.named_parameters())[PRE + nm], sd[PRE + nm]) for nm in IG.NAMES)


def test_sampling_extrapolates_from_the_head_per_forward(monkeypatch, golden):
    from simpletuner_amd.sampling import sample_images
    plugin, _, _ = _trainer(monkeypatch)
    g = torch.Generator().manual_seed(9)
    pe, pp, lat = torch.randn(2, 24, 128, generator=g), torch.randn(2, 64, generator=g), torch.randn(2, 16, 16, 8, generator=g)
    kw = dict(latent_height=16, latent_width=8, num_inference_steps=1, decode=False, latents=lat)
    calls = []
    real = plugin.model_predict

    def spy(batch):
        out = real(batch)
        calls.append((bool(batch.get("return_internal_guidance")), out))
        return out

    plugin.model_predict = spy
    base = sample_images(plugin, pe, pp, **kw)
    assert calls[-1][0] is False and "internal_guidance_prediction" not in calls[-1][1]          # s = 1 (the config's default) skips the head entirely
    assert torch.equal(sample_images(plugin, pe, pp, internal_guidance_scale=1.0, **kw), base)
    guided = sample_images(plugin, pe, pp, internal_guidance_scale=1.5, **kw)
    flag, out = calls[-1]
    final, inter = out["model_prediction"].float(), out["internal_guidance_prediction"].float()
    assert flag and not torch.equal(guided, base) and (inter - final).abs().max() > 0
    # one Euler step is linear in the prediction: x1 = x0 + dsigma * pred, so (guided - x0) / (base - x0) carries inter + s * (final - inter) over final
    x0 = lat.to(BF16).float()
    want = (inter + 1.5 * (final - inter)).to(BF16).float()
    step = (base.float() - x0)
    dsig = (step * final).sum() / (final * final).sum()
    assert PU.rel_l2(guided.float() - x0, dsig * want) < 2e-2
    plugin.config.validation_internal_guidance_scale = 1.5          # the config's value is the default
    assert torch.equal(sample_images(plugin, pe, pp, **kw), guided)
    with pytest.raises(ValueError) as ei:
        sample_images(plugin, pe, pp, internal_guidance_scale=0, **kw)
    assert str(ei.value) == golden["errors"]["bad_scale"]
    plain = _plugin(monkeypatch, lora_rank=8)
    plain.add_lora_adapter()
    with pytest.raises(ValueError) as ei:
        sample_images(plain, pe, pp, internal_guidance_scale=1.5, **kw)
    assert str(ei.value) == golden["errors"]["no_head"]

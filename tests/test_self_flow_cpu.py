"""Self-Flow (CREPA with crepa_feature_source=self_flow) on the CPU: the fp64 restatement against the executed reference (tests/golden/self_flow_vectors.pt), the
stand-ins inside the kernels' derived bounds, the configuration surface with the reference's texts, the SD3 engine on the emulator against autograd through the
oracle, and Trainer.train_step with the EMA teacher."""
import hashlib
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import layersync_ref as LS
from tests import parity_utils as PU
from tests import self_flow_bounds as SB
from tests import self_flow_ref as SF
from tests import test_sd3_host_sequencing_cpu as SH

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "self_flow_vectors.pt"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PRE = SF.PREFIX
W_ALIGN = 4.0          # the alignment weight of the engine tests: large enough for the regulariser's share of every gradient to show


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


# ------------------------------------------------------------------------------------------------
# (a) the restatement equals the executed reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("ratio", [0.0, 0.25, 0.5])
def test_views_restatement_equals_the_executed_reference(golden, dt, ratio):
    """fp32 latents: the reference computes in fp32 — within 8 fp32 ulps of the terms' magnitude.  bf16 latents: the reference rounds sigma, 1 - sigma, both products
    and the sum to bf16: five roundings of half a bf16 ulp, at most 2^-8 relative each — d sigma moves both terms by 2^-8 sigma (|x| + |n|), fl(1 - sigma) the first
    by 2^-8 |x|, the products by 2^-8 of themselves, the sum by 2^-8 |result|: |ref - fp64| <= 2^-8 (3 (|x| + |n|) + |result|), i.e. 4 half-ulps at the operands'
    magnitude.  The sigma grid, the teacher's and the tokens' timesteps are rounded to bf16 there (half an ulp, 2^-8 relative); the kernel keeps them fp32."""
    v = golden["views"][f"{dt}_ratio{ratio}"]
    r = SF.views64(v["latents"], v["noise"], v["base_sigmas"], v["alt_sigmas"], v["base_timesteps"], v["alt_timesteps"], v["uniforms"], v["ratio"], v["patch_size"])
    assert torch.equal(r["mask"], v["crepa_self_flow_mask"])
    mag = v["latents"].to(F64).abs() + v["noise"].to(F64).abs()
    if dt == "fp32":
        tol_x = lambda ref: 8 * 2.0 ** -24 * mag
        tol_s = lambda ref: 2.0 ** -24 * ref.abs()
    else:
        tol_x = lambda ref: 2.0 ** -8 * (3 * mag + ref.abs())
        tol_s = lambda ref: 2.0 ** -8 * ref.abs()
    for got, key, tol in ((r["noisy_student"], "noisy_latents", tol_x), (r["noisy_teacher"], "crepa_teacher_noisy_latents", tol_x), (r["sigma_grid"], "sigmas", tol_s),
                          (r["token_timesteps"], "timesteps", tol_s), (r["sigma_teacher"].view(-1, 1, 1, 1), "crepa_teacher_sigmas", tol_s),
                          (r["timestep_teacher"], "crepa_teacher_timesteps", tol_s)):
        ref = v[key].to(F64)
        assert got.shape == ref.shape, key
        assert bool(((got - ref).abs() <= tol(got)).all()), (key, float(((got - ref).abs() / tol(got).clamp_min(1e-300)).max()))
    if ratio == 0.0:          # nothing masked: the student is the homogeneous base view
        assert torch.equal(r["token_timesteps"], v["base_timesteps"].to(F64)[:, None].expand_as(r["token_timesteps"]))


def test_loss_restatement_equals_the_executed_reference(golden):
    g = golden["loss"]
    params = tuple(g["params"][nm] for nm in SF.NAMES)
    w = g["logs"]["crepa_weight"]
    loss, sim, _, proj, dh, grads = SF.loss64(g["hidden"], g["teacher"], params, w)
    close = lambda a, b: float((a.to(F64) - b.to(F64)).abs().max()) <= 1e-5 * max(float(b.to(F64).abs().max()), 1e-30)
    assert close(proj, g["projection"]) and abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert abs(float(sim) - g["logs"]["crepa_alignment_score"]) <= 1e-5 * abs(float(sim)) and g["logs"]["crepa_similarity_self"] == g["logs"]["crepa_alignment_score"]
    assert abs(g["logs"]["crepa_loss"] - float(loss)) <= 1e-5 * abs(float(loss)) and g["logs"]["crepa_cutoff"] is False
    assert close(dh, g["grad_hidden"])
    for nm in SF.NAMES:
        assert close(grads[nm], g["grads"][nm]), nm
    assert g["state_keys"] == list(SF.NAMES) and g["module_name"] + "." == PRE and g["attached"] and g["eps"] == SF.EPS and g["param_dtype"] == "torch.float32"
    # the cutoff inside compute_loss: no loss, the cutoff logs — what auxiliary_loss reproduces
    assert g["cutoff"]["loss_is_none"] and g["cutoff"]["logs"]["crepa_cutoff"] is True and g["cutoff"]["logs"]["crepa_weight"] == 0.0 and g["cutoff"]["logs"]["crepa_loss"] == 0.0


def test_scheduler_restatement_equals_the_executed_reference(golden):
    from simpletuner_amd.self_flow import WeightSchedule
    assert set(WeightSchedule.KINDS) <= {c["config"].get("crepa_scheduler") for c in golden["scheduler"].values()}
    for name, case in golden["scheduler"].items():
        sch = WeightSchedule(SimpleNamespace(**case["config"]), case["max_train_steps"])
        for row in case["rows"]:
            w = sch.weight(row["step"], similarity=row["similarity"])
            assert w == row["weight"] and sch.ema == row["ema"] and sch.triggered == row["cutoff"], (name, row, w, sch.ema, sch.triggered)
    rows = golden["scheduler"]["threshold_recoverable"]["rows"]
    assert any(r["weight"] == 0.0 for r in rows) and rows[-1]["weight"] > 0.0          # the recoverable mode comes back
    rows = golden["scheduler"]["threshold_permanent"]["rows"]
    first = next(i for i, r in enumerate(rows) if r["weight"] == 0.0)
    assert all(r["weight"] == 0.0 and r["cutoff"] for r in rows[first:])                # the permanent mode does not


def test_sources_and_validation_texts_equal_the_executed_reference(golden):
    from simpletuner_amd import self_flow as M
    assert list(M.SOURCES) == golden["sources"]["values"]
    for row in golden["sources"]["table"]:
        cfg = SimpleNamespace(**{k: row[k] for k in ("crepa_feature_source", "crepa_use_backbone_features", "crepa_self_flow")})
        kind, val = row["result"]
        if kind == "ok":
            assert M.feature_source(cfg) == val, row
        else:
            with pytest.raises(ValueError) as ei:
                M.feature_source(cfg)
            assert str(ei.value) == val
    e = golden["errors"]
    base = dict(crepa_enabled=True, crepa_feature_source="self_flow", crepa_block_index=1, crepa_teacher_block_index=2, use_ema=True)
    for kw, supported, text in ((dict(), False, e["unsupported_family"]), (dict(use_ema=False), True, e["no_ema"]), (dict(crepa_teacher_block_index=None), True, e["no_teacher_block"]),
                                (dict(crepa_self_flow_mask_ratio=0.6), True, e["ratio_high"]), (dict(crepa_self_flow_mask_ratio=-0.1), True, e["ratio_negative"]),
                                (dict(twinflow_enabled=True), True, e["twinflow"]), (dict(crepa_feature_source="dino"), True, e["bad_source"]),
                                (dict(crepa_use_backbone_features=True), True, e["backbone_flag_conflict"]),
                                (dict(crepa_feature_source="backbone", crepa_self_flow=True), True, e["self_flow_flag_conflict"]),
                                (dict(crepa_feature_source=None, crepa_use_backbone_features=True, crepa_self_flow=True), True, e["both_legacy"])):
        with pytest.raises(ValueError) as ei:
            M.validate(SimpleNamespace(**{**base, **kw}), "Golden Family", supported)
        assert str(ei.value) == text
    assert M.validate(SimpleNamespace(**base), "x", True) == "self_flow" and M.mask_ratio(SimpleNamespace()) == 0.1 and M.mask_ratio(SimpleNamespace(crepa_self_flow_mask_ratio=None)) == 0.0


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins (what the engine tests below run on) stay inside the kernels' bounds; the checker rejects a planted error
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["compact", "strided"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ratio", SB.VIEW_RATIOS)
@pytest.mark.parametrize("shape", SB.VIEW_SHAPES)
def test_views_stand_in_stays_inside_the_derived_bounds(monkeypatch, shape, ratio, dtype, strided):
    SB.check_views_case(SF.install(monkeypatch), "cpu", shape, ratio, dtype, strided)


@pytest.mark.parametrize("D,B,S,strided", SB.HEAD_CASES)
def test_head_stand_ins_stay_inside_the_derived_bounds(monkeypatch, D, B, S, strided):
    SB.check_head_case(SF.install(monkeypatch), "cpu", D, B, S, strided)


def test_the_bounds_reject_a_planted_one_ulp_error(monkeypatch):
    """every bound is tight enough to see ONE bf16 ulp (fp32 outputs: 16 fp32 ulps) planted on the element where the output is largest"""
    ops = SF.install(monkeypatch)
    _, r = SB.check_head_case(ops, "cpu", 128, 3, 10, False)
    ga, be, W, b = r["params"]
    M, D = r["xhat"].shape

    def planted(got, ref, tol, bf16=True):
        i = got.abs().reshape(-1).argmax()
        bad = got.clone().reshape(-1)
        step = (SB.ulp_bf16(bad[i].to(F64)) if bf16 else 16 * 2.0 ** -24 * bad[i].to(F64).abs())
        bad[i] = (bad[i].to(F64) + step * (1 if bad[i] >= 0 else -1)).to(got.dtype)          # away from zero: the next representable value of that scale
        assert bad[i] != got.reshape(-1)[i]
        return SB.worst_ratio(bad.reshape(got.shape), ref.reshape(got.shape), tol.reshape(got.shape))[1]

    fb = SB.fold_bounds(ga, be, W, b)
    assert not planted(r["Wf"], *fb["Wf"]) and not planted(r["c"], *fb["c"])
    xh, tx, _, _ = SB.rows_bounds(r["h"].reshape(M, D))
    assert not planted(r["xhat"], xh, tx)
    assert not planted(r["proj"], *SB.gemm_bounds(r["xhat"], r["Wf"], r["c"]))
    s = float(torch.tensor(-0.37, dtype=F32))
    wb = SB.wgrad_bounds(r["P"], r["db"], ga, be, W, s)
    for i, k in enumerate(("g_gamma", "g_beta", "g_W", "g_b")):
        # (the two column sums over D terms are bounded by (D + 10) u sum |terms|: they are held to one ulp of their bf16 operand P, the elementwise two to fp32 ulps)
        assert not planted(r["grads"][i], *wb[k], bf16=k in ("g_gamma", "g_beta")), k
    # the views: a bf16 ulp on the student's view, and a token that took the wrong timestep
    g = torch.Generator().manual_seed(1)
    shape = (3, 16, 6, 10)
    lat, noise, u = torch.randn(shape, generator=g).to(BF16), torch.randn(shape, generator=g).to(BF16), torch.rand(3, 3, 5, generator=g)
    sig, alt = torch.tensor([0.3, 0.7, 0.55]), torch.tensor([0.65, 0.2, 0.55])
    out = ops.self_flow_views(lat, noise, sig, alt, sig * 1000, alt * 1000, u, 0.25, 2)
    vb = SB.views_bounds(lat, noise, sig, alt, sig * 1000, alt * 1000, u, 0.25, 2)
    assert SB.worst_ratio(out[0], *vb["noisy_student"])[1] and not planted(out[0], *vb["noisy_student"])
    tok = out[2].clone()
    tok[0, 0] = 650.0 if tok[0, 0] == 300.0 else 300.0
    assert not SB.worst_ratio(tok, *vb["token_timesteps"])[1]


def test_views_stand_in_refuses_what_the_kernel_refuses(monkeypatch):
    from tests import ops_emulator as EMU
    ops = SF.install(monkeypatch)
    z = lambda *s: torch.zeros(*s, dtype=BF16)
    v = torch.zeros(1)
    for shape in ((1, 16, 3, 2), (1, 16, 2, 5)):
        with pytest.raises(EMU.EmuError, match="H % patch_size != 0 or W % patch_size != 0"):
            ops.self_flow_views(z(*shape), z(*shape), v, v, v, v, torch.zeros(1, shape[2] // 2, shape[3] // 2), 0.1, 2)
    with pytest.raises(EMU.EmuError, match="mask ratio"):
        ops.self_flow_views(z(1, 16, 2, 2), z(1, 16, 2, 2), v, v, v, v, torch.zeros(1, 1, 1), 0.6, 2)


def test_abi_exports_the_self_flow_symbols():
    """include/st355.h declares, lib.py lists and types, and (when it is built) the library exports the five new entries"""
    from simpletuner_amd import lib
    names = ["st355_self_flow_views", "st355_self_flow_fold", "st355_self_flow_rows", "st355_self_flow_wgrad_workspace", "st355_self_flow_wgrad"]
    header = (ROOT / "include" / "st355.h").read_text()
    for n in names:
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    assert "self_flow.hip" in (ROOT / "simpletuner_amd" / "csrc" / "Makefile").read_text()
    if lib.is_built():
        L = lib.load()
        assert all(hasattr(L, n) for n in names)


# ------------------------------------------------------------------------------------------------
# (c) plugin surface
# ------------------------------------------------------------------------------------------------
CFG = dict(crepa_enabled=True, crepa_feature_source="self_flow", crepa_block_index=1, crepa_teacher_block_index=2, use_ema=True, ema_decay=0.9, crepa_lambda=0.5)


def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family="sd3", layers=3, arch=None, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    SF.install(monkeypatch)
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
        plugin.load_model(**(arch or SH._arch(layers)))
    return plugin


def _setup(plugin):
    """the trainer's order: the trainable arena first, then post_model_load_setup"""
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return plugin


def test_post_model_load_setup_accepts_self_flow_for_sd3(monkeypatch, golden):
    """the configuration path (on the parent commit `crepa_enabled` raises NotImplementedError here, whatever the feature source)"""
    for kw in (dict(), dict(crepa_feature_source="selfflow"), dict(crepa_feature_source=None, crepa_self_flow=True)):
        plugin = _setup(_plugin(monkeypatch, **{**CFG, **kw}))
        comp = plugin.get_trained_component()
        assert (comp._sf_block, comp._sf_teacher_block) == (1, 2) and plugin.self_flow.mask_ratio == 0.1 and plugin.self_flow.patch_size == 2
    own = dict(comp.named_parameters())
    D = comp.D
    assert [tuple(own[PRE + nm].shape) for nm in SF.NAMES] == [(D,), (D,), (D, D), (D,)]
    init = golden["loss"]["init"]          # nn.LayerNorm / nn.Linear defaults: (1, 0), the weight and the bias inside 1 / sqrt(D) and spread over it
    assert (own[PRE + "0.weight"] == 1).all() and (own[PRE + "0.bias"] == 0).all() and init["norm_weight_one"] and init["norm_bias_zero"]
    for nm in ("1.weight", "1.bias"):
        assert 0 < own[PRE + nm].abs().max() <= 1 / D ** 0.5 and own[PRE + nm].std() > 0.4 / D ** 0.5
    assert init["linear_abs_max"] <= init["bound"] and init["bias_abs_max"] <= init["bound"]
    assert all(own[PRE + nm].requires_grad and own[PRE + nm].dtype == F32 and own[PRE + nm].data_ptr() % 16 == 0 for nm in SF.NAMES)
    plugin.freeze_components()
    assert all(own[PRE + nm].requires_grad for nm in SF.NAMES)
    params = comp.trainable_parameters()
    from simpletuner_amd.training.optimizer import flat_view
    assert flat_view([p.data for p in params]) is not None and all(any(p is own[PRE + nm] for p in params) for nm in SF.NAMES)
    # the seed is documented: the adapters' generator (config seed + 7), behind every A / B draw — the same configuration draws the same projector
    again = _setup(_plugin(monkeypatch, **CFG)).get_trained_component()
    assert torch.equal(again.lora_flat, comp.lora_flat)
    # off: nothing is laid out, nothing imported, the forward returns one output, auxiliary_loss passes the loss through
    sys.modules.pop("simpletuner_amd.self_flow", None)
    plugin = _setup(_plugin(monkeypatch))
    comp = plugin.get_trained_component()
    assert plugin.self_flow is None and comp._sf_block is None and comp._sf is None and not any(n.startswith(PRE) for n, _ in comp.named_parameters())
    assert "simpletuner_amd.self_flow" not in sys.modules
    loss = torch.tensor(1.5)
    assert plugin.auxiliary_loss({"model_prediction": None}, {}, loss) == (loss, None)


def test_reference_errors_through_the_plugin(monkeypatch, golden):
    e = golden["errors"]
    for kw, text in ((dict(use_ema=False), e["no_ema"]), (dict(crepa_self_flow_mask_ratio=0.6), e["ratio_high"]), (dict(twinflow_enabled=True), e["twinflow"]),
                     (dict(crepa_use_backbone_features=True), e["backbone_flag_conflict"])):
        ok = _plugin(monkeypatch, **CFG)
        ok.add_lora_adapter()
        for k, v in kw.items():
            setattr(ok.config, k, v)
        with pytest.raises(ValueError) as ei:
            ok.post_model_load_setup()
        assert str(ei.value) == text
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, **{**CFG, "crepa_teacher_block_index": None})
    assert str(ei.value) == e["no_teacher_block"]
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, **{**CFG, "crepa_block_index": None})
    assert str(ei.value) == e["no_block_index"]
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, **{**CFG, "crepa_feature_source": "dino"})
    assert str(ei.value) == e["bad_source"]
    with pytest.raises(ValueError, match=r"crepa_teacher_block_index must be within \[0, 2\], got 3"):
        _plugin(monkeypatch, **{**CFG, "crepa_teacher_block_index": 3})
    # a training forward without teacher features, and a training step without an EMA
    plugin = _setup(_plugin(monkeypatch, **CFG))
    d = SH._inputs(2, 16, 24, 33)
    with pytest.raises(ValueError) as ei:
        plugin.get_trained_component()(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"])
    assert str(ei.value) == e["no_teacher_features"]
    with pytest.raises(ValueError, match="EMA teacher weights are required but unavailable; enable use_ema or allow fallback."):
        plugin._self_flow_teacher_features({})
    with pytest.raises(ValueError) as ei:
        plugin.auxiliary_loss({"model_prediction": None}, {}, torch.tensor(1.0, requires_grad=True))
    assert str(ei.value) == e["no_hidden"]


def test_refusals_by_name(monkeypatch):
    from simpletuner_amd.training.trainer import Trainer
    for flag in ("crepa_enabled", "irepa_enabled", "urepa_enabled"):          # any other source, and the REPA family, as before
        with pytest.raises(NotImplementedError, match=f"{flag}: the REPA regularisers align with an external vision encoder"):
            _plugin(monkeypatch, **{flag: True}).post_model_load_setup()
    for src in ("encoder", "backbone"):
        with pytest.raises(NotImplementedError, match="crepa_enabled: the REPA regularisers"):
            _plugin(monkeypatch, crepa_enabled=True, crepa_feature_source=src).post_model_load_setup()
    with pytest.raises(NotImplementedError, match="irepa_enabled"):
        _plugin(monkeypatch, **{**CFG, "irepa_enabled": True}).post_model_load_setup()
    with pytest.raises(NotImplementedError, match=r"crepa_enabled: Self-Flow .* is not built for .* \(built: SD3 LoRA\)"):          # Flux: the follow-up
        _plugin(monkeypatch, "flux", **CFG).post_model_load_setup()
    from simpletuner_amd.pixart.model import PixartSigma
    from simpletuner_amd.pixart.transformer import PixArtTransformer2DModel
    from simpletuner_amd.sdxl.model import SDXL
    from tests import test_pixart_host_sequencing_cpu as PH
    from tests import test_unet_host_sequencing_cpu as UH
    pix = PixartSigma.__new__(PixartSigma)
    pix.config, pix.accelerator, pix.model, pix.controlnet = SimpleNamespace(**CFG), _acc(), PixArtTransformer2DModel(device="cpu", **PH.ARCH), None
    with pytest.raises(NotImplementedError, match=r"crepa_enabled: Self-Flow .* \(built: SD3 LoRA\)"):
        pix.post_model_load_setup()
    unet, _ = UH._unet(monkeypatch, "sdxl_small", 3)
    plug = SDXL.__new__(SDXL)
    plug.config, plug.accelerator, plug.model, plug.controlnet = SimpleNamespace(**CFG), _acc(), unet, None
    with pytest.raises(NotImplementedError, match=r"crepa_enabled: Self-Flow .* \(built: SD3 LoRA\)"):
        plug.post_model_load_setup()
    no = "crepa_enabled \\(self_flow\\) "
    routes = {"routes": [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": 2}]}
    for kw, text in ((dict(model_type="full"), no + "under a full fine-tune"), (dict(lora_type="lycoris"), no + "with lora_type=lycoris"),
                     (dict(use_dora=True), no + "with use_dora"), (dict(lora_dropout=0.1), no + "with lora_dropout=0.1"),
                     (dict(layersync_enabled=True, layersync_student_block=1), no + "together with layersync_enabled"),
                     (dict(internal_guidance_enabled=True), no + "together with internal_guidance_enabled"),
                     (dict(nextlat_enabled=True, nextlat_weight=0.3), no + "together with nextlat_enabled"), (dict(hip_graph=True), "hip_graph: Self-Flow"),
                     (dict(tread_config=routes), no + "with TREAD routing"), (dict(scheduled_sampling_max_step_offset=2), no + "with scheduled sampling / ReflexFlow"),
                     (dict(scheduled_sampling_reflexflow=True), no + "with scheduled sampling / ReflexFlow"), (dict(distillation_method="flow_dpo"), no + "with distillation_method=flow_dpo"),
                     (dict(mixflow_enabled=True), no + "with mixflow_enabled")):
        ok = _plugin(monkeypatch, **CFG)
        ok.add_lora_adapter()
        for k, v in kw.items():
            setattr(ok.config, k, v)
        with pytest.raises(NotImplementedError, match=text):
            ok.post_model_load_setup()
    ok = _plugin(monkeypatch, **CFG)
    ok.add_lora_adapter()
    ok.xm_config = SimpleNamespace(enabled=True)
    with pytest.raises(ValueError, match="XM noise-candidate training is not compatible with CREPA self-flow"):
        ok.post_model_load_setup()
    with pytest.raises(NotImplementedError, match="SD3.5 dual-attention blocks"):          # SD3.5: refused where the component learns its blocks
        _plugin(monkeypatch, arch=SH._arch(3, qk_norm="rms_norm", dual=(0, 1)), **CFG)
    with pytest.raises(NotImplementedError, match="crepa_enabled: post_model_load_setup while the component has no adapter arena"):
        _plugin(monkeypatch, **CFG).post_model_load_setup()
    for kw, text in ((dict(hip_graph=True), "hip_graph: Self-Flow"), (dict(optimizer="muon"), "optimizer 'muon' with crepa_enabled.*st355-adamw"),
                     (dict(optimizer="soap"), "optimizer 'soap' with crepa_enabled.*optimi-lion")):
        plugin = _plugin(monkeypatch, **{**CFG, **kw})
        plugin.SUPPORTS_MUON_CLIP = True
        plugin.add_lora_adapter()
        with pytest.raises(NotImplementedError, match=text):
            Trainer(plugin.config, plugin, plugin.accelerator)
    # the component: the projector cannot join an arena that is laid out, and excludes the heads and LayerSync
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter()
    with pytest.raises(RuntimeError, match="before add_lora_adapter"):
        plugin.get_trained_component().set_self_flow(1, 2)
    from simpletuner_amd.sd3 import transformer as T
    m = T.SD3Transformer2DModel(device="cpu", **SH._arch(3))
    m.set_self_flow(1, 2)
    for call, text in ((lambda: m.set_internal_guidance(1), "together with Internal Guidance"), (lambda: m.set_nextlat(1), "together with NextLat"),
                       (lambda: m.set_layersync(1, 2), "together with LayerSync")):
        with pytest.raises(NotImplementedError, match=text):
            call()
    with pytest.raises(NotImplementedError, match="together with LayerSync / Internal Guidance / NextLat"):
        T.SD3Transformer2DModel(device="cpu", nextlat_block_index=1, **SH._arch(3)).set_self_flow(1, 2)
    with pytest.raises(NotImplementedError, match=r"crepa_enabled \(self_flow\) with use_dora"):
        m.add_lora_adapter(rank=8, dora=True)
    with pytest.raises(NotImplementedError, match="lycoris lokr with .* a Self-Flow projector"):
        m.add_lokr_adapter()


# ------------------------------------------------------------------------------------------------
# (d) host sequencing: similarity and every gradient against autograd through the oracle
# ------------------------------------------------------------------------------------------------
def _set_ckpt(model, mode):
    if mode != "plain":
        model.enable_gradient_checkpointing()
    if mode == "segmented":
        model.set_gradient_checkpointing_interval(2)


def sd3_model(install, monkeypatch, layers, student, teacher, dev="cpu", arch=SH._arch, seed=11):
    """tests/test_sd3_host_sequencing_cpu.py::_model with the projector laid out, its values seeded off the initial ones"""
    if install is not None:
        install(monkeypatch)
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device=dev, **arch(layers))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = model.config
        model.pos_embed.pos_embed.copy_(T.sincos_2d(model.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])
    model.set_self_flow(student, teacher)
    model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    SF.seed_projector(model)
    return model


def token_timesteps(B, Si, seed=3):
    """a mixed schedule: every token one of two per-sample timesteps"""
    g = torch.Generator().manual_seed(seed)
    base, alt = (torch.rand(B, 1, generator=g) * 0.8 + 0.1) * 1000.0, (torch.rand(B, 1, generator=g) * 0.8 + 0.1) * 1000.0
    return torch.where(torch.rand(B, Si, generator=g) < 0.25, alt, base).contiguous(), torch.minimum(base, alt).reshape(B)


def shadow_of(model, seed=5):
    """an EMA shadow that has moved away from the masters"""
    g = torch.Generator().manual_seed(seed)
    return (model.lora_flat.detach().cpu() + 0.01 * torch.randn(model.lora_flat.shape, generator=g)).to(model.lora_flat.device)


def teacher_features(model, d, shadow, t_T, block):
    dev = model.lora_flat.device
    with torch.no_grad(), model.teacher_values(shadow):
        res = model(hidden_states=d["lat"].to(dev), encoder_hidden_states=d["prompt"].to(dev), pooled_projections=d["pooled"].to(dev), timestep=t_T.to(dev),
                    crepa_capture_block_index=block)
    assert res.sample is None
    return res.crepa_hidden_states


def record_tap_dx(monkeypatch):
    """wraps SelfFlowTap.backward: the gradient with respect to the student block's output right before and right behind the tap's own contribution"""
    from simpletuner_amd import engine as E
    seen, inner = {}, E.SelfFlowTap.backward

    def backward(self, dsim, dx_view, accumulate=False, sync=None):
        seen["before"] = dx_view.detach().float().cpu().clone()
        inner(self, dsim, dx_view, accumulate, sync)
        seen["after"] = dx_view.detach().float().cpu().clone()

    monkeypatch.setattr(E.SelfFlowTap, "backward", backward)
    return seen


def hip_side(model, d, tok, feats, weight):
    dev = model.lora_flat.device
    res = model(hidden_states=d["lat"].to(dev), encoder_hidden_states=d["prompt"].to(dev), pooled_projections=d["pooled"].to(dev), timestep=tok.to(dev),
                crepa_teacher_features=feats, return_dict=True)
    out, sim = res.sample, res.crepa_similarity
    assert sim.dim() == 0 and sim.dtype == F32 and sim.requires_grad
    loss = ((out.float() - d["target"].to(dev).float()) ** 2).mean() - weight * sim
    loss.backward()
    return out.detach().cpu(), loss.detach().cpu(), sim.detach().cpu()


def oracle_side(monkeypatch, model, d, tok, feats, student, weight):
    """autograd through the oracle's student forward on the tokenwise schedule, the alignment on its recorded block output: (pred, loss, sim, lora params, projector
    parameters with .grad, d(-w sim) / d h_student, the regulariser's share of the adapters' gradient)"""
    _, lora, scale = PU.oracle_state(model)
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    out, outs = SF.sd3_oracle_blocks(monkeypatch, model, SH._ocfg(model), d, d["lat"], tok, lp, scale)
    own = dict(model.named_parameters())
    head = {nm: own[PRE + nm].detach().cpu().clone().requires_grad_(True) for nm in SF.NAMES}
    sim = SF.similarity_autograd(outs[student], feats.detach().float().cpu(), tuple(head[nm] for nm in SF.NAMES))
    mse = ((out - d["target"].float()) ** 2).mean()
    total = mse - weight * sim
    wrt = [t for ab in lp.values() for t in ab]
    g_mse = torch.autograd.grad(mse, wrt, retain_graph=True, allow_unused=True)
    dh = torch.autograd.grad(-weight * sim, outs[student], retain_graph=True)[0]
    total.backward()
    return out.detach(), total.detach(), sim.detach(), lp, head, dh, LS._regulariser_share(wrt, g_mse)


def check_step(model, hip, oracle, seen):
    out, loss, sim = hip
    o_out, o_loss, o_sim, lp, head, dh, share = oracle
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, abs(o_loss.item()))
    assert abs(sim.item() - o_sim.item()) < 1e-3          # a mean of cosines: absolute, bf16 block outputs against the fp32 oracle
    assert share >= 0.05, share          # dropping the injection would miss the gradient tolerances by a wide margin
    worst = LS.check_lora_grads(model, lp, 5e-2)
    own = dict(model.named_parameters())
    rg = max(PU.rel_l2(own[PRE + nm].grad, head[nm].grad) for nm in SF.NAMES)
    cg = min(PU.cos_sim(own[PRE + nm].grad, head[nm].grad) for nm in SF.NAMES)
    assert rg < 6e-2 and cg > 0.998, f"projector gradients: rel={rg:.3e} cos={cg:.5f}"
    # dX at the student block: what the tap added.  The view is bf16: its own rounding (2^-9 of what it holds) on top of the chain's stored bf16 operands (g, G, xhat:
    # 2^-6 of the contribution covers them with the oracle's fp32-vs-bf16 block output)
    got, ref = (seen["after"] - seen["before"]).reshape(dh.shape), dh.float()
    assert ref.norm() > 0 and (got - ref).norm() <= 2.0 ** -9 * seen["after"].norm() + 2.0 ** -6 * ref.norm(), ((got - ref).norm().item(), ref.norm().item())
    return share, worst, rg


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented"])
@pytest.mark.parametrize("student,teacher", [(0, 1), (1, 2), (2, 0)])          # 3 joint blocks (the last is context_pre_only); the teacher may lie below the student
def test_sd3_engine_with_self_flow_matches_autograd_through_the_oracle(monkeypatch, student, teacher, ckpt):
    model = sd3_model(SF.install, monkeypatch, 3, student, teacher)
    _set_ckpt(model, ckpt)
    d = SH._inputs(2, 16, 24, 33)
    tok, t_T = token_timesteps(2, 8 * 12)
    masters = model.lora_flat.clone()
    feats = teacher_features(model, d, shadow_of(model), t_T, teacher)
    assert torch.equal(masters, model.lora_flat)
    seen = record_tap_dx(monkeypatch)
    hip = hip_side(model, d, tok, feats, W_ALIGN)
    share, worst, rg = check_step(model, hip, oracle_side(monkeypatch, model, d, tok, feats, student, W_ALIGN), seen)
    print(f"[emu] sd3 self-flow student {student} teacher {teacher} {ckpt}: share={share:.3e}, adapters rel-L2={worst:.3e}, projector rel-L2={rg:.3e}")


def test_teacher_forward_equals_a_component_holding_the_shadow_and_leaves_the_masters(monkeypatch):
    model = sd3_model(SF.install, monkeypatch, 3, 1, 2)
    d = SH._inputs(2, 16, 24, 33)
    _, t_T = token_timesteps(2, 8 * 12)
    shadow, masters = shadow_of(model), model.lora_flat.clone()
    for g in model.lora_groups:
        g.pack()                         # (what every forward does first: the operands of the masters)
    packs = [(g.A_cat.clone(), g.B_blk.clone(), g.A_cat_T.clone(), g.B_blk_T.clone()) for g in model.lora_groups]
    feats = teacher_features(model, d, shadow, t_T, 2)
    assert torch.equal(masters, model.lora_flat)                                                   # the masters are never written
    for g, kept in zip(model.lora_groups, packs):                                                   # ... and the operands are the masters' again on exit
        assert all(torch.equal(a, b) for a, b in zip((g.A_cat, g.B_blk, g.A_cat_T, g.B_blk_T), kept))
    other = sd3_model(None, monkeypatch, 3, 1, 2)                                                   # a component whose adapter VALUES are the shadow
    with torch.no_grad():
        other.lora_flat.copy_(shadow)
        res = other(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=t_T, crepa_capture_block_index=2)
    assert torch.equal(res.crepa_hidden_states, feats) and feats.dtype == BF16 and feats.is_contiguous() and tuple(feats.shape) == (2, 96, model.D)
    with torch.no_grad():                                                                           # and it differs from the masters' own forward
        own = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=t_T, crepa_capture_block_index=2)
    assert not torch.equal(own.crepa_hidden_states, feats)
    with pytest.raises(ValueError, match="crepa_capture_block_index must name a block"):
        model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=t_T, crepa_capture_block_index=3)
    with pytest.raises(ValueError, match="the adapters end at"):
        with model.teacher_values(shadow[:100]):
            pass


def test_gradient_accumulation_adds_and_cutoff_zeroes_the_projector_gradients(monkeypatch):
    model = sd3_model(SF.install, monkeypatch, 3, 1, 2)
    d = SH._inputs(2, 16, 24, 33)
    tok, t_T = token_timesteps(2, 8 * 12)
    feats = teacher_features(model, d, shadow_of(model), t_T, 2)
    hip_side(model, d, tok, feats, W_ALIGN)
    once = model.lora_grad_flat.clone()
    model.accumulate_lora_grads = True
    hip_side(model, d, tok, feats, W_ALIGN)
    lo, hi = model._sf.flat_lo, model._sf.flat_hi
    assert once[lo:hi].abs().max() > 0 and torch.allclose(model.lora_grad_flat[lo:hi], 2 * once[lo:hi], rtol=1e-6, atol=0)
    model.accumulate_lora_grads = False
    # cutoff: the similarity is returned but takes no part in the loss — the tap launches nothing, its gradient views are zero, and the adapters' gradient is the
    # plain tokenwise step's
    for p in model.parameters():
        p.grad = None
    res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=tok, crepa_teacher_features=feats)
    model.self_flow_cutoff()
    ((res.sample.float() - d["target"].float()) ** 2).mean().backward()
    assert model.lora_grad_flat[lo:hi].abs().max() == 0
    cut = model.lora_grad_flat.clone()
    plain = sd3_model(None, monkeypatch, 3, 1, 2)
    plain._sf_block = None          # the same weights without the tap
    out = plain(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=tok).sample
    ((out.float() - d["target"].float()) ** 2).mean().backward()
    assert torch.equal(out, res.sample) and torch.equal(cut[:lo], plain.lora_grad_flat[:lo])


# ------------------------------------------------------------------------------------------------
# (e) Trainer.train_step with the EMA teacher
# ------------------------------------------------------------------------------------------------
def _trainer(monkeypatch, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _setup(_plugin(monkeypatch, **{**CFG, "lora_rank": 8, "lora_init_b_std": 0.02, "learning_rate": 1e-3, "crepa_self_flow_mask_ratio": 0.25, **cfg_kw}))
    SF.seed_projector(plugin.get_trained_component())
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    g = torch.Generator().manual_seed(17)
    alt = torch.rand(2, generator=g) * 0.8 + 0.1
    lat = devt["latents"]
    batch = {"latent_batch": lat, "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"], "crepa_alt_sigmas": alt,
             "crepa_alt_timesteps": alt * 1000.0, "crepa_self_flow_uniforms": torch.rand(lat.shape[0], lat.shape[2] // 2, lat.shape[3] // 2, generator=g)}
    return plugin, trainer, batch, devt


def test_prepare_batch_builds_both_views_and_evaluation_stays_homogeneous(monkeypatch):
    plugin, trainer, batch, devt = _trainer(monkeypatch)
    p = plugin.prepare_batch(dict(batch), {"global_step": 4})
    lat, B = p["latents"], p["latents"].shape[0]
    r = SF.views64(lat, p["input_noise"], devt["sigmas"], batch["crepa_alt_sigmas"], devt["sigmas"] * 1000, batch["crepa_alt_timesteps"], batch["crepa_self_flow_uniforms"], 0.25, 2)
    assert p["timesteps"].shape == (B, (lat.shape[2] // 2) * (lat.shape[3] // 2)) and torch.equal(p["timesteps"].double(), r["token_timesteps"].float().double())
    assert 0 < int(r["mask"].sum()) < r["mask"].numel()
    vb = SB.views_bounds(lat, p["input_noise"], devt["sigmas"], batch["crepa_alt_sigmas"], devt["sigmas"] * 1000, batch["crepa_alt_timesteps"], batch["crepa_self_flow_uniforms"], 0.25, 2)
    assert SB.worst_ratio(p["noisy_latents"], *vb["noisy_student"])[1] and SB.worst_ratio(p["crepa_teacher_noisy_latents"], *vb["noisy_teacher"])[1]
    assert torch.equal(p["crepa_teacher_timesteps"].double(), r["timestep_teacher"].float().double()) and p["crepa_global_step"] == 4 and p["sigmas"] is None
    assert torch.equal(p["flow_target"].float(), (p["noise"].float() - lat.float()).to(BF16).float())          # the flow target is unchanged
    with torch.no_grad():          # evaluation: the homogeneous batch of every other run
        q = plugin.prepare_batch(dict(batch), {"global_step": 4})
    assert q["timesteps"].shape == (B,) and "crepa_teacher_noisy_latents" not in q
    # ratio 0 with an alternate draw that is not cleaner: the teacher's view IS the student's, and at step 0 (the shadow equals the parameters) so are its features
    plugin2, trainer2, batch2, devt2 = _trainer(monkeypatch, crepa_self_flow_mask_ratio=0.0, crepa_block_index=2)
    batch2 = dict(batch2, crepa_alt_sigmas=devt2["sigmas"] + 0.05, crepa_alt_timesteps=(devt2["sigmas"] + 0.05) * 1000.0)
    p2 = plugin2.prepare_batch(dict(batch2), {"global_step": 0})
    assert torch.equal(p2["noisy_latents"], p2["crepa_teacher_noisy_latents"]) and torch.equal(p2["timesteps"], p2["crepa_teacher_timesteps"][:, None].expand_as(p2["timesteps"]))
    from simpletuner_amd import engine as E
    seen, inner = {}, E.SelfFlowTap.tap

    def tap(self, g, view):
        if g == self.block:
            seen["student"], seen["teacher"] = view.detach().clone(), self.teacher.detach().clone()
        inner(self, g, view)

    monkeypatch.setattr(E.SelfFlowTap, "tap", tap)
    plugin2.model_predict(p2)
    # (the tokenwise route forms its modulation rows per token, the per-sample route per sample: the same numbers up to the bf16 roundings of two GEMM routes)
    assert PU.rel_l2(seen["student"], seen["teacher"]) < 1e-2


def test_train_step_aligns_to_the_moving_ema_and_keeps_the_logs(monkeypatch, golden):
    plugin, trainer, batch, _ = _trainer(monkeypatch)
    comp = plugin.get_trained_component()
    assert plugin.ema_model is trainer.ema_model and trainer.ema_model.shadow_flat is not None
    own = dict(comp.named_parameters())
    before = [own[PRE + nm].detach().clone() for nm in SF.NAMES]
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    mse, _ = plugin.loss_with_logs(prepared, pred)
    total, logs = plugin.auxiliary_loss(pred, prepared, mse)
    assert list(logs) == list(golden["loss"]["logs"]) and logs["crepa_cutoff"] is False and logs["crepa_weight"] == 0.5
    sim = pred["crepa_similarity"].item()
    assert logs["crepa_alignment_score"] == sim == logs["crepa_similarity_self"] == logs["crepa_alignment_score_ema"] and abs(logs["crepa_loss"] + 0.5 * sim) < 1e-7
    assert abs(total.item() - (mse.item() - 0.5 * sim)) < 1e-5
    for p in comp.trainable_parameters():
        p.grad = None
    plugin.self_flow.schedule.ema = None
    masters = []
    for step in range(3):
        masters.append(comp.lora_flat.clone())
        loss = trainer.train_step(dict(batch))
        if step == 0:
            assert abs(loss.item() - total.item()) < 1e-5 and trainer.last_aux_logs == logs
        # the shadow lags the masters from the first update on: the teacher is no longer the student
        sh = trainer.ema_model.shadow_flat
        assert not torch.equal(sh, comp.lora_flat[:sh.numel()]) and not torch.equal(masters[-1], comp.lora_flat)
    assert all(not torch.equal(own[PRE + nm].detach(), b) for nm, b in zip(SF.NAMES, before))          # AdamW moved all four
    assert trainer.last_aux_logs["crepa_alignment_score_ema"] != trainer.last_aux_logs["crepa_alignment_score"]


def test_cutoff_step_adds_nothing_to_the_loss_or_the_gradient(monkeypatch, golden):
    plugin, trainer, batch, _ = _trainer(monkeypatch, crepa_cutoff_step=1)
    comp = plugin.get_trained_component()
    lo, hi = comp._sf.flat_lo, comp._sf.flat_hi
    trainer.train_step(dict(batch))
    assert trainer.last_aux_logs["crepa_cutoff"] is False
    head = comp.lora_flat[lo:hi].clone()
    prepared = plugin.prepare_batch(dict(batch), dict(trainer.state))
    pred = plugin.model_predict(prepared)
    mse, _ = plugin.loss_with_logs(prepared, pred)
    total, logs = plugin.auxiliary_loss(pred, prepared, mse)
    want = golden["loss"]["cutoff"]["logs"]
    assert total is mse and list(logs) == list(want) and logs["crepa_cutoff"] is True and logs["crepa_weight"] == 0.0 and logs["crepa_loss"] == 0.0
    total.backward()
    assert comp.lora_grad_flat[lo:hi].abs().max() == 0 and comp.lora_grad_flat[:lo].abs().max() > 0
    for p in comp.trainable_parameters():
        p.grad = None
    trainer.train_step(dict(batch))          # ... and through the trainer: AdamW's decay alone moves the projector (no gradient reaches it)
    assert trainer.last_aux_logs["crepa_cutoff"] is True
    moved = (comp.lora_flat[lo:hi] - head).abs().max().item()
    assert moved <= 1.1 * 1e-3 * 1e-2 * head.abs().max().item() + 1e-3 * 1.0          # lr * weight_decay * |p|, plus at most lr from the moments of step 1


def test_save_and_resume_continue_bit_identically(monkeypatch, tmp_path):
    plugin, trainer, batch, _ = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    trainer.save_state(str(tmp_path / "ck"))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / "ck" / "pytorch_lora_weights.safetensors"))
    own = dict(plugin.get_trained_component().named_parameters())
    for nm in SF.NAMES:          # the projector travels with the adapter file under the reference's module name
        assert torch.equal(saved["transformer." + PRE + nm].float(), own[PRE + nm].detach().to(saved["transformer." + PRE + nm].dtype).float())
    want = [trainer.train_step(dict(batch)).item() for _ in range(2)]
    want_w, want_sh = plugin.get_trained_component().lora_flat.clone(), trainer.ema_model.shadow_flat.clone()
    plugin2, trainer2, _, _ = _trainer(monkeypatch)
    with torch.no_grad():
        plugin2.get_trained_component().lora_flat.add_(0.25)
    trainer2.load_state(str(tmp_path / "ck"))
    got = [trainer2.train_step(dict(batch)).item() for _ in range(2)]
    assert got == want and torch.equal(plugin2.get_trained_component().lora_flat, want_w) and torch.equal(trainer2.ema_model.shadow_flat, want_sh)
    # a file that carries a projector needs a component that has one
    plain = _setup(_plugin(monkeypatch, lora_rank=8))
    with pytest.raises(ValueError, match="LoRA checkpoint carries a Self-Flow projector"):
        plain.load_lora_weights(input_dir=str(tmp_path / "ck"))


def test_launch_trace_with_the_flag_off_is_the_parents(tmp_path):
    """flag off, nothing moved: tools/launch_trace.py over the SD3 tokenwise host-sequencing tests and the LoRA NextLat engine tests (the tokenwise forward and
    backward this feature consumes; the tap list and the adapter arena it extends) gives, byte for byte, the file it gave at the parent commit, whose digest was
    recorded there (tests/golden/self_flow_launch_trace.sha256)"""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "launch_trace.py"), str(out), "-k", SB.TRACE_SELECTION], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = (ROOT / "tests" / "golden" / "self_flow_launch_trace.sha256").read_text().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

"""LayerSync (helpers/training/layersync.py) on the CPU: the fp64 restatement against the executed reference's golden file, the plugin / trainer surface, and the
engines' host sequencing — where the regulariser's gradient enters the hand-written dX chain, under every checkpoint mode — against autograd through the oracle
(tests/ops_emulator.py + the two stand-ins of tests/layersync_ref.py)."""
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import layersync_ref as LS
from tests import parity_utils as PU
from tests import test_flux_host_sequencing_cpu as FH
from tests import test_sd3_host_sequencing_cpu as SH

BF16 = torch.bfloat16
# the weight of the engine cases: at the reference's default 0.2 the regulariser is ~2 % of these tiny models' adapter gradient, below the gradient tolerances —
# a dropped or misplaced injection would pass.  8.0 makes the two terms comparable (every case asserts the regulariser's measured share)
LAMBDA = 8.0


# ------------------------------------------------------------------------------------------------
# (c) host sequencing: loss and every trainable gradient against autograd through the oracle
# ------------------------------------------------------------------------------------------------
def _set_ckpt(model, mode):
    if mode != "plain":
        model.enable_gradient_checkpointing()
    if mode == "segmented":
        model.set_gradient_checkpointing_interval(2)


def _flux_model(monkeypatch, layers, single):
    model = FH._model(monkeypatch, layers, single)          # (installs the emulator)
    LS.install(monkeypatch)
    return model


def _sd3_model(monkeypatch, layers):
    model = SH._model(monkeypatch, layers)
    LS.install(monkeypatch)
    return model


def _flux_hip(model, d, lam):
    out, sim = model(hidden_states=d["packed"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], img_ids=d["img_ids"],
                     txt_ids=d["txt_ids"], guidance=d["guidance"], return_dict=False)
    assert sim.dim() == 0 and sim.dtype == torch.float32 and sim.requires_grad
    loss = ((out.float() - d["target"].float()) ** 2).mean() - lam * sim
    loss.backward()
    return out.detach(), loss.detach(), sim.detach()


FLUX_PAIRS = [(0, 1), (1, 3), (2, 4), (3, 3)]          # 2 double + 3 single blocks: both double; last double -> single; both single; teacher == student (the reference's default)


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented"])
@pytest.mark.parametrize("student,teacher", FLUX_PAIRS)
@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_flux_engine_with_layersync_matches_autograd_through_the_oracle(monkeypatch, full, student, teacher, ckpt):
    model = _flux_model(monkeypatch, 2, 3)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, targets="all", init_b_std=0.02)
    _set_ckpt(model, ckpt)
    model.set_layersync(student, teacher)
    d = FH._inputs(2, 16, 8, 24)
    out, loss, sim = _flux_hip(model, d, LAMBDA)
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_sim, P, lp, share = LS.flux_oracle(monkeypatch, model, d, student, teacher, LAMBDA, full, None if full else lora, scale)
    print(f"[emu] flux layersync {'full' if full else 'lora'} s{student} t{teacher} {ckpt}: sim={sim.item():.6f} oracle={o_sim.item():.6f} regulariser share of the gradient={share:.3e}")
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, abs(o_loss.item()))
    assert abs(sim.item() - o_sim.item()) < 2e-3 / LAMBDA          # the loss tolerance above, carried by the regulariser's term alone
    if teacher == student:
        assert abs(sim.item() - 1.0) < 1e-3
    else:
        assert share > 0.2, share        # dropping the injection would miss the gradient tolerances by a wide margin
    LS.check_full_grads(model, P) if full else LS.check_lora_grads(model, lp, 5e-2)          # the tolerances of tests/test_flux_host_sequencing_cpu.py


def _sd3_hip(model, d, lam):
    out, sim = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    assert sim.dim() == 0 and sim.dtype == torch.float32 and sim.requires_grad
    loss = ((out.float() - d["target"].float()) ** 2).mean() - lam * sim
    loss.backward()
    return out.detach(), loss.detach(), sim.detach()


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented"])
@pytest.mark.parametrize("student,teacher", [(0, 1), (1, 2), (2, 2)])          # 3 joint blocks (the last is context_pre_only); teacher == student is the reference's default
@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_with_layersync_matches_autograd_through_the_oracle(monkeypatch, full, student, teacher, ckpt):
    model = _sd3_model(monkeypatch, 3)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    _set_ckpt(model, ckpt)
    model.set_layersync(student, teacher)
    d = SH._inputs(2, 16, 24, 33)
    out, loss, sim = _sd3_hip(model, d, LAMBDA)
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_sim, P, lp, share = LS.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, student, teacher, LAMBDA, full, None if full else lora, scale)
    print(f"[emu] sd3 layersync {'full' if full else 'lora'} s{student} t{teacher} {ckpt}: sim={sim.item():.6f} oracle={o_sim.item():.6f} regulariser share of the gradient={share:.3e}")
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, abs(o_loss.item()))
    assert abs(sim.item() - o_sim.item()) < 2e-3 / LAMBDA          # the loss tolerance above, carried by the regulariser's term alone
    if teacher == student:
        assert abs(sim.item() - 1.0) < 1e-3
    else:
        assert share > 0.2, share
    LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",)) if full else LS.check_lora_grads(model, lp, 5e-2)          # tests/test_sd3_host_sequencing_cpu.py


# ------------------------------------------------------------------------------------------------
# (a) the restatement against the executed reference (tests/golden/layersync_vectors.pt, tools/gen_layersync_golden.py)
# ------------------------------------------------------------------------------------------------
GOLDEN = Path(__file__).resolve().parent / "golden" / "layersync_vectors.pt"


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=True)


@pytest.mark.parametrize("case", ["case", "zero_rows", "same_layer"])
def test_restatement_equals_the_executed_reference(golden, case):
    """loss, logs and d loss / d student of LayerSyncRegularizer.compute_loss.  The golden numbers are fp32 (a D-term dot product and two norms per row): the
    fp64 restatement may differ from them by the reference's own rounding, 5 * D * 2^-24 relative (D = 64: 1.9e-5); `zero_rows` holds one all-zero student row
    (gradient t^ / 1e-12 / N, ~1e9) and one all-zero teacher row (gradient 0) — F.normalize's clamp, as executed"""
    g = golden[case]
    D = g["student"].shape[-1]
    tol = 5 * D * 2.0 ** -24
    loss, logs, grad = LS.loss64(g["student"], g["teacher"], g["weight"])
    assert abs(loss.item() - g["loss"].item()) <= tol and abs(logs["layersync_similarity"] - g["logs"]["layersync_similarity"]) <= tol
    assert abs(logs["layersync_loss"] - g["logs"]["layersync_loss"]) <= tol
    ref = g["grad_student"].double()
    assert torch.isfinite(grad).all() and ref.abs().max() > 0
    if case == "same_layer":          # the gradient vanishes analytically; what is left in the fp32 reference is its rounding of (t^ - c s^)
        assert abs(logs["layersync_similarity"] - 1.0) <= tol and grad.abs().max() <= 1e-12 and ref.abs().max() <= tol * g["weight"] / ref.shape[0]
        return
    rows_scale = ref.abs().amax(dim=-1, keepdim=True)
    assert ((grad - ref).abs() <= tol * rows_scale).all(), ((grad - ref).abs() / rows_scale.clamp_min(1e-300)).max().item()
    if case == "zero_rows":
        (b0, r0), (b1, r1) = g["zero_student_row"], g["zero_teacher_row"]
        assert ref[b0, r0].abs().max() > 1e8 and grad[b0, r0].abs().max() > 1e8 and ref[b1, r1].abs().max() == 0 and grad[b1, r1].abs().max() == 0


def test_index_resolution_and_error_texts_equal_the_executed_reference(golden):
    from simpletuner_amd.foundation import ModelFoundation as MF
    n = golden["n_layers"]
    for (si, ti), (s_ref, t_ref) in golden["index_table"].items():
        for resolve in (LS.resolve_layer, MF._layersync_resolve):
            assert resolve(si, "student", n) == s_ref and resolve(ti if ti is not None else si, "teacher", n) == t_ref, (si, ti)
    e = golden["errors"]
    for resolve in (LS.resolve_layer, MF._layersync_resolve):
        for key, call in (("negative_index", lambda: resolve(-1, "student", n)), ("not_an_int", lambda: resolve("three", "teacher", n)),
                          ("out_of_range", lambda: resolve(n + 2, "teacher", n)), ("none_index", lambda: resolve(None, "student", n))):
            with pytest.raises(ValueError) as ei:
                call()
            assert str(ei.value) == e[key], key
    assert golden["default_lambda"] == 0.2 and golden["lambda_zero_means_default"] == 0.2


# ------------------------------------------------------------------------------------------------
# (b) plugin / trainer surface
# ------------------------------------------------------------------------------------------------
def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    LS.install(monkeypatch)
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
        plugin.load_model(**SH._arch(3))
    return plugin


@pytest.mark.parametrize("family,n_blocks", [("flux", 4), ("sd3", 3)])
def test_post_model_load_setup_accepts_layersync_for_flux_and_sd3(monkeypatch, golden, family, n_blocks):
    plugin = _plugin(monkeypatch, family, layersync_enabled=True, layersync_student_block=2, layersync_teacher_block=3)
    plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    assert comp._layersync == (1, 2) and plugin.layersync.weight == 0.2          # 1-based depths; lambda defaults to the paper's 0.2
    plugin = _plugin(monkeypatch, family, layersync_enabled=True, layersync_student_block=0, layersync_lambda=0.5)
    plugin.post_model_load_setup()
    assert plugin.get_trained_component()._layersync == (0, 0) and plugin.layersync.weight == 0.5          # teacher unset: the student's own layer
    e = golden["errors"]
    for kw, text in ((dict(), e["no_student"]), (dict(layersync_student_block=1, layersync_lambda=-0.5), e["bad_lambda"]),
                     (dict(layersync_student_block=-1), e["negative_index"]),
                     (dict(layersync_student_block=n_blocks + 2), f"LayerSync could not find student layer at indices [{n_blocks + 1}, {n_blocks + 2}].")):
        with pytest.raises(ValueError) as ei:
            _plugin(monkeypatch, family, layersync_enabled=True, **kw).post_model_load_setup()
        assert str(ei.value) == text
    with pytest.raises(ValueError, match="must not lie below the student"):
        _plugin(monkeypatch, family, layersync_enabled=True, layersync_student_block=3, layersync_teacher_block=1).post_model_load_setup()
    with pytest.raises(ValueError, match="out of range"):
        plugin.get_trained_component().set_layersync(0, n_blocks)
    # off: nothing is set, the forward returns one output, auxiliary_loss passes the loss through
    plugin = _plugin(monkeypatch, family)
    plugin.post_model_load_setup()
    assert plugin.layersync is None and plugin.get_trained_component()._layersync is None
    loss = torch.tensor(1.5)
    assert plugin.auxiliary_loss({"model_prediction": None}, {}, loss) == (loss, None)


@pytest.mark.parametrize("flag", ["crepa_enabled", "irepa_enabled", "urepa_enabled", "internal_guidance_enabled", "nextlat_enabled"])
def test_the_other_regularisers_are_still_refused_by_name(monkeypatch, flag):
    with pytest.raises(NotImplementedError, match=flag):
        _plugin(monkeypatch, "flux", **{flag: True}).post_model_load_setup()


def test_layersync_is_refused_for_pixart_and_the_unets(monkeypatch):
    from simpletuner_amd.pixart.model import PixartSigma
    from simpletuner_amd.pixart.transformer import PixArtTransformer2DModel
    from simpletuner_amd.sdxl.model import SDXL
    from tests import test_pixart_host_sequencing_cpu as PH
    from tests import test_unet_host_sequencing_cpu as UH
    LS.install(monkeypatch)
    unet, _ = UH._unet(monkeypatch, "sdxl_small", 3)
    for cls, comp in ((PixartSigma, PixArtTransformer2DModel(device="cpu", **PH.ARCH)), (SDXL, unet)):
        plug = cls.__new__(cls)
        plug.config, plug.accelerator, plug.model, plug.controlnet = SimpleNamespace(layersync_enabled=True, layersync_student_block=1), _acc(), comp, None
        with pytest.raises(NotImplementedError, match="layersync_enabled: LayerSync is not built for"):
            plug.post_model_load_setup()


def test_tread_hip_graph_tiny_and_tokenwise_combinations_are_refused_by_name(monkeypatch):
    from simpletuner_amd.training.trainer import Trainer
    routes = {"routes": [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": 2}]}
    with pytest.raises(NotImplementedError, match="layersync_enabled with TREAD routing"):
        _plugin(monkeypatch, "flux", layersync_enabled=True, layersync_student_block=1, tread_config=routes).post_model_load_setup()
    # a router handed to the component directly: refused by the engine at the training forward
    for family in ("flux", "sd3"):
        plugin = _plugin(monkeypatch, family, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=2)
        plugin.add_lora_adapter()
        plugin.post_model_load_setup()
        comp = plugin.get_trained_component()
        comp.set_router(object(), routes["routes"])
        d = FH._inputs(2, 16, 8, 24) if family == "flux" else SH._inputs(2, 16, 24, 33)
        run = (lambda: _flux_hip(comp, d, 0.2)) if family == "flux" else (lambda: _sd3_hip(comp, d, 0.2))
        with pytest.raises(NotImplementedError, match="LayerSync under TREAD routing"):
            run()
        comp.set_router(None, None)
        tok = dict(d, t=d["t"][:, None].expand(-1, (16 // 2) * ((8 if family == "flux" else 24) // 2)).contiguous())
        run = (lambda: _flux_hip(comp, tok, 0.2)) if family == "flux" else (lambda: _sd3_hip(comp, tok, 0.2))
        with pytest.raises(NotImplementedError, match="LayerSync with tokenwise timesteps"):
            run()
    plugin = _plugin(monkeypatch, "flux", layersync_enabled=True, layersync_student_block=1, hip_graph=True)
    plugin.add_lora_adapter()
    with pytest.raises(NotImplementedError, match="hip_graph: LayerSync"):
        Trainer(plugin.config, plugin, plugin.accelerator)
    # 'tiny': adapters on single blocks 7 and 20 only — the backward stops at single block 7, a student below it would never be reached
    model = _flux_model(monkeypatch, 1, 21)
    model.add_lora_adapter(rank=4, targets="tiny")
    model.set_layersync(2, 9)
    with pytest.raises(NotImplementedError, match="LayerSync: student block 2 lies below the first block that carries an adapter"):
        _flux_hip(model, FH._inputs(1, 8, 8, 24), 0.2)


def test_train_step_adds_the_regulariser_and_keeps_its_logs(monkeypatch):
    """Trainer.train_step: loss = mse - lambda * similarity, the logs as floats in `last_aux_logs` (layersync.py:55-58), the similarity from the engine's tap"""
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, "flux", layersync_enabled=True, layersync_student_block=2, layersync_teacher_block=4, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    mse, _ = plugin.loss_with_logs(prepared, pred)
    total, logs = plugin.auxiliary_loss(pred, prepared, mse)
    sim = pred["layersync_similarity"]
    assert set(logs) == {"layersync_loss", "layersync_similarity"} and all(isinstance(v, float) for v in logs.values())
    assert logs["layersync_similarity"] == sim.item() and abs(logs["layersync_loss"] + 0.2 * sim.item()) < 1e-7
    assert abs(total.item() - (mse.item() - 0.2 * sim.item())) < 1e-6 and 0.0 < sim.item() < 1.0
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - total.item()) < 1e-6 and trainer.last_aux_logs == logs
    with torch.no_grad():          # a prediction outside training carries no similarity: the regulariser cannot be evaluated on it
        with pytest.raises(ValueError, match="no hidden state buffer"):
            plugin.auxiliary_loss(plugin.model_predict(prepared), prepared, mse)


# ------------------------------------------------------------------------------------------------
# (d) with LayerSync off the engines launch what they launched before
# ------------------------------------------------------------------------------------------------
def test_launch_stream_without_layersync_is_the_recorded_one(tmp_path):
    """tools/launch_trace.py over the Flux and SD3 LoRA host-sequencing tests: the digest of its output was recorded at the commit before LayerSync
    (tests/golden/layersync_launch_trace.sha256) — every emulated launch, its operands' dtypes, shapes and strides, in order"""
    import hashlib
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, str(root / "tools" / "launch_trace.py"), str(out), "-k", "test_lora_path_through_the_emulator_matches_the_oracle"],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = (root / "tests" / "golden" / "layersync_launch_trace.sha256").read_text().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

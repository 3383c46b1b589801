"""Self-Transcendence (distillation_method=self_transcendence) on the CPU: the fp64 restatement against the executed reference
(tests/golden/self_transcendence_vectors.pt), the stand-ins inside the kernels' derived bounds, the configuration surface with the reference's texts, the SD3 engine
on the emulator against autograd through the oracle, and Trainer.train_step in both stages."""
import hashlib
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import layersync_ref as LS
from tests import parity_utils as PU
from tests import self_transcendence_bounds as TB
from tests import self_transcendence_ref as ST
from tests import test_sd3_host_sequencing_cpu as SH

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "self_transcendence_vectors.pt"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PRE = ST.PREFIX
# the fp64 restatement against the executed reference's fp32 records: the reference's own arithmetic is fp32 (projector, MSE, mean).  Its size is MEASURED by
# tools/gen_self_transcendence_golden.py as the relative distance (loss, dh, every parameter gradient) between the reference run in fp32 and the same class run in
# fp64, recorded per case as `fp32_vs_fp64`: worst 2.6e-7.  The restatement is held to about four times that, everywhere
REF_TOL = 1e-6
# the engine step at the GPU test's shapes (_arch(3), SH._inputs(2, 16, 24, 33), Hp 128, weights W_GUIDE): the stand-ins' worst projector-gradient rel-L2 against
# the oracle, measured here on the CPU (printed by test_sd3_engine_with_self_transcendence_matches_autograd_through_the_oracle); the GPU test allows twice this
PROJECTOR_GRAD_REL_CPU = {"vae": 5.2e-3, "self": 4.0e-3}          # measured: 5.19e-3 (vae, student 1), 3.92e-3 (self, student 1)
W_GUIDE = {"vae": 4.0, "self": 0.2}          # the guide weight of the engine tests: the regulariser's share of the adapters' gradient >= 0.1 in both stages
HP = 128
TMIN, TMAX = 0.4, 0.7
SIGMAS = torch.tensor([0.55, 0.9])          # one sample inside the range, one outside


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


# ------------------------------------------------------------------------------------------------
# (a) the restatement equals the executed reference
# ------------------------------------------------------------------------------------------------
def test_normalisation_and_every_value_error_equal_the_executed_reference(golden):
    from simpletuner_amd import self_transcendence as M
    for rec in golden["normalize"]:
        if rec["error"] is None:
            assert M.normalized_config(rec["config"]) == rec["normalized"], rec["config"]
        else:
            with pytest.raises(ValueError) as e:
                M.normalized_config(rec["config"])
            assert str(e.value) == rec["error"], rec["config"]
    assert M.normalized_config({"student_block": 1}) == {**M.DEFAULTS, "student_block": 1}
    for rec in golden["requirements"]:
        assert M.training_batch_requirements(rec["config"]) == rec["requirements"]


def test_factor_grid_and_target_tokens_equal_the_executed_reference(golden):
    from simpletuner_amd.engine import self_transcendence_grid
    for rec in golden["factor_grid"]:
        if rec["error"] is None:
            assert tuple(self_transcendence_grid(rec["shape"], rec["tokens"])) == tuple(rec["grid"]) == tuple(ST.factor_grid64(rec["shape"], rec["tokens"])), rec
        else:
            for fn in (self_transcendence_grid, ST.factor_grid64):
                with pytest.raises(ValueError) as e:
                    fn(rec["shape"], rec["tokens"])
                assert str(e.value) == rec["error"]
    assert any(r["error"] is not None for r in golden["factor_grid"]) and any(r["grid"] is not None and r["grid"][0] != r["grid"][1] for r in golden["factor_grid"])
    for rec in golden["target_tokens"]:
        assert torch.equal(ST.vae_target_tokens64(rec["latents"], rec["tokens"]).float(), rec["out"].float())


@pytest.mark.parametrize("case", ["vae", "vae_slice", "self", "self_cfg1", "none_active", "inclusive_ends"])
def test_loss_restatement_equals_the_executed_reference(golden, case):
    rec = golden["loss"][case]
    params = tuple(rec["params"][nm] for nm in ST.NAMES)
    if rec["stage"] == "vae":
        tokens = ST.vae_target_tokens64(rec["target"], rec["hidden"].shape[1])
    else:
        tokens = ST.cfg_target64(rec["cond"], rec["uncond"], rec["cfg_scale"])
    r = ST.loss64(rec["hidden"], params, tokens, rec["sigmas"], rec["timestep_min"], rec["timestep_max"], weight=rec["weight"])
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert abs(r["guide"].item() - rec["guide"]) <= REF_TOL * max(abs(rec["guide"]), 1e-30) and r["n"] == rec["n_active"]
    assert abs((rec["original"] + rec["weight"] * r["guide"].item()) - rec["loss_out"]) <= REF_TOL * abs(rec["loss_out"])
    assert list(rec["logs"]) == (["self_transcendence/loss", "self_transcendence/weight"] + (["self_transcendence/teacher_cfg_scale"] if rec["stage"] == "self" else []))
    assert abs(rec["logs"]["self_transcendence/loss"] - r["guide"].item()) <= REF_TOL * max(abs(rec["guide"]), 1e-30)
    if rec["n_active"] == 0:
        assert r["guide"].item() == 0.0 == rec["guide"] and all(float(g.abs().max()) == 0.0 for g in rec["grads"].values()) and float(r["dh"].abs().max()) == 0.0
        return
    assert rel(r["dh"], rec["dh"]) <= REF_TOL
    for nm in ST.NAMES:
        assert rel(r["grads"][nm], rec["grads"][nm]) <= REF_TOL, nm
    assert rec["fp32_vs_fp64"] <= REF_TOL / 3          # where the tolerance comes from: the reference's own fp32 arithmetic against itself in fp64


def test_stop_step_branch_and_its_logs_equal_the_executed_reference(golden):
    rec = golden["stop_step"]
    assert rec["logs"] == {"self_transcendence/loss": 0.0, "self_transcendence/weight": 0.0} and rec["loss_out"] == rec["original"]
    assert all(float(g.abs().max()) == 0.0 for g in rec["grads"].values())
    assert rec["step_counter"] == "trainer.py:6876 step = state['global_step']; :6955 step += 1 per fetched batch; :7000 pre_training_step(model, step)"


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins lie inside the derived bounds (the cases of the GPU tests)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TB.VAE_CASES, ids=lambda c: c["id"])
def test_vae_loss_stand_in_stays_inside_the_derived_bounds(case):
    TB.check_vae_loss(ST.st_vae_loss, case, "cpu")


@pytest.mark.parametrize("case", TB.CFG_CASES, ids=lambda c: c["id"])
def test_cfg_loss_stand_in_stays_inside_the_derived_bounds(case):
    TB.check_cfg_loss(ST.st_cfg_loss, case, "cpu")


@pytest.mark.parametrize("case", TB.FOLD_CASES, ids=lambda c: c["id"])
def test_fold_stand_in_stays_inside_the_derived_bounds(case):
    TB.check_fold(ST.st_fold, case, "cpu")


@pytest.mark.parametrize("case", TB.WGRAD_CASES, ids=lambda c: c["id"])
def test_wgrad_stand_in_stays_inside_the_derived_bounds(case):
    TB.check_wgrad(ST.st_wgrad, case, "cpu")


@pytest.mark.parametrize("case", TB.DX_CASES, ids=lambda c: c["id"])
def test_dx_add_stand_in_stays_inside_the_derived_bounds(case):
    TB.check_dx_add(ST.st_dx_add, case, "cpu")


def test_the_bounds_reject_a_planted_error():
    """a checker that accepts everything checks nothing: one element of G off by two bf16 ulps, and a loss off by 1e-4 relative, are both caught"""
    def bad_g(pred, *a):
        out = ST.st_vae_loss(pred, *a)
        flat = pred.view(-1)
        i = int(flat.float().abs().argmax())
        flat[i] = (flat[i].float() * (1 + 2.0 ** -6)).to(BF16)
        return out

    def bad_loss(pred, target, grid, sigmas, tmin, tmax, per_sample, stats):
        out = ST.st_vae_loss(pred, target, grid, sigmas, tmin, tmax, per_sample, stats)
        stats[0] *= 1 + 1e-4
        return out

    for bad in (bad_g, bad_loss):
        with pytest.raises(AssertionError):
            TB.check_vae_loss(bad, TB.VAE_CASES[0], "cpu")


def test_abi_exports_the_self_transcendence_symbols():
    from simpletuner_amd import lib
    names = ["st355_st_fold", "st355_st_loss_workspace", "st355_st_vae_loss", "st355_st_cfg_loss", "st355_st_wgrad", "st355_st_dx_add"]
    header = (ROOT / "include" / "st355.h").read_text()
    for n in names:
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    assert "self_transcendence.hip" in (ROOT / "simpletuner_amd" / "csrc" / "Makefile").read_text()
    if lib.is_built():
        L = lib.load()
        assert all(hasattr(L, n) for n in names)


# ------------------------------------------------------------------------------------------------
# (c) host sequencing: guide loss and every gradient against autograd through the oracle
# ------------------------------------------------------------------------------------------------
def sd3_model(install, monkeypatch, layers, stage, student, teacher, dev="cpu", arch=SH._arch, seed=11, hp=HP):
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
    model.set_self_transcendence(stage, student, teacher, hp, TMIN, TMAX, 3.0)
    model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    ST.seed_projector(model)
    return model


def snapshot_of(model, seed=5):
    """a teacher snapshot that differs from the masters"""
    g = torch.Generator().manual_seed(seed)
    return (model.lora_flat.detach().cpu() + 0.01 * torch.randn(model.lora_flat.shape, generator=g)).to(model.lora_flat.device)


def teacher_capture(model, d, snapshot, block, neg_prompt, neg_pooled):
    """ONE no-grad forward at batch 2B: conditional rows, then unconditional rows"""
    dev = model.lora_flat.device
    two = lambda a, b: torch.cat([a, b], dim=0).to(dev)
    with torch.no_grad(), model.teacher_values(snapshot):
        res = model(hidden_states=two(d["lat"], d["lat"]), encoder_hidden_states=two(d["prompt"], neg_prompt), pooled_projections=two(d["pooled"], neg_pooled),
                    timestep=two(d["t"], d["t"]), crepa_capture_block_index=block)
    assert res.sample is None
    return res.crepa_hidden_states


def negatives(d, seed=41):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(d["prompt"].shape, generator=g)).to(BF16), (0.5 * torch.randn(d["pooled"].shape, generator=g)).to(BF16)


def record_tap_dx(monkeypatch):
    from simpletuner_amd import engine as E
    seen, inner = {}, E.SelfTranscendenceTap.backward

    def backward(self, dg, dx_view, accumulate=False, sync=None):
        if dx_view is not None:
            seen["before"] = dx_view.detach().float().cpu().clone()
        inner(self, dg, dx_view, accumulate, sync)
        if dx_view is not None:
            seen["after"] = dx_view.detach().float().cpu().clone()

    monkeypatch.setattr(E.SelfTranscendenceTap, "backward", backward)
    return seen


def hip_side(model, d, target, sigmas, weight):
    dev = model.lora_flat.device
    res = model(hidden_states=d["lat"].to(dev), encoder_hidden_states=d["prompt"].to(dev), pooled_projections=d["pooled"].to(dev), timestep=d["t"].to(dev),
                self_transcendence_target=target, self_transcendence_sigmas=sigmas.to(dev), return_dict=True)
    out, guide = res.sample, getattr(res, ST.KEY)
    assert guide.dim() == 0 and guide.dtype == F32 and guide.requires_grad
    loss = ((out.float() - d["target"].to(dev).float()) ** 2).mean() + weight * guide
    loss.backward()
    return out.detach().cpu(), loss.detach().cpu(), guide.detach().cpu()


def engine_step(monkeypatch, install, stage, student, teacher=2, dev="cpu", layers=3, arch=SH._arch, sigmas=SIGMAS):
    """one SD3 LoRA step with the guide loss, engine against oracle: (model, hip, oracle, seen)"""
    model = sd3_model(install, monkeypatch, layers, stage, student, teacher, dev=dev, arch=arch)
    d = SH._inputs(2, 16, 24, 33)
    w = W_GUIDE[stage]
    _, lora, scale = PU.oracle_state(model)
    if stage == "vae":
        target_hip = d["target"].to(dev)
        target_ref = d["target"].float()
    else:
        masters = model.lora_flat.clone()
        cap = teacher_capture(model, d, snapshot_of(model), teacher, *negatives(d))
        assert torch.equal(masters, model.lora_flat) and tuple(cap.shape) == (4, 96, model.D) and cap.dtype == BF16
        target_hip = cap
        target_ref = (cap[:2].float().cpu(), cap[2:].float().cpu())
    seen = record_tap_dx(monkeypatch)
    hip = hip_side(model, d, target_hip, sigmas, w)
    oracle = ST.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, student, w, stage, target_ref, sigmas, TMIN, TMAX, 3.0, lora=lora, scale=scale)
    return model, hip, oracle, seen


def check_step(model, hip, oracle, seen, proj_rel, below_first=False):
    """the thresholds of tests/test_nextlat_gpu.py's SD3 step: prediction rel-L2 < 2e-2 and cosine > 0.9995, |loss difference| < 1e-3 max(1, |loss|) (the loss
    holds weight x the guide loss), adapters check_lora_grads(5e-2, cos 0.999); the projector's six gradients below `proj_rel`"""
    out, loss, guide = hip
    o_out, o_loss, o_guide, lp, head, dh, share = oracle
    assert PU.rel_l2(out, o_out) < 2e-2 and PU.cos_sim(out, o_out) > 0.9995 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))
    assert share >= 0.1, share          # dropping the injection would miss the gradient tolerances by a wide margin
    worst = LS.check_lora_grads(model, lp, 5e-2, 0.999)
    own = dict(model.named_parameters())
    rg = max(PU.rel_l2(own[PRE + nm].grad, head[nm].grad) for nm in ST.NAMES)
    cg = min(PU.cos_sim(own[PRE + nm].grad, head[nm].grad) for nm in ST.NAMES)
    assert rg <= proj_rel and cg > 0.999, f"projector gradients: rel={rg:.3e} cos={cg:.5f}"
    if not below_first:
        got, ref = (seen["after"] - seen["before"]).reshape(dh.shape), dh.float()
        assert ref.norm() > 0 and (got - ref).norm() <= 2.0 ** -9 * seen["after"].norm() + 2.0 ** -6 * ref.norm(), ((got - ref).norm().item(), ref.norm().item())
    return share, worst, rg


@pytest.mark.parametrize("stage,student", [("vae", 0), ("vae", 1), ("self", 1), ("self", 0)])
def test_sd3_engine_with_self_transcendence_matches_autograd_through_the_oracle(monkeypatch, stage, student):
    model, hip, oracle, seen = engine_step(monkeypatch, ST.install, stage, student)
    share, worst, rg = check_step(model, hip, oracle, seen, PROJECTOR_GRAD_REL_CPU[stage])
    print(f"[emu] sd3 self-transcendence {stage} student {student}: share={share:.3e}, adapters rel-L2={worst:.3e}, projector rel-L2={rg:.3e}")
    if stage == "vae":          # the columns of the last Linear that are not read: gradient exactly zero
        own = dict(model.named_parameters())
        assert float(own[PRE + "net.4.weight"].grad[64:].abs().max()) == 0.0 and float(own[PRE + "net.4.bias"].grad[64:].abs().max()) == 0.0


@pytest.mark.parametrize("ckpt", ["per-block", "segmented"])
def test_gradient_checkpointing_runs_the_tap_once_in_the_saving_forward(monkeypatch, ckpt):
    def install(mp):
        ST.install(mp)
        from simpletuner_amd.sd3 import transformer as T
        inner = T.SD3Transformer2DModel.add_lora_adapter

        def add(self, *a, **k):
            out = inner(self, *a, **k)
            self.enable_gradient_checkpointing()
            if ckpt == "segmented":
                self.set_gradient_checkpointing_interval(2)
            return out

        mp.setattr(T.SD3Transformer2DModel, "add_lora_adapter", add)

    model, hip, oracle, seen = engine_step(monkeypatch, install, "vae", 1)
    assert model.gradient_checkpointing
    check_step(model, hip, oracle, seen, PROJECTOR_GRAD_REL_CPU["vae"])


@pytest.mark.parametrize("stage", ["vae", "self"])
def test_sd35_dual_attention_blocks_take_the_tap(monkeypatch, stage):
    arch = lambda layers: SH._arch(layers, qk_norm="rms_norm", dual=(0, 1))
    model, hip, oracle, seen = engine_step(monkeypatch, ST.install, stage, 1, arch=arch)
    check_step(model, hip, oracle, seen, 2 * PROJECTOR_GRAD_REL_CPU[stage])


def test_no_active_sample_gives_zero_loss_and_zero_gradient(monkeypatch):
    model = sd3_model(ST.install, monkeypatch, 3, "vae", 1, None)
    d = SH._inputs(2, 16, 24, 33)
    _, _, guide = hip_side(model, d, d["target"], torch.tensor([0.1, 0.9]), 4.0)
    h = model._st
    assert guide.item() == 0.0 and float(model.lora_grad_flat[h.flat_lo:h.flat_hi].abs().max()) == 0.0 and float(model.lora_grad_flat[:h.flat_lo].abs().max()) > 0
    plain = sd3_model(None, monkeypatch, 3, "vae", 1, None)
    plain._st_cfg = None
    out = plain(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"]).sample
    ((out.float() - d["target"].float()) ** 2).mean().backward()
    assert torch.allclose(model.lora_grad_flat[:h.flat_lo], plain.lora_grad_flat[:h.flat_lo], rtol=0, atol=0)


def test_gradient_accumulation_adds_the_projector_gradients(monkeypatch):
    model = sd3_model(ST.install, monkeypatch, 3, "vae", 1, None)
    d = SH._inputs(2, 16, 24, 33)
    hip_side(model, d, d["target"], SIGMAS, 4.0)
    once = model.lora_grad_flat.clone()
    model.accumulate_lora_grads = True
    hip_side(model, d, d["target"], SIGMAS, 4.0)
    lo, hi = model._st.flat_lo, model._st.flat_hi
    assert once[lo:hi].abs().max() > 0 and torch.allclose(model.lora_grad_flat[lo:hi], 2 * once[lo:hi], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------
# (d) the plugin, the distiller and Trainer.train_step
# ------------------------------------------------------------------------------------------------
def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _dcfg(stage="vae", **kw):
    base = {"stage": stage, "student_block": 1, "projector_hidden_dim": HP, "weight": 0.5}
    if stage == "self":
        base.update(teacher_block=2, cfg_scale=3.0)
    base.update(kw)
    return {"self_transcendence": base}


def _plugin(monkeypatch, family="sd3", layers=3, stage="vae", dkw=None, method="self_transcendence", **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    ST.install(monkeypatch)
    extra = dict(distillation_method=method, distillation_config=_dcfg(stage, **(dkw or {}))) if method else {}
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, **extra, **cfg_kw)
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


def _setup(plugin):
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return plugin


def _trainer(monkeypatch, stage="vae", dkw=None, seed_projector=True, method="self_transcendence", **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _setup(_plugin(monkeypatch, stage=stage, dkw=dkw, method=method, **{"lora_rank": 8, "lora_init_b_std": 0.02, "learning_rate": 1e-3, **cfg_kw}))
    if seed_projector and method:
        ST.seed_projector(plugin.get_trained_component())
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    sig = torch.tensor([0.55, 0.9])
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    if stage == "self":
        g = torch.Generator().manual_seed(19)
        batch["negative_prompt_embeds"] = (0.5 * torch.randn(devt["prompt"].shape, generator=g)).to(BF16)
        batch["negative_add_text_embeds"] = (0.5 * torch.randn(devt["pooled"].shape, generator=g)).to(BF16)
    return plugin, trainer, batch, sig


@pytest.mark.parametrize("stage", ["vae", "self"])
def test_self_transcendence_adds_its_logs_and_changes_the_loss(monkeypatch, stage):
    """two Trainer.train_steps: the two (stage `vae`) or three (stage `self`) log keys with the reference's values — the guide loss is the masked per-sample MSE of
    the fp64 restatement on the recorded student block, the weight the configured one — and a loss that differs from the plain run's.  (On the parent commit the
    Trainer's construction raises NotImplementedError: distillation_method=self_transcendence: not built on the st355 path (built: flow_dpo).)"""
    from simpletuner_amd import engine as E
    plugin, trainer, batch, sig = _trainer(monkeypatch, stage)
    seen, inner = {}, E.SelfTranscendenceTap.tap

    def tap(self, g, view):
        if g == self.block and not self.off:
            seen["h"], seen["target"] = view.detach().float().clone(), self.target.detach().float().clone()
        inner(self, g, view)

    monkeypatch.setattr(E.SelfTranscendenceTap, "tap", tap)
    comp = plugin.get_trained_component()
    own = dict(comp.named_parameters())
    losses, keys = [], ["self_transcendence/loss", "self_transcendence/weight"] + (["self_transcendence/teacher_cfg_scale"] if stage == "self" else [])
    for step in range(2):
        params = tuple(own[PRE + nm].detach().clone() for nm in ST.NAMES)
        losses.append(trainer.train_step(dict(batch)).item())
        logs = trainer.last_aux_logs
        assert [k for k in logs if k.startswith("self_transcendence/")] == keys and logs["self_transcendence/weight"] == 0.5
        if stage == "self":
            assert logs["self_transcendence/teacher_cfg_scale"] == 3.0
            tokens = ST.cfg_target64(seen["target"][:2], seen["target"][2:], 3.0)
        else:
            tokens = ST.vae_target_tokens64(seen["target"], seen["h"].shape[1])
        want = ST.loss64(seen["h"], params, tokens, sig, TMIN, TMAX)["guide"].item()
        assert abs(logs["self_transcendence/loss"] - want) < 2e-2 * want and want > 0
    assert trainer.state["global_step"] == 2
    plain_plugin, plain, pbatch, _ = _trainer(monkeypatch, stage, method=None)
    plain_losses = [plain.train_step(dict(pbatch)).item() for _ in range(2)]
    assert all(abs(a - b) > 1e-3 for a, b in zip(losses, plain_losses)), (losses, plain_losses)
    assert not any(k.startswith("self_transcendence/") for k in (plain.last_aux_logs or {}))


def test_teacher_snapshot_is_frozen_and_the_masters_survive_the_teacher_forward(monkeypatch):
    plugin, trainer, batch, _ = _trainer(monkeypatch, "self")
    comp = plugin.get_trained_component()
    assert trainer.distiller.snapshot is None
    start = comp.lora_flat.clone()
    trainer.train_step(dict(batch))
    snap = trainer.distiller.snapshot
    assert torch.equal(snap, start) and snap.data_ptr() != comp.lora_flat.data_ptr()          # taken at the first pre_training_step, before any update
    trainer.train_step(dict(batch)); trainer.train_step(dict(batch))
    assert torch.equal(trainer.distiller.snapshot, start) and not torch.equal(comp.lora_flat, start)          # ... and never updated
    masters = comp.lora_flat.clone()
    prepared = plugin.prepare_batch(dict(batch), dict(trainer.state))
    cap = trainer.distiller.teacher_capture(plugin, prepared)
    assert torch.equal(masters, comp.lora_flat) and tuple(cap.shape) == (4, prepared['latents'].shape[2] * prepared['latents'].shape[3] // 4, comp.D)          # bit-identical before and after a teacher forward
    with pytest.raises(ValueError) as e:
        trainer.distiller.teacher_capture(plugin, {k: v for k, v in prepared.items() if not k.startswith("negative_")})
    assert str(e.value) == "Self-Transcendence self stage requires cached empty-prompt embeddings."


def test_teacher_adapter_path_round_trips_and_raises_the_named_errors(monkeypatch, tmp_path, caplog):
    plugin, trainer, batch, _ = _trainer(monkeypatch, "self")
    trainer.train_step(dict(batch))
    trainer.save_state(str(tmp_path / "ck"))
    path = str(tmp_path / "ck" / "pytorch_lora_weights.safetensors")
    saved = plugin.get_trained_component().lora_flat.clone()
    plugin2, trainer2, batch2, _ = _trainer(monkeypatch, "self", dkw={"teacher_adapter_path": path})
    comp2 = plugin2.get_trained_component()
    live = comp2.lora_flat.clone()
    trainer2.distiller.pre_training_step(plugin2, 1)
    snap, h = trainer2.distiller.snapshot, comp2._st
    assert torch.equal(comp2.lora_flat, live)                                                       # the live student values stay untouched
    from safetensors.torch import load_file, save_file
    f = load_file(path)
    for n, p in comp2.named_parameters():
        if ".lora_" in n:
            k = "transformer." + n.replace(".default.", ".")
            lo = (p.data_ptr() - comp2.lora_flat.data_ptr()) // 4
            assert torch.equal(snap[lo:lo + p.numel()].view(p.shape), f[k].float())
    assert not torch.equal(snap[:h.flat_lo], live[:h.flat_lo])
    # the named errors
    _, t3, _, _ = _trainer(monkeypatch, "self", dkw={"teacher_adapter_path": str(tmp_path / "nope.safetensors")})
    with pytest.raises(FileNotFoundError) as e:
        t3.distiller.pre_training_step(None, 1)
    assert str(e.value) == f"Self-Transcendence teacher adapter does not exist: {tmp_path / 'nope.safetensors'}"
    keys = sorted(k for k in f if ".lora_" in k)
    cut = {k: v for k, v in f.items() if k != keys[0]}
    cut["transformer.extra.tensor"] = torch.zeros(2)
    save_file(cut, str(tmp_path / "cut.safetensors"))
    _, t4, _, _ = _trainer(monkeypatch, "self", dkw={"teacher_adapter_path": str(tmp_path / "cut.safetensors")})
    with pytest.raises(ValueError) as e:
        t4.distiller.pre_training_step(None, 1)
    assert str(e.value) == f"Self-Transcendence teacher adapter is missing required tensors: {keys[0][len('transformer.'):]}"
    full = dict(f)
    full["transformer.extra.tensor"] = torch.zeros(2)
    save_file(full, str(tmp_path / "more.safetensors"))
    _, t5, _, _ = _trainer(monkeypatch, "self", dkw={"teacher_adapter_path": str(tmp_path / "more.safetensors")})
    with caplog.at_level("WARNING", logger="SelfTranscendenceDistiller"):
        t5.distiller.pre_training_step(None, 1)
    assert any("Self-Transcendence teacher adapter contains unused tensors: " in r.getMessage() and "extra.tensor" in r.getMessage() for r in caplog.records)


def _trace(monkeypatch, fn):
    """the names of every simpletuner_amd.ops wrapper called inside fn, in order"""
    from simpletuner_amd import ops
    calls = []
    for name in dir(ops):
        f = getattr(ops, name)
        if callable(f) and not name.startswith("_") and getattr(f, "__module__", "").startswith(("tests.", "simpletuner_amd.ops")) and not isinstance(f, type):
            def wrap(*a, _f=f, _n=name, **k):
                calls.append(_n)
                return _f(*a, **k)
            monkeypatch.setattr(ops, name, wrap)
    fn()
    return calls


@pytest.mark.parametrize("stage", ["vae", "self"])
def test_a_step_past_stop_step_launches_what_the_plain_step_launches(monkeypatch, stage):
    plugin, trainer, batch, _ = _trainer(monkeypatch, stage, dkw={"stop_step": 2})
    comp = plugin.get_trained_component()
    h = comp._st
    trainer.train_step(dict(batch))                      # loop step 1 < stop_step: active
    assert trainer.last_aux_logs["self_transcendence/weight"] == 0.5 and trainer.last_aux_logs["self_transcendence/loss"] > 0
    plain_plugin, plain, pbatch, _ = _trainer(monkeypatch, stage, method=None)
    plain.train_step(dict(pbatch))
    with monkeypatch.context() as mp:
        got = _trace(mp, lambda: trainer.train_step(dict(batch)))          # loop step 2 >= stop_step: weight 0
    assert trainer.last_aux_logs["self_transcendence/weight"] == 0.0 and trainer.last_aux_logs["self_transcendence/loss"] == 0.0
    with monkeypatch.context() as mp:
        want = _trace(mp, lambda: plain.train_step(dict(pbatch)))
    assert got == want and len(got) > 20 and not any(n.startswith("st_") for n in got)
    # the gradient views of the projector were zeroed: AdamW's decay and the moments of step 1 alone move it
    head = comp.lora_flat[h.flat_lo:h.flat_hi].clone()
    prepared = plugin.prepare_batch(dict(batch), dict(trainer.state))
    pred = plugin.model_predict(prepared)
    loss, _ = plugin.loss_with_logs(prepared, pred)
    out, logs = trainer.distiller.compute_distill_loss(prepared, pred, loss)
    assert out is loss and logs == {"self_transcendence/loss": 0.0, "self_transcendence/weight": 0.0}
    loss.backward()
    assert float(comp.lora_grad_flat[h.flat_lo:h.flat_hi].abs().max()) == 0.0 and float(comp.lora_grad_flat[:h.flat_lo].abs().max()) > 0
    assert torch.equal(head, comp.lora_flat[h.flat_lo:h.flat_hi])


def test_save_and_resume_continue_bit_identically(monkeypatch, tmp_path):
    plugin, trainer, batch, _ = _trainer(monkeypatch, "vae")
    trainer.train_step(dict(batch))
    trainer.save_state(str(tmp_path / "ck"))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / "ck" / "pytorch_lora_weights.safetensors"))
    own = dict(plugin.get_trained_component().named_parameters())
    for nm in ST.NAMES:          # the projector travels with the adapter file under the reference's module name
        k = "transformer." + PRE + nm
        assert torch.equal(saved[k].float(), own[PRE + nm].detach().to(saved[k].dtype).float())
    assert sorted(k for k in saved if PRE in k) == sorted("transformer." + PRE + nm for nm in ST.NAMES)
    want = [trainer.train_step(dict(batch)).item() for _ in range(2)]
    want_w = plugin.get_trained_component().lora_flat.clone()
    plugin2, trainer2, _, _ = _trainer(monkeypatch, "vae")
    with torch.no_grad():
        plugin2.get_trained_component().lora_flat.add_(0.25)
    trainer2.load_state(str(tmp_path / "ck"))
    got = [trainer2.train_step(dict(batch)).item() for _ in range(2)]
    assert got == want and torch.equal(plugin2.get_trained_component().lora_flat, want_w)
    plain = _setup(_plugin(monkeypatch, method=None, lora_rank=8))
    with pytest.raises(ValueError, match="LoRA checkpoint carries a Self-Transcendence projector"):
        plain.load_lora_weights(input_dir=str(tmp_path / "ck"))


def test_projector_initial_values_are_nn_linear_defaults_behind_the_adapter_draws(monkeypatch):
    a = _setup(_plugin(monkeypatch, lora_rank=8)).get_trained_component()
    b = _setup(_plugin(monkeypatch, method=None, lora_rank=8)).get_trained_component()
    h = a._st
    assert torch.equal(a.lora_flat[:b.lora_flat.numel()][:h.flat_lo - 8], b.lora_flat[:h.flat_lo - 8])          # every A / B draw is unchanged
    assert h.flat_lo % 8 == 0 and h.flat_hi - h.flat_lo == sum(p.numel() for p in h.params) and all(p.dtype == F32 for p in h.params)
    for W, bias in ((h.W1, h.b1), (h.W2, h.b2), (h.W3, h.b3)):
        bound = 1.0 / W.shape[1] ** 0.5
        assert float(W.abs().max()) <= bound and float(bias.abs().max()) <= bound and float(W.abs().max()) > 0.9 * bound and float(W.std()) > 0.5 * bound
    names = [n for n, _ in a.named_parameters() if n.startswith(PRE)]
    assert names == [PRE + nm for nm in ST.NAMES]


# ------------------------------------------------------------------------------------------------
# (e) every refusal, by exact text
# ------------------------------------------------------------------------------------------------
def test_refusals_by_exact_text(monkeypatch):
    from simpletuner_amd.training.trainer import Trainer
    flag = "distillation_method=self_transcendence"
    tail = " is not built on the st355 path (built: SD3 LoRA)"

    def build(**kw):
        family, stage, dkw = kw.pop("family", "sd3"), kw.pop("stage", "vae"), kw.pop("dkw", None)
        plugin = _plugin(monkeypatch, family=family, stage=stage, dkw=dkw, lora_rank=8, **kw)
        if str(getattr(plugin.config, "model_type", "lora")) == "lora":
            plugin.add_lora_adapter()
        return Trainer(plugin.config, plugin, plugin.accelerator)

    with pytest.raises(NotImplementedError) as e:
        build(family="flux")
    assert str(e.value) == f"{flag} is not built for {e.value.args[0].split(' for ')[1].split(' on ')[0]} on the st355 path (built: SD3 LoRA)"
    cases = [
        (dict(use_dora=True), f"{flag} with use_dora (the teacher forward packs standard LoRA operands from the snapshot, which the DoRA fold does not take){tail}"),
        (dict(hip_graph=True), f"{flag} with hip_graph (the step reads its logs on the host every step and cannot be captured){tail}"),
        (dict(tread_config={"routes": [{"selection_ratio": 0.5, "start_layer_idx": 0, "end_layer_idx": 1}]}),
         f"{flag} with TREAD routing (the routed block's token count no longer matches the target's){tail}"),
        (dict(xm_noise_candidates_enabled=True), f"{flag} with XM noise candidates{tail}"),
        (dict(scheduled_sampling_max_step_offset=2),
         f"{flag} with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow: the rollout re-times the samples the mask reads){tail}"),
        (dict(twinflow_enabled=True), f"{flag} with twinflow_enabled{tail}"),
        (dict(controlnet=True), f"{flag} with controlnet{tail}"),
    ]
    from simpletuner_amd import self_transcendence as M
    from simpletuner_amd.sd3.model import SD3
    probe = SimpleNamespace(MODEL_TYPE=SD3.MODEL_TYPE, SELF_TRANSCENDENCE_BUILT=True, NAME="sd3", xm_config=None)
    base = dict(model_type="lora", lora_type="standard")
    for kw, text in cases:
        with pytest.raises(NotImplementedError) as e:
            M.refuse_unbuilt({**base, **kw}, probe)
        assert str(e.value) == text, kw
    for k, name in (("layersync_enabled", "LayerSync"), ("internal_guidance_enabled", "Internal Guidance"), ("nextlat_enabled", "NextLat")):
        with pytest.raises(NotImplementedError) as e:
            M.refuse_unbuilt({**base, k: True}, probe)
        assert str(e.value) == f"{flag} with {k} ({name} claims the same arena tail or tap order){tail}"
    with pytest.raises(NotImplementedError) as e:
        M.refuse_unbuilt({**base, "crepa_enabled": True}, probe)
    assert str(e.value) == f"{flag} with crepa_enabled (Self-Flow's tokenwise timesteps; the same arena tail){tail}"
    with pytest.raises(NotImplementedError) as e:
        M.refuse_unbuilt({**base, "model_type": "full"}, probe)
    assert str(e.value) == f"{flag} with model_type=full (a full fine-tune needs a separate frozen copy of the model as the teacher){tail}"
    for fam in ("flux", "pixart"):
        with pytest.raises(NotImplementedError) as e:
            M.refuse_unbuilt(base, SimpleNamespace(MODEL_TYPE=SD3.MODEL_TYPE, NAME=fam))
        assert str(e.value) == f"{flag} is not built for {fam} on the st355 path (built: SD3 LoRA)"
    from simpletuner_amd.foundation import ModelTypes
    with pytest.raises(ValueError) as e:
        M.refuse_unbuilt(base, SimpleNamespace(MODEL_TYPE=ModelTypes.UNET, NAME="sdxl"))
    assert str(e.value) == "Self-Transcendence supports diffusion transformer model families, not UNet models."
    with pytest.raises(ValueError) as e:
        M.refuse_unbuilt({**base, "lora_type": "lycoris"}, probe)
    assert str(e.value) == "Self-Transcendence supports full-model and standard PEFT LoRA training; LyCORIS is not supported."
    # through the Trainer, at construction
    with pytest.raises(NotImplementedError) as e:
        build(use_dora=True)
    assert str(e.value) == cases[0][1]
    with pytest.raises(NotImplementedError) as e:
        build(hip_graph=True)
    assert "hip_graph" in str(e.value)
    # the component's own refusals
    from simpletuner_amd.sd3 import transformer as T
    m = T.SD3Transformer2DModel(device="cpu", **SH._arch(3))
    with pytest.raises(ValueError) as e:
        m.set_self_transcendence("vae", 3)
    assert str(e.value) == "Self-Transcendence student_block must be within [0, 2], got 3."
    with pytest.raises(ValueError) as e:
        m.set_self_transcendence("self", 1, 7)
    assert str(e.value) == "Self-Transcendence teacher_block must be within [0, 2], got 7."
    m.set_self_transcendence("vae", 1, None, HP)
    with pytest.raises(NotImplementedError, match="distillation_method=self_transcendence together with Self-Flow"):
        m.set_self_flow(1, 2)
    with pytest.raises(ValueError) as e:
        m.add_lokr_adapter()
    assert str(e.value) == "Self-Transcendence supports full-model and standard PEFT LoRA training; LyCORIS is not supported."
    m.add_lora_adapter(rank=8)
    d = SH._inputs(2, 16, 24, 33)
    with pytest.raises(NotImplementedError, match="distillation_method=self_transcendence with tokenwise timesteps is not built on the st355 path"):
        m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"][:, None].expand(2, 96).contiguous(),
          self_transcendence_target=d["target"], self_transcendence_sigmas=SIGMAS)
    m2 = T.SD3Transformer2DModel(device="cpu", **SH._arch(3))
    m2.add_lora_adapter(rank=8)
    with pytest.raises(RuntimeError, match="before add_lora_adapter"):
        m2.set_self_transcendence("vae", 1)
    # flow_dpo's own refusal text is untouched
    from simpletuner_amd.flow_dpo import create_distiller
    with pytest.raises(NotImplementedError) as e:
        create_distiller(SimpleNamespace(config={"distillation_method": "dmd"}))
    assert str(e.value) == "distillation_method=dmd: not built on the st355 path (built: flow_dpo)"


def test_lora_dropout_is_overridden_to_zero(monkeypatch):
    plugin = _plugin(monkeypatch, lora_rank=8, lora_dropout=0.1)
    plugin.add_lora_adapter()
    assert plugin.config.lora_dropout == 0.0 and plugin.get_trained_component().lora_dropout is None


def test_nothing_is_imported_allocated_or_launched_with_the_method_absent(monkeypatch):
    code = ("import sys, torch\nsys.path.insert(0, '.')\nfrom tests import test_self_transcendence_cpu as T\nimport pytest\nmp = pytest.MonkeyPatch()\n"
            "plugin, trainer, batch, _ = T._trainer(mp, 'vae', method=None)\ntrainer.train_step(dict(batch))\n"
            "comp = plugin.get_trained_component()\nassert comp._st is None and comp._st_cfg is None and trainer.distiller is None\n"
            "assert 'simpletuner_amd.self_transcendence' not in sys.modules\nassert not any(n.startswith('self_transcendence') for n, _ in comp.named_parameters())\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_launch_trace_with_the_flag_off_is_the_parents(tmp_path):
    """flag off, nothing moved: tools/launch_trace.py over the SD3 tokenwise host-sequencing tests and the LoRA NextLat / Self-Flow engine tests (the tap list and
    the adapter arena tail this feature extends) gives, byte for byte, the file it gave at the parent commit, whose digest was recorded there
    (tests/golden/self_transcendence_flag_off_launch_trace.sha256)"""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "launch_trace.py"), str(out), "-k", TB.TRACE_SELECTION], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = (ROOT / "tests" / "golden" / "self_transcendence_flag_off_launch_trace.sha256").read_text().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

"""DoRA (`use_dora`) on the CPU: the fp64 restatement against autograd (and the detached norm pinned), the SD3 engine on the kernel-contract emulator against
autograd through the oracle with the DoRA linear, the arena lay-out, the plugin / trainer surface and the adapter files.  peft is not installed: the rule is
pinned to the published formula as tests/dora_ref.py restates it, not to executed reference code."""
import hashlib
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from oracle import sd3 as OS
from tests import dora_ref as DR
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# (a) the rule
# ------------------------------------------------------------------------------------------------
def _problem(M=37, N=24, K=40, r=4, seed=0, bias=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    return dict(x=rn(M, K), W=rn(N, K) / K ** 0.5, b=rn(N) if bias else None, A=rn(r, K) / K ** 0.5, Bm=0.3 * rn(N, r), m=1.0 + 0.2 * rn(N).abs(), s=0.5, dy=rn(M, N))


@pytest.mark.parametrize("bias", [True, False])
def test_restatement_equals_autograd_with_the_detached_norm(bias):
    p = _problem(bias=bias)
    leaves = {k: p[k].clone().requires_grad_(True) for k in ("x", "A", "Bm", "m")}
    y = DR.dora_autograd(leaves["x"], p["W"], p["b"], leaves["A"], leaves["Bm"], leaves["m"], p["s"])
    y.backward(p["dy"])
    y64, dx, dA, dB, dm, g, norm = DR.dora64(p["x"], p["W"], p["b"], p["A"], p["Bm"], p["m"], p["s"], p["dy"])
    for name, got, want in (("y", y64, y.detach()), ("dx", dx, leaves["x"].grad), ("dA", dA, leaves["A"].grad), ("dB", dB, leaves["Bm"].grad), ("dm", dm, leaves["m"].grad)):
        err = (got - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-13, (name, err)          # fp64 rounding of sums of at most 40 terms
    # peft's form: base(x) + (g - 1) . (x W^T) + g . s B A x, the bias outside the scale
    xw = p["x"] @ p["W"].t()
    peft = xw + (0.0 if p["b"] is None else p["b"]) + (g - 1.0) * xw + g * p["s"] * ((p["x"] @ p["A"].t()) @ p["Bm"].t())
    assert (peft - y64).abs().max().item() < 1e-12


def test_the_gradient_without_the_detach_differs():
    """paper section 4.3 / peft: the norm is a constant of the backward.  Autograd THROUGH the norm gives other dA / dB — the restatement follows the detached rule"""
    p = _problem()
    grads = {}
    for detach in (True, False):
        A, Bm = p["A"].clone().requires_grad_(True), p["Bm"].clone().requires_grad_(True)
        DR.dora_autograd(p["x"], p["W"], p["b"], A, Bm, p["m"], p["s"], detach=detach).backward(p["dy"])
        grads[detach] = (A.grad, Bm.grad)
    _, _, dA, dB, *_ = DR.dora64(p["x"], p["W"], p["b"], p["A"], p["Bm"], p["m"], p["s"], p["dy"])
    assert PU.rel_l2(dA, grads[True][0]) < 1e-12 and PU.rel_l2(dB, grads[True][1]) < 1e-12
    assert PU.rel_l2(dA, grads[False][0]) > 1e-2 and PU.rel_l2(dB, grads[False][1]) > 1e-2


# ------------------------------------------------------------------------------------------------
# (b) the SD3 engine on the emulator
# ------------------------------------------------------------------------------------------------
def _model(monkeypatch, layers, sd35=False, dora=True, rank=16, targets="default", pre=None, **kw):
    DR.install(monkeypatch)
    model = SH._model(monkeypatch, layers, sd35)
    DR.install(monkeypatch)                       # (SH._model installs the plain emulator again)
    if pre is not None:
        pre(model)
    model.add_lora_adapter(rank=rank, alpha=float(rank), init_b_std=0.02, targets=targets, dora=dora, **kw)
    model.train()
    return model


def _perturb(model, seed=3):
    """move the magnitudes off their initial value, so that g != 1 and dm is a gradient of something"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(DR.KEY):
                p.mul_((1.0 + 0.2 * (torch.rand(p.shape, generator=g) - 0.5)).to(p.device))


def _oracle(monkeypatch, model, d, dora=True):
    mags = {k: v.requires_grad_(True) for k, v in DR.magnitudes(model).items()}
    if dora:
        monkeypatch.setattr(OS, "linear", DR.dora_linear(mags))
    P, lora, scale = PU.oracle_state(model)
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    out = OS.sd3_forward(P, SH._ocfg(model), d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale)
    loss = ((out - d["target"].float()) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), lp, mags


def _ref_grad(name, lp, mags, div=1.0):
    key, which = name.split(".lora_")
    if which.startswith("magnitude"):
        return mags[key].grad / div
    return lp[key][0 if which.startswith("A") else 1].grad / div


def _worst(model, lp, mags, div=1.0):
    worst = {"A": 0.0, "B": 0.0, "m": 0.0}
    for name, p in model.named_parameters():
        if ".lora_" in name:
            which = name.split(".lora_")[1]
            k = "m" if which.startswith("magnitude") else which[0]
            worst[k] = max(worst[k], PU.rel_l2(p.grad, _ref_grad(name, lp, mags, div)))
    return worst


@pytest.mark.parametrize("targets", ["default", "all"])
@pytest.mark.parametrize("ckpt", ["plain", "per-block"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_engine_with_dora_matches_autograd_through_the_dora_oracle(monkeypatch, sd35, ckpt, targets):
    model = _model(monkeypatch, 3, sd35, targets=targets)
    _perturb(model)
    if ckpt != "plain":
        model.gradient_checkpointing = True
    d = SH._inputs(2, 16, 24, 33)
    out, loss = SH._hip_side(model, d)
    o_out, o_loss, lp, mags = _oracle(monkeypatch, model, d)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, lp, mags)
    assert max(worst.values()) < 5e-2, worst
    assert any(n.endswith(DR.KEY) and p.grad.abs().max() > 0 for n, p in model.named_parameters())
    # ... and a reference that forgets the row scale is far outside the same tolerances
    monkeypatch.undo()
    DR.install(monkeypatch)
    n_out, _, nlp, nm = _oracle(monkeypatch, model, d, dora=False)
    assert PU.rel_l2(out, n_out) > 2e-2
    print(f"[emu] sd3{'.5' if sd35 else ''} DoRA {ckpt} {targets}: worst gradient rel-L2 {worst}")


@pytest.mark.parametrize("ckpt", ["plain", "per-block"])          # (under routing every plan is the per-block one, as in the reference)
def test_sd3_engine_with_dora_under_tread(monkeypatch, ckpt):
    from simpletuner_amd.training.tread import ReplayRouter
    d = SH._inputs(2, 16, 16, 24)
    B, Si = 2, 64
    g = torch.Generator().manual_seed(11)
    perm = torch.stack([torch.randperm(Si, generator=g) for _ in range(B)])
    Kk = Si - int(round(Si * 0.5))
    rec = {"mask": torch.ones(B, Si, dtype=torch.bool).scatter_(1, perm[:, :Kk], False), "ids_keep": perm[:, :Kk], "ids_mask": perm[:, Kk:], "ids_shuffle": perm,
           "ids_restore": torch.argsort(perm, dim=1)}
    routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]
    model = _model(monkeypatch, 4, True, rank=8)
    _perturb(model)
    model.set_router(ReplayRouter([rec]), routes)
    if ckpt != "plain":
        model.gradient_checkpointing = True
    out, loss = SH._hip_side(model, d)
    mags = {k: v.requires_grad_(True) for k, v in DR.magnitudes(model).items()}
    monkeypatch.setattr(OS, "linear", DR.dora_linear(mags))
    P, lora, scale = PU.oracle_state(model)
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    o_out = OS.sd3_forward(P, SH._ocfg(model), d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale,
                           tread={"routes": routes, "mask_infos": [rec]})
    o_loss = ((o_out - d["target"].float()) ** 2).mean()
    o_loss.backward()
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, lp, mags)
    assert max(worst.values()) < 5e-2, worst


def test_gradient_accumulation_adds_the_second_micro_step(monkeypatch):
    model = _model(monkeypatch, 3, True)
    _perturb(model)
    d1, d2 = SH._inputs(2, 16, 24, 33, seed=5), SH._inputs(2, 16, 24, 33, seed=6)
    SH._hip_side(model, d1)
    model.accumulate_lora_grads = True
    for p in model.parameters():
        p.grad = None                            # the engine's flat gradient arena keeps the first micro-step's values
    SH._hip_side(model, d2)
    got = {n: p.grad.clone() for n, p in model.named_parameters() if ".lora_" in n}
    refs = []
    for d in (d1, d2):
        _, _, lp, mags = _oracle(monkeypatch, model, d)
        refs.append({n: _ref_grad(n, lp, mags) for n in got})
    for n in got:
        assert PU.rel_l2(got[n], refs[0][n] + refs[1][n]) < 5e-2, n


def test_init_gives_g_of_exactly_one_and_the_plain_lora_forward(monkeypatch):
    d = SH._inputs(2, 16, 24, 33)
    run = lambda m: m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()
    model = _model(monkeypatch, 3, True)
    for g in model.lora_groups:
        assert torch.equal(g.dora.g, torch.ones_like(g.dora.g)) and torch.equal(g.dora.Wf, g.dora.lin.w) and torch.equal(g.dora.Bf, g.B_blk)
    a = run(model)
    for g in model.lora_groups:          # (the fold of the forward reproduces the norm: still exactly 1)
        assert torch.equal(g.dora.g, torch.ones_like(g.dora.g))
    from simpletuner_amd.sd3 import transformer as T
    monkeypatch.setattr(T, "_BLOCK_ABI", False)          # the plain LoRA, host-sequenced like DoRA
    plain = _model(monkeypatch, 3, True, dora=False)
    monkeypatch.setattr(T, "_BLOCK_ABI", False)
    assert all(g.dora is None for g in plain.lora_groups)
    assert torch.equal(a, run(plain))
    model.eval()                                         # DoRA is part of the weight: eval() and no-grad forwards apply it too
    _perturb(model)
    with torch.no_grad():
        assert not torch.equal(run(model), run(plain))


# ------------------------------------------------------------------------------------------------
# (c) the arena
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["none", "internal_guidance", "nextlat", "layersync"])
def test_parameters_and_gradients_are_one_run_with_the_magnitudes_behind_the_adapters(monkeypatch, extra):
    from simpletuner_amd.training.optimizer import flat_view
    pre = {"none": None, "internal_guidance": lambda m: m.set_internal_guidance(1), "nextlat": lambda m: m.set_nextlat(None),
           "layersync": lambda m: m.set_layersync(0, 1)}[extra]
    model = _model(monkeypatch, 3, True, pre=pre)
    params = model.trainable_parameters()
    names = {id(p): n for n, p in model.named_parameters()}
    order = [names[id(p)] for p in params]
    kinds = ["m" if n.endswith(DR.KEY) else ("ab" if ".lora_" in n else "head") for n in order]
    assert kinds == sorted(kinds, key=("ab", "m", "head").index), "A / B first, then the magnitudes, then a head"
    n_targets = sum(len(g.targets) for g in model.lora_groups)
    assert kinds.count("m") == n_targets and kinds.count("ab") == 2 * n_targets
    fv = flat_view(params)
    assert fv is not None and fv.data_ptr() == model.lora_flat.data_ptr() and fv.numel() == sum(p.numel() for p in params)
    off = 0
    for p in params:
        assert p.data_ptr() == model.lora_flat.data_ptr() + 4 * off
        off += p.numel()
    for g in model.lora_groups:
        assert g.dora.m.data_ptr() == model.lora_flat.data_ptr() + 4 * g.dora.flat_lo and g.dora.gm.data_ptr() == model.lora_grad_flat.data_ptr() + 4 * g.dora.flat_lo
        assert all(p.dtype == F32 and p.dim() == 1 for n, p in model.named_parameters() if n.endswith(DR.KEY))
    d = SH._inputs(2, 16, 24, 33)
    out = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    loss = ((out[0].float() - d["target"].float()) ** 2).mean()
    for extra_out in out[1:]:
        loss = loss + extra_out.float().mean()
    loss.backward()
    gv = flat_view([p.grad for p in params])
    assert gv is not None and gv.numel() == fv.numel()


def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, **cfg_kw):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    DR.install(monkeypatch)
    cfg = default_config(model_family="sd3", train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=0.02, **cfg_kw)
    plugin = SD3(cfg, _acc())
    plugin.load_model(**SH._arch(2))
    return plugin


def _trainer(monkeypatch, dora=True, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, learning_rate=1e-3, **cfg_kw)
    plugin.config.use_dora = dora
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


@pytest.mark.parametrize("opt", ["st355-adamw", "adamw_bf16", "optimi-lion", "torch-adafactor"])
def test_one_train_step_moves_the_magnitudes(monkeypatch, opt):
    plugin, trainer, batch = _trainer(monkeypatch, optimizer=opt)
    comp = plugin.get_trained_component()
    assert comp.lora_dora and all(g.dora is not None for g in comp.lora_groups)
    before = {n: p.detach().clone() for n, p in comp.named_parameters() if n.endswith(DR.KEY)}
    assert before
    trainer.train_step(dict(batch))
    trainer.train_step(dict(batch))          # (B = 0.02 noise at init: the first step's dm is already non-zero, the second sees g != 1)
    moved = [n for n, p in comp.named_parameters() if n.endswith(DR.KEY) and not torch.equal(p.detach(), before[n])]
    assert len(moved) == len(before)


# ------------------------------------------------------------------------------------------------
# (d) refusals, by name
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_path", ["simpletuner_amd.flux.model.Flux", "simpletuner_amd.pixart.model.PixartSigma", "simpletuner_amd.sdxl.model.SDXL",
                                      "simpletuner_amd.sd1x.model.StableDiffusion1"])
def test_families_without_the_fold_refuse_the_flag_by_name(cls_path):
    import importlib
    mod, cls = cls_path.rsplit(".", 1)
    Plug = getattr(importlib.import_module(mod), cls)
    plug = Plug.__new__(Plug)
    plug.config = SimpleNamespace(model_type="lora", lora_type="standard", use_dora=True)
    with pytest.raises(NotImplementedError) as ei:
        plug.use_dora_value()
    assert str(ei.value) == f"use_dora: DoRA is not built for {Plug.NAME} on the st355 path (built: SD3); set --use_dora=false"
    for cfg in (SimpleNamespace(model_type="lora", lora_type="standard"), SimpleNamespace(model_type="lora", lora_type="standard", use_dora=False),
                SimpleNamespace(model_type="full", use_dora=True), SimpleNamespace(model_type="lora", lora_type="lycoris", use_dora=True)):
        plug.config = cfg
        assert plug.use_dora_value() is False          # absent = off; a full fine-tune and lycoris ignore the flag


@pytest.mark.parametrize("kw,pat", [(dict(lora_dropout=0.1), r"use_dora with lora_dropout=0\.1"), (dict(optimizer="muon"), r"use_dora with optimizer 'muon'"),
                                    (dict(optimizer="soap"), r"use_dora with optimizer 'soap'"), (dict(lora_format="comfyui"), r"use_dora with lora_format=comfyui")])
def test_sd3_refuses_the_combinations_that_are_not_built(monkeypatch, kw, pat):
    plugin = _plugin(monkeypatch, **kw)
    plugin.config.use_dora = True
    with pytest.raises(NotImplementedError, match=pat):
        plugin.add_lora_adapter()


def test_the_component_refuses_dora_with_dropout_and_the_export_refuses_comfyui(monkeypatch, tmp_path):
    with pytest.raises(NotImplementedError, match="use_dora with lora_dropout=0.25"):
        _model(monkeypatch, 2, dropout=0.25)
    plugin, trainer, batch = _trainer(monkeypatch)
    plugin.config.lora_format = "comfyui"
    with pytest.raises(NotImplementedError, match="use_dora: the ComfyUI export of a DoRA adapter"):
        plugin.save_lora_weights(str(tmp_path))


# ------------------------------------------------------------------------------------------------
# (e) files
# ------------------------------------------------------------------------------------------------
def test_adapter_file_round_trip_both_spellings_and_the_mismatch_errors(monkeypatch, tmp_path):
    from safetensors.torch import load_file, save_file
    plugin, trainer, batch = _trainer(monkeypatch)
    trainer.train_step(dict(batch))
    comp = plugin.get_trained_component()
    path = plugin.save_lora_weights(str(tmp_path / "a"))
    flat = load_file(path)
    mk = [k for k in flat if "lora_magnitude_vector" in k]
    assert len(mk) == sum(len(g.targets) for g in comp.lora_groups)
    assert all(k.startswith("transformer.") and k.endswith(".lora_magnitude_vector.weight") and flat[k].dtype == F32 and flat[k].dim() == 1 for k in mk)
    want = comp.lora_flat.clone()
    plugin2, _, _ = _trainer(monkeypatch)
    assert not torch.equal(plugin2.get_trained_component().lora_flat, want)
    plugin2.load_lora_weights(input_dir=str(tmp_path / "a"))
    assert torch.equal(plugin2.get_trained_component().lora_flat, want)
    # the key without `.weight`
    os.makedirs(tmp_path / "b")
    save_file({(k[:-len(".weight")] if k in mk else k): v for k, v in flat.items()}, str(tmp_path / "b" / plugin.LORA_WEIGHT_NAME))
    plugin3, _, _ = _trainer(monkeypatch)
    plugin3.load_lora_weights(input_dir=str(tmp_path / "b"))
    assert torch.equal(plugin3.get_trained_component().lora_flat, want)
    # a DoRA file into a plain adapter, and the reverse
    plain, ptrainer, _ = _trainer(monkeypatch, dora=False)
    with pytest.raises(ValueError, match=r"carries DoRA magnitude vectors \(lora_magnitude_vector\) but the adapter was built without them: set --use_dora=true"):
        plain.load_lora_weights(input_dir=str(tmp_path / "a"))
    plain.save_lora_weights(str(tmp_path / "c"))
    with pytest.raises(ValueError, match="use_dora is set but the LoRA checkpoint carries no DoRA magnitude vectors"):
        plugin3.load_lora_weights(input_dir=str(tmp_path / "c"))


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


# ------------------------------------------------------------------------------------------------
# (f) flag off
# ------------------------------------------------------------------------------------------------
TRACE_K = "test_sd3_host_sequencing_cpu and (lora_path or tread_routing)"


def test_the_launch_trace_with_the_flag_off_is_the_one_recorded_before_dora(tmp_path):
    """tools/launch_trace.py over the SD3 host-sequencing tests (the LoRA path, and TREAD / the checkpoint plans): every emulated launch with its operands' dtypes,
    shapes and strides, in order.  The digest under tests/golden/ was recorded on the commit before DoRA: with the flag off nothing is launched differently."""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_trace.py"), str(out), "-k", TRACE_K], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = open(os.path.join(ROOT, "tests", "golden", "dora_flag_off_launch_trace.sha256")).read().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

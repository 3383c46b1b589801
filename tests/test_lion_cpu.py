"""Lion ("optimi-lion") without a GPU: the registry entry against the reference's (tests/golden/lion_vectors.pt, written by tools/gen_lion_golden.py), the checker of
tests/lion_bounds.py on a correct CPU stand-in and on three planted errors, the trainer surface on the kernel-contract emulator, and state handling.  St355Lion's
kernel call is replaced by the stand-in tests/lion_bounds.lion_step_cpu."""
from types import SimpleNamespace

import pytest
import torch

from tests import lion_bounds as LB

GOLD = LB.golden()
H = GOLD["hyper"]
F32, BF16 = torch.float32, torch.bfloat16


# ---- (a) registry ------------------------------------------------------------------------------------------------------------------------------------------
def test_registry_entry_equals_the_reference_default_settings():
    from simpletuner_amd.training.optimizer import OPTIMIZER_CHOICE, St355Lion, optimizer_settings
    entry = OPTIMIZER_CHOICE["optimi-lion"]
    assert entry["class"] is St355Lion and entry["precision"] == "any"
    assert entry["default_settings"] == GOLD["default_settings"]
    assert "override_lr_scheduler" not in entry
    assert optimizer_settings("optimi-lion", SimpleNamespace()) == GOLD["default_settings"]
    merged = optimizer_settings("optimi-lion", SimpleNamespace(optimizer_config="weight_decay=0.01,kahan_sum=false"))
    assert merged == dict(GOLD["default_settings"], weight_decay=0.01, kahan_sum=False)


def test_integration_offers_the_entry_to_simpletuner():
    import inspect

    from simpletuner_amd import integration
    assert "OPTIMIZER_CHOICE.items()" in inspect.getsource(integration)          # the dict is iterated: the new entry needs no line of its own


def test_make_inputs_reproduces_the_recorded_sample():
    x = LB.make_inputs(2097155, F32, GOLD["seeds"]["fp32"], grad_scale=H["grad_scale"], beta1=H["beta1"])
    for k in ("g", "m", "p"):
        assert torch.equal(LB.bits(x[k][:2048]), LB.bits(GOLD["sample"][k])), k
    assert x["zeros"] == 1024 and x["cancel"] == 64
    assert not x["g"][:1024].any() and not x["m"][:1024].any()


# ---- (b) the checker accepts a correct implementation and rejects three planted errors -----------------------------------------------------------------
def _one(dtype, n, wd, kahan, plant=None, seed="fp32"):
    x = LB.make_inputs(n, dtype, GOLD["seeds"][seed], grad_scale=H["grad_scale"], beta1=H["beta1"])
    c = LB.lion_consts(H["lr"], H["beta1"], H["beta2"], wd, H["grad_scale"])
    p, m = x["p"].clone(), x["m"].clone()
    comp = x["comp"].clone() if kahan else None
    LB.lion_step_cpu(p, x["g"], m, H["lr"], H["beta1"], H["beta2"], wd, H["grad_scale"], comp=comp, plant=plant)
    reports, info = LB.check_step(f"stand-in {dtype} n={n} wd={wd} kahan={kahan} plant={plant}", c, x["p"], x["g"], x["m"], p, m, x["comp"] if kahan else None, comp,
                                  verbose=plant is None)
    return reports, info, x, p


@pytest.mark.parametrize("dtype,n,kahan", [(F32, 131075, False), (BF16, 131080, False), (BF16, 131080, True), (F32, 1027, False), (BF16, 1032, True)])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_stand_in_is_within_the_bounds_of_its_own_restatement(dtype, n, kahan, wd):
    reports, info, x, p = _one(dtype, n, wd, kahan)
    LB.assert_reports(reports)
    if dtype == F32 and n > 64000:
        assert info["undecided"] > 0, "the 64 cancelling elements must make the undecided branch run"
    z = x["zeros"]
    if wd == 0.0:                                                            # g = m = 0: the parameter's bits stay
        assert torch.equal(LB.bits(p[:z]), LB.bits(x["p"][:z]))


@pytest.mark.parametrize("plant", ["sign_of_m", "betas_swapped", "decay_after"])
@pytest.mark.parametrize("dtype,n,kahan", [(F32, 131075, False), (BF16, 131080, True)])
def test_checker_rejects_planted_errors(dtype, n, kahan, plant):
    reports, _, _, _ = _one(dtype, n, 1e-2, kahan, plant=plant)
    assert not LB.reports_ok(reports), f"{plant} passed the bounds"


def test_checker_refuses_inputs_that_do_not_decide_the_sign():
    n = 4096
    z = torch.zeros(n)
    m = torch.full((n,), 0.5)
    g = (-(m.double() * LB.f32(0.9) / (1.0 - LB.f32(0.9)))).float()         # every element cancels
    with pytest.raises(AssertionError, match="undecided"):
        LB.check_step("all cancel", LB.lion_consts(1e-3, 0.9, 0.99, 0.0, 1.0), z, g, m, z, m)


# ---- (c) the trainer on the kernel-contract emulator ----------------------------------------------------------------------------------------------------
def _recording(monkeypatch):
    """install the stand-in, recording (inputs before, kwargs, outputs after) of every call"""
    from simpletuner_amd import ops
    calls = []

    def rec(p, g, m, lr, beta1=0.9, beta2=0.99, weight_decay=0.0, grad_scale=1.0, comp=None, ema=None, ema_decay=0.0, p_bf16=None):
        before = dict(p=p.clone(), g=g.clone(), m=m.clone(), comp=None if comp is None else comp.clone(), ema=None if ema is None else ema.clone())
        LB.lion_step_cpu(p, g, m, lr, beta1, beta2, weight_decay, grad_scale, comp=comp, ema=ema, ema_decay=ema_decay, p_bf16=p_bf16)
        calls.append(dict(before=before, hp=dict(lr=lr, beta1=beta1, beta2=beta2, wd=weight_decay, gs=grad_scale, ema_decay=ema_decay),
                          after=dict(p=p.clone(), m=m.clone(), comp=None if comp is None else comp.clone(), ema=None if ema is None else ema.clone())))

    monkeypatch.setattr(ops, "lion_step", rec)
    return calls


def _check_calls(calls, what):
    for k, c in enumerate(calls):
        b, a, hp = c["before"], c["after"], c["hp"]
        consts = LB.lion_consts(hp["lr"], hp["beta1"], hp["beta2"], hp["wd"], hp["gs"], hp["ema_decay"])
        reports, _ = LB.check_step(f"{what} step {k + 1}", consts, b["p"], b["g"], b["m"], a["p"], a["m"], b["comp"], a["comp"])
        LB.assert_reports(reports)
        if a["ema"] is not None:
            ema = LB.ema_bf16 if a["ema"].dtype == BF16 else LB.ema_f32
            chk = LB.check_bf16 if a["ema"].dtype == BF16 else LB.check_f32
            LB.assert_reports([chk(f"{what} step {k + 1} ema", a["ema"], *ema(b["ema"], a["p"], consts["omd"]), flat=True)])


def test_trainer_runs_flux_lora_with_optimi_lion(monkeypatch):
    """three train_steps of the smallest host-loop Flux LoRA configuration with optimizer="optimi-lion": the registry's settings reach the optimizer, the step is ONE
    call over the fp32 adapter arena, and every step's (p, m) is within the bounds of the restatement fed the same stored gradients.  lora_B starts at zero, so the
    first gradient of every lora_A is exactly zero: sign(0) = 0 must leave it alone."""
    from simpletuner_amd.training.optimizer import St355Lion
    from tests.test_trainer_host_loop_cpu import _batch, _build
    plugin, trainer, cpu, devt = _build(monkeypatch, 1, 1, 2, 8, 8, 24, lora_rank=8, learning_rate=1e-3, optimizer="optimi-lion")
    calls = _recording(monkeypatch)
    assert isinstance(trainer.optimizer, St355Lion) and trainer.lr_scheduler is None
    group = trainer.optimizer.param_groups[0]
    assert group["lr"] == 1e-3 and tuple(group["betas"]) == (0.9, 0.99) and group["weight_decay"] == 0.0 and group["kahan_sum"] is True
    model = plugin.get_trained_component()
    start = model.lora_flat.clone()
    losses = [float(trainer.train_step(_batch(devt))) for _ in range(3)]
    assert len(calls) == 3 and all(c["before"]["p"].numel() == model.lora_flat.numel() and c["before"]["p"].dtype == F32 for c in calls)
    assert all(c["before"]["comp"] is None for c in calls), "fp32 parameters never get a compensation buffer"
    _check_calls(calls, "flux lora")
    first = calls[0]
    idle = (first["before"]["g"] == 0)
    assert bool(idle.any()) and torch.equal(LB.bits(first["after"]["p"][idle]), LB.bits(start[idle]))
    assert not torch.equal(model.lora_flat, start) and all(l == l for l in losses)
    assert trainer.state["global_step"] == 3
    for p in trainer.params:
        assert set(trainer.optimizer.state[p]) == {"exp_avg"} and trainer.optimizer.state[p]["exp_avg"].dtype == F32


def test_trainer_runs_full_rank_with_fused_ema_on_the_bf16_arena(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Lion
    from tests.test_trainer_host_loop_cpu import _batch, _build
    plugin, trainer, cpu, devt = _build(monkeypatch, 1, 1, 2, 8, 8, 24, model_type="full", learning_rate=1e-4, use_ema=True, ema_decay=0.9, optimizer="optimi-lion",
                                        optimizer_config="weight_decay=0.01")
    calls = _recording(monkeypatch)
    assert isinstance(trainer.optimizer, St355Lion)
    for _ in range(3):
        trainer.train_step(_batch(devt))
    assert len(calls) == 3 and trainer.optimizer.ema_applied
    assert all(c["before"]["p"].dtype == BF16 and c["before"]["comp"] is not None and c["before"]["ema"] is not None and c["hp"]["wd"] == 0.01 for c in calls)
    _check_calls(calls, "flux full rank")
    assert trainer.ema_model.optimization_step == 3
    p0 = trainer.params[0]
    assert set(trainer.optimizer.state[p0]) == {"exp_avg", "kahan_comp"} and trainer.optimizer.state[p0]["exp_avg"].dtype == BF16


def test_trainer_still_refuses_unbuilt_optimizers():
    from simpletuner_amd.training.trainer import Trainer, default_config
    comp = SimpleNamespace(trainable_parameters=lambda: [torch.nn.Parameter(torch.zeros(8))], full=False)
    plug = SimpleNamespace(get_trained_component=lambda: comp, accelerator=SimpleNamespace(num_processes=1))
    with pytest.raises(NotImplementedError, match="optimi-stableadamw"):
        Trainer(default_config(optimizer="optimi-stableadamw"), plug, SimpleNamespace(num_processes=1))


# ---- (d) state handling -----------------------------------------------------------------------------------------------------------------------------------
def _arena(dtype, seed, shapes=((16, 64), (64, 16), (40,))):
    g = torch.Generator().manual_seed(seed)
    n = sum(int(torch.tensor(s).prod()) for s in shapes)
    flat = (0.05 * torch.randn(n, generator=g)).to(dtype)
    grad = torch.zeros(n, dtype=dtype)
    ps, off = [], 0
    for s in shapes:
        k = int(torch.tensor(s).prod())
        p = torch.nn.Parameter(flat[off:off + k].view(s))
        p.grad = grad[off:off + k].view(s)
        ps.append(p)
        off += k
    return flat, grad, ps


def _set_grads(grad, step):
    g = torch.Generator().manual_seed(GOLD["seeds"]["optimizer"] + step)
    grad.copy_((1e-2 * torch.randn(grad.numel(), generator=g)).to(grad.dtype))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_resume_from_a_state_dict_is_bit_exact(monkeypatch, tmp_path, dtype):
    from simpletuner_amd.training.optimizer import St355Lion
    LB.install(monkeypatch)
    make = lambda ps, lr=1e-3: St355Lion(ps, lr=lr, weight_decay=0.01)
    a_flat, a_grad, a_ps = _arena(dtype, 1)
    a = make(a_ps)
    for s in range(1, 5):
        _set_grads(a_grad, s)
        a.step()
    b_flat, b_grad, b_ps = _arena(dtype, 1)
    b = make(b_ps)
    for s in range(1, 3):
        _set_grads(b_grad, s)
        b.step()
    sd = b.state_dict()
    keys = {"exp_avg", "kahan_comp"} if dtype == BF16 else {"exp_avg"}
    assert sorted(sd["state"]) == [0, 1, 2] and all(set(st) == keys for st in sd["state"].values())
    assert all(st["exp_avg"].dtype == dtype and st["exp_avg"].shape == p.shape for st, p in zip(sd["state"].values(), b_ps))
    torch.save({"state": {k: {n: v.detach().clone() for n, v in st.items()} for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]}, tmp_path / "optimizer.bin")
    c_flat, c_grad, c_ps = _arena(dtype, 99)                   # fresh objects, different init ...
    c_flat.copy_(b_flat)                                       # ... the model weights come from the checkpoint
    c = make(c_ps, lr=0.5)
    c.load_state_dict(torch.load(tmp_path / "optimizer.bin"))
    assert c.param_groups[0]["lr"] == 1e-3
    for s in range(3, 5):
        _set_grads(c_grad, s)
        c.step()
    assert torch.equal(LB.bits(c_flat), LB.bits(a_flat))
    assert torch.equal(LB.bits(c._flat[0]["m"]), LB.bits(a._flat[0]["m"]))
    if dtype == BF16:
        assert torch.equal(LB.bits(c._flat[0]["comp"]), LB.bits(a._flat[0]["comp"]))
    else:
        assert c._flat[0]["comp"] is None


def test_constructor_and_compensation_buffer_rules(monkeypatch):
    from simpletuner_amd import ops
    from simpletuner_amd.training.optimizer import St355Lion
    _, _, ps = _arena(F32, 2)
    with pytest.raises(NotImplementedError, match="decouple_lr"):
        St355Lion(ps, lr=1e-3, decouple_lr=True)
    with pytest.raises(ValueError, match="beta1"):
        St355Lion(ps, lr=1e-3, betas=(1.0, 0.99))
    calls = []
    monkeypatch.setattr(ops, "lion_step", lambda p, g, m, *a, **k: (calls.append((p.numel(), k.get("comp") is not None)), LB.lion_step_cpu(p, g, m, *a, **k))[1])
    # fp32: one call for the whole group, no compensation buffer whatever kahan_sum says; foreach and unknown registry keys are accepted
    flat, grad, ps = _arena(F32, 3)
    opt = St355Lion(ps, lr=1e-3, kahan_sum=True, foreach=True, max_lr=None)
    _set_grads(grad, 1)
    opt.step()
    assert calls == [(flat.numel(), False)] and all("kahan_comp" not in opt.state[p] for p in ps)
    # bf16: compensated when kahan_sum is True or None, not when False
    for kahan, want in ((True, True), (None, True), (False, False)):
        calls.clear()
        flat, grad, ps = _arena(BF16, 4)
        opt = St355Lion(ps, lr=1e-3, kahan_sum=kahan)
        _set_grads(grad, 1)
        opt.step()
        assert calls == [(flat.numel(), want)] and all(("kahan_comp" in opt.state[p]) == want for p in ps)
    # parameters that are not one contiguous run: one call per tensor, the same arithmetic
    calls.clear()
    flat, grad, ps = _arena(F32, 3)
    loose = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for q, p in zip(loose, ps):
        q.grad = p.grad.clone()
    ref = St355Lion(ps, lr=1e-3, weight_decay=0.01)
    opt = St355Lion(loose, lr=1e-3, weight_decay=0.01)
    for s in (1, 2):
        _set_grads(grad, s)
        for q, p in zip(loose, ps):
            q.grad.copy_(p.grad)
        ref.step()
        opt.step()
    assert [c[0] for c in calls] == [flat.numel()] + [p.numel() for p in ps] + [flat.numel()] + [p.numel() for p in ps]
    for q, p in zip(loose, ps):
        assert torch.equal(q, p) and torch.equal(opt.state[q]["exp_avg"], ref.state[p]["exp_avg"])

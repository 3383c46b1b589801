"""Adafactor without a GPU: the fp64 restatement (tests/adafactor_ref.py) and the fp32 stand-in against torch.optim.Adafactor EXECUTED on the CPU, the
stand-in inside the derived bounds (tests/adafactor_bounds.py), St355Adafactor's state layout, size and state-dict exchange with torch's class, the
registry / trainer surface with its refusals, and the trainer's host loop — St355Adafactor's kernel calls replaced by the CPU stand-in."""
import copy
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import adafactor_bounds as AB
from tests import adafactor_ref as AR

ROOT = Path(__file__).resolve().parent.parent
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
HP = dict(beta2_decay=-0.8, eps2=1e-3, d=1.0)
_CACHE = {}


def _torch_runs(dtype, wd, gs):
    """torch.optim.Adafactor(foreach=False) on the arena instance's values, in fp32 and in fp64, eps1 given as the instance dtype's epsilon; computed once"""
    key = (dtype, wd, gs)
    if key not in _CACHE:
        offs, n, p0, grads = AR.make_arena(dtype)
        eps1 = torch.finfo(dtype).eps
        runs = {}
        for dt in (F32, F64):
            ps = [torch.nn.Parameter(t.to(dt).clone()) for t in AR.tensors_of(p0, offs)]
            opt = torch.optim.Adafactor(ps, lr=AR.LR, eps=(eps1, HP["eps2"]), weight_decay=wd, foreach=False)
            traj = []
            for k in range(AR.STEPS):
                for p, g in zip(ps, AR.tensors_of(grads[k], offs)):
                    p.grad = g.to(dt) * gs
                opt.step()
                traj.append([p.detach().clone() for p in ps])
            runs[dt] = (traj, opt)
        _CACHE[key] = (offs, n, p0, grads, eps1, runs)
    return _CACHE[key]


def _dist(a, b):
    return max(float((x.to(F64) - y.to(F64)).abs().max()) for A, B in zip(a, b) for x, y in zip(A, B))


def _params(flat, gflat, offs, shapes=AR.ARENA_SHAPES):
    ps = []
    for p, g in zip(AR.tensors_of(flat, offs, shapes), AR.tensors_of(gflat, offs, shapes)):
        q = torch.nn.Parameter(p)
        q.grad = g
        ps.append(q)
    return ps


def _packed(dtype, seed=0):
    """the arena's tensors back to back (what St355Adafactor steps: one contiguous run), values of make_arena"""
    offs, n, p0, grads = AR.make_arena(dtype, seed)
    vals, gvals = AR.tensors_of(p0, offs), [AR.tensors_of(g, offs) for g in grads]
    flat = torch.cat([v.reshape(-1) for v in vals]).clone()
    gsteps = [torch.cat([v.reshape(-1) for v in gv]) for gv in gvals]
    poffs, o = [], 0
    for v in vals:
        poffs.append(o)
        o += v.numel()
    return flat, gsteps, poffs


@pytest.mark.parametrize("wd,gs", AR.CASES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_restatement_and_stand_in_follow_the_executed_torch_class(dtype, wd, gs):
    """tolerance: torch-fp32's own distance from torch-fp64 over the three steps, computed here, times 4 (the margin of SOAP's trajectory tests for an
    independent fp32 evaluation of a well-posed rule).  The restatement itself must reproduce torch-fp64 to fp64 rounding"""
    offs, n, p0, grads, eps1, runs = _torch_runs(dtype, wd, gs)
    t32, t64 = runs[F32][0], runs[F64][0]
    gl = [AR.tensors_of(g, offs) for g in grads]
    mine, _, inter = AR.run_fp64(AR.tensors_of(p0, offs), gl, AR.LR, eps=(eps1, HP["eps2"]), weight_decay=wd, grad_scale=gs)
    d_rule, d_torch = _dist(mine, t64), _dist(t32, t64)
    assert d_rule <= 1e-12 * max(1.0, float(p0.abs().max())), d_rule
    # the arena is what the issue describes
    denoms = [float(x["denom"]) for xs in inter for x in xs]
    assert any(d > 1.0 for d in denoms) and any(d == 1.0 for d in denoms)
    assert float(inter[0][AR.ZERO_TENSOR]["rms"]) == 0.0 and float(inter[0][AR.ZERO_TENSOR]["alpha"]) == HP["eps2"] * AR.LR
    v = inter[0][AR.PART_CLAMPED]["v"]
    assert bool((v < eps1 * eps1).any()) and bool((v > eps1 * eps1).any())
    assert bool((inter[0][AR.ROW_MEAN_CLAMPED]["rm"] == eps1).all()) and not any(bool((x["rm"] == eps1).any()) for i, x in enumerate(inter[0])
                                                                                     if i in (0, 1, AR.PART_CLAMPED, 3))
    # the fp32 stand-in on the same values as an fp32 arena (eps1 explicit: the instance dtype's)
    plan = AR.AdafactorPlanCPU(offs, AR.ARENA_SHAPES, None)
    pf = p0.to(F32).clone()
    rv, cv, var = torch.zeros(plan.rv_len), torch.zeros(plan.cv_len), torch.zeros(plan.var_len)
    standin = []
    for k in range(AR.STEPS):
        AR.adafactor_step_cpu(plan, pf, grads[k].to(F32), rv, cv, var, k + 1, AR.LR, eps1=eps1, weight_decay=wd, grad_scale=gs, **HP)
        standin.append([t.clone() for t in AR.tensors_of(pf, offs)])
    d_standin = _dist(standin, t32)
    print(f"[adafactor] {dtype} wd {wd} gs {gs}: restatement vs torch-fp64 {d_rule:.2e}; torch-fp32 vs torch-fp64 {d_torch:.3e}; stand-in vs torch-fp32 {d_standin:.3e}")
    assert d_torch > 0.0 and d_standin <= 4.0 * d_torch


@pytest.mark.parametrize("wd,gs", AR.CASES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_stand_in_lies_inside_the_derived_bounds(dtype, wd, gs):
    offs, n, p0, grads = AR.make_arena(dtype)
    plan = AR.AdafactorPlanCPU(offs, AR.ARENA_SHAPES, None)
    pf = p0.clone()
    rv, cv, var = torch.zeros(plan.rv_len), torch.zeros(plan.cv_len), torch.zeros(plan.var_len)
    eps1 = torch.finfo(dtype).eps

    def states():
        out = []
        for i, (b, R, C) in enumerate(plan.factors):
            if R == 0:
                out.append({"variance": var[plan.var_offsets[i]:plan.var_offsets[i] + C].clone()})
            else:
                out.append({"row_var": rv[plan.rv_offsets[i]:plan.rv_offsets[i] + b * R].view(b, R, 1).clone(),
                            "col_var": cv[plan.cv_offsets[i]:plan.cv_offsets[i] + b * C].view(b, 1, C).clone()})
        return out

    worst = 0.0
    pads = AR.pad_mask(offs, n)
    for k in range(AR.STEPS):
        pb, sb = [t.clone() for t in AR.tensors_of(pf, offs)], states()
        AR.adafactor_step_cpu(plan, pf, grads[k], rv, cv, var, k + 1, AR.LR, weight_decay=wd, grad_scale=gs, **HP)       # eps1=None: the arena dtype's
        c = AB.consts(k + 1, AR.LR, HP["beta2_decay"], eps1, HP["eps2"], HP["d"], wd, gs)
        worst, _ = AB.check_step(f"step {k + 1}", AR.ARENA_SHAPES, pb, AR.tensors_of(grads[k], offs), sb, AR.tensors_of(pf, offs), states(), c, dtype, worst, any_order=True)
    assert not pf[pads].any() and pf.dtype == dtype
    print(f"[adafactor] {dtype} wd {wd} gs {gs}: stand-in worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_state_layout_size_and_exchange_with_torchs_class(monkeypatch, dtype):
    from simpletuner_amd.training.optimizer import St355Adafactor
    AR.install(monkeypatch)
    eps1 = torch.finfo(dtype).eps
    wd = 0.01
    flat, gsteps, poffs = _packed(dtype)
    gflat = torch.zeros_like(flat)
    ps = _params(flat, gflat, poffs)
    opt = St355Adafactor(ps, lr=AR.LR, weight_decay=wd, foreach=True)
    # torch's own class on the same values, fp32 (the stand-in's arithmetic; for the bf16 instance torch in bf16 rounds its state, which the st355 path does not)
    tps = [torch.nn.Parameter(p.detach().to(F32).clone()) for p in ps]
    topt = torch.optim.Adafactor(tps, lr=AR.LR, eps=(eps1, 1e-3), weight_decay=wd, foreach=False)

    def both(k):
        gflat.copy_(gsteps[k])
        opt.step()
        for tp, p in zip(tps, ps):
            tp.grad = p.grad.to(F32).clone()
        topt.step()

    both(0)
    both(1)
    st = opt._flat[0]
    assert opt.abi_calls == 2 and opt.fuses_ema is False and not opt._buffers
    # layout: keys, shapes, dtypes, view-ness
    for p, tp in zip(ps, tps):
        s, ts = opt.state[p], topt.state[tp]
        assert set(s) == set(ts), (set(s), set(ts))
        assert torch.is_tensor(s["step"]) and s["step"].dtype == ts["step"].dtype and s["step"].dim() == 0 and float(s["step"]) == float(ts["step"]) == 2.0
        for key in set(s) - {"step"}:
            assert s[key].shape == ts[key].shape and s[key].dtype == F32, key
            buf = st[key]
            assert buf.data_ptr() <= s[key].data_ptr() < buf.data_ptr() + 4 * max(buf.numel(), 1) and s[key]._base is not None
    # size: exactly 4 (sum batch (R + C)) + 4 (sum of the 1-D lengths), and no buffer of the arena's length
    fac = [AR.factor_shape(tuple(p.shape)) for p in ps]
    want = 4 * sum(b * (R + C) for b, R, C in fac if R) + 4 * sum(C for b, R, C in fac if not R)
    bufs = [st["row_var"], st["col_var"], st["variance"]]
    assert sum(b.numel() * b.element_size() for b in bufs) == want
    assert all(b.numel() < flat.numel() for b in bufs) and not any(torch.is_tensor(v) and v.numel() == flat.numel() for v in st.values())
    tol32 = None
    if dtype == F32:
        # the third step after an exchange of state dicts, both directions, within the trajectory tolerance (4 x torch-fp32's distance from torch-fp64)
        _, _, _, _, _, runs = _torch_runs(dtype, wd, 1.0)
        tol32 = 4.0 * _dist(runs[F32][0], runs[F64][0])
    saved_torch, saved_mine = copy.deepcopy(topt.state_dict()), copy.deepcopy(opt.state_dict())
    p_torch2, p_mine2 = [tp.detach().clone() for tp in tps], flat.clone()
    both(2)
    # torch's state dict -> St355Adafactor (either dtype: the fp32 one, and one cast to bf16 as torch keeps it for bf16 parameters)
    for cast in (F32, BF16):
        sd = copy.deepcopy(saved_torch)
        for s in sd["state"].values():
            for key in s:
                if key != "step":
                    s[key] = s[key].to(cast)
        flat2 = torch.cat([t.reshape(-1) for t in p_torch2]).to(dtype)
        g2 = gsteps[2].clone()
        opt2 = St355Adafactor(_params(flat2, g2, poffs), lr=0.5)
        opt2.load_state_dict(sd)
        assert opt2.param_groups[0]["lr"] == AR.LR and opt2._flat[0]["step"] == 2
        assert all(opt2.state[p][k].dtype == F32 for p in opt2.param_groups[0]["params"] for k in opt2.state[p] if k != "step")
        for i, p in enumerate(opt2.param_groups[0]["params"]):         # the fp32 buffers hold exactly the saved values (after the cast, where there was one)
            for k, t in sd["state"][i].items():
                if k != "step":
                    assert torch.equal(opt2.state[p][k], t.to(F32)), (i, k)
        opt2.step()
        assert all(float(opt2.state[p]["step"]) == 3.0 for p in opt2.param_groups[0]["params"])
        if dtype == F32 and cast == F32:
            got = AR.tensors_of(flat2, poffs)
            assert max(float((a - b.detach()).abs().max()) for a, b in zip(got, tps)) <= tol32
    # St355Adafactor's state dict -> torch's class (fp32 instance: torch casts the state to the parameters' dtype, which is the state's own there)
    if dtype == F32:
        tps3 = [torch.nn.Parameter(t.clone()) for t in AR.tensors_of(p_mine2, poffs)]
        topt3 = torch.optim.Adafactor(tps3, lr=0.5, foreach=False)
        topt3.load_state_dict(copy.deepcopy(saved_mine))          # (torch adopts the tensors it is handed when dtype and device already fit)
        for tp, g in zip(tps3, AR.tensors_of(gsteps[2], poffs)):
            tp.grad = g.clone()
        topt3.step()
        assert all(float(topt3.state[tp]["step"]) == 3.0 for tp in tps3)          # every saved entry carries its own step tensor: torch counts one step, not one per parameter
        assert max(float((a.detach() - b).abs().max()) for a, b in zip(tps3, AR.tensors_of(flat, poffs))) <= tol32
    # its own state dict round-trips bit for bit
    flat4 = p_mine2.clone()
    opt4 = St355Adafactor(_params(flat4, gsteps[2].clone(), poffs), lr=0.5)
    opt4.load_state_dict(saved_mine)
    opt4.step()
    assert torch.equal(flat4, flat) and all(torch.equal(opt4._flat[0][k], st[k]) for k in ("row_var", "col_var", "variance"))


def test_constructor_refusals_and_the_missing_fallback(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Adafactor
    AR.install(monkeypatch)
    flat, gsteps, poffs = _packed(F32)
    ps = _params(flat, gsteps[0].clone(), poffs)
    with pytest.raises(NotImplementedError, match="maximize"):
        St355Adafactor(ps, lr=1e-2, maximize=True)
    with pytest.raises(NotImplementedError, match="tensor lr"):
        St355Adafactor(ps, lr=torch.tensor(1e-2))
    with pytest.raises(ValueError, match="beta2_decay"):
        St355Adafactor(ps, lr=1e-2, beta2_decay=0.5)
    with pytest.raises(ValueError, match="Clipping threshold"):
        St355Adafactor(ps, lr=1e-2, d=0.5)
    loose = [torch.nn.Parameter(torch.zeros(8, 40)), torch.nn.Parameter(torch.zeros(40, 8))]
    for q in loose:
        q.grad = torch.ones_like(q)
    with pytest.raises(NotImplementedError, match="one contiguous run"):
        St355Adafactor(loose, lr=1e-2).step()
    opt = St355Adafactor(ps, lr=1e-2)
    ps[3].grad = ps[3].grad.clone()                              # a gradient outside the arena: no per-tensor path
    with pytest.raises(RuntimeError, match="one flat arena"):
        opt.step()
    with pytest.raises(NotImplementedError, match="float16"):
        St355Adafactor([torch.nn.Parameter(torch.zeros(8, 8, dtype=torch.float16))], lr=1e-2).load_state_dict({"state": {}, "param_groups": [{"params": [0]}]})


class _Plugin:
    def __init__(self, comp):
        self.comp = comp
        self.accelerator = SimpleNamespace(num_processes=1)

    def get_trained_component(self):
        return self.comp


def test_trainer_wiring_registry_and_refusals(monkeypatch):
    """fails without the feature: NotImplementedError: optimizer 'torch-adafactor' is not built"""
    from simpletuner_amd.training.optimizer import OPTIMIZER_CHOICE, St355Adafactor, optimizer_settings
    from simpletuner_amd.training.trainer import Trainer, default_config
    AR.install(monkeypatch)
    entry = OPTIMIZER_CHOICE["torch-adafactor"]
    assert entry["class"] is St355Adafactor and entry["precision"] == "any"
    assert entry["default_settings"] == {"beta2_decay": -0.8, "eps": (None, 1e-3), "d": 1.0, "weight_decay": 0.0}
    assert optimizer_settings("torch-adafactor", SimpleNamespace(optimizer_config="eps1=1e-6"))["eps"] == (1e-6, 1e-3)       # an explicit eps1 is used as given
    flat, gsteps, poffs = _packed(F32)
    ps = _params(flat, gsteps[0].clone(), poffs, AR.ARENA_SHAPES)
    comp = SimpleNamespace(trainable_parameters=lambda: ps, full=False)
    acc = SimpleNamespace(num_processes=1)
    tr = Trainer(default_config(optimizer="torch-adafactor", optimizer_config="weight_decay=0.01", learning_rate=2e-3), _Plugin(comp), acc)
    assert isinstance(tr.optimizer, St355Adafactor) and tr.optimizer.fuses_ema is False
    group = tr.optimizer.param_groups[0]
    assert group["lr"] == 2e-3 and group["weight_decay"] == 0.01 and group["beta2_decay"] == -0.8 and tuple(group["eps"]) == (None, 1e-3) and group["d"] == 1.0
    # Internal Guidance / NextLat put 1-D tensors into the arena: Adafactor takes them, so neither is refused
    Trainer(default_config(optimizer="torch-adafactor", internal_guidance_enabled=True), _Plugin(comp), acc)
    Trainer(default_config(optimizer="torch-adafactor", nextlat_enabled=True), _Plugin(comp), acc)
    Trainer(default_config(optimizer="torch-adafactor", hip_graph=True), _Plugin(comp), acc)
    with pytest.raises(NotImplementedError) as e:
        Trainer(default_config(optimizer="adamw_schedulefree"), _Plugin(comp), acc)
    assert "torch-adafactor" in str(e.value) and "adamw_schedulefree" in str(e.value)
    with pytest.raises(NotImplementedError, match="lion"):
        Trainer(default_config(optimizer="lion"), _Plugin(comp), acc)
    with pytest.raises(NotImplementedError, match="maximize"):
        Trainer(default_config(optimizer="torch-adafactor", optimizer_config="maximize=true"), _Plugin(comp), acc)
    # the UNet full fine-tune: a trainable set dominated by [Cout, Cin, 3, 3] convolutions
    conv = torch.zeros(32 * 16 * 9 + 32 + 16 * 8, dtype=BF16)
    cps = [torch.nn.Parameter(conv[:32 * 16 * 9].view(32, 16, 3, 3)), torch.nn.Parameter(conv[32 * 16 * 9:32 * 16 * 9 + 32]), torch.nn.Parameter(conv[32 * 16 * 9 + 32:].view(16, 8))]
    unet = SimpleNamespace(trainable_parameters=lambda: cps, full=True)
    with pytest.raises(NotImplementedError, match=r"torch-adafactor.*SDXL / SD 1\.5.*3 x 3"):
        Trainer(default_config(optimizer="torch-adafactor", model_family="sdxl", model_type="full"), _Plugin(unet), acc)
    Trainer(default_config(optimizer="torch-adafactor", model_family="sdxl"), _Plugin(SimpleNamespace(trainable_parameters=lambda: ps, full=False)), acc)     # its LoRA arena is 2-D: built


def test_sd3_full_parameter_shapes_are_the_checkpoints():
    """the factorisation is taken from the parameters as the component exposes them: they must have the shapes diffusers_state_dict() saves (the
    reference's tensors), or the row / column split and the per-tensor RMS / clip would differ from the reference's"""
    from tests import ops_emulator as EMU
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    from tests.test_trainer_host_loop_cpu import _acc
    mp = pytest.MonkeyPatch()
    try:
        EMU.install(mp)
        cfg = default_config(model_family="sd3", model_type="full", train_batch_size=1, seed=5)
        plugin = SD3(cfg, _acc())
        plugin.load_model(sample_size=32, num_layers=2, num_attention_heads=2, attention_head_dim=64, joint_attention_dim=128, caption_projection_dim=128,
                          pooled_projection_dim=64, pos_embed_max_size=24)
        plugin.freeze_components()
        model = plugin.get_trained_component()
        saved = model.diffusers_state_dict()
        named = dict(model.named_parameters())
        full = model.trainable_parameters()
        assert len(full) == len(named) and {id(p) for p in full} == {id(p) for p in named.values()}
        for name, p in named.items():
            assert name in saved and tuple(saved[name].shape) == tuple(p.shape), name
        assert tuple(named["pos_embed.proj.weight"].shape)[-2:] == (2, 2) and named["pos_embed.proj.weight"].dim() == 4
    finally:
        mp.undo()


def _sd3(monkeypatch, model_type, **kw):
    from tests import ops_emulator as EMU
    from tests import parity_utils as PU
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import Trainer, default_config
    from tests.test_trainer_host_loop_cpu import _acc
    EMU.install(monkeypatch)
    AR.install(monkeypatch)
    cfg = default_config(model_family="sd3", model_type=model_type, train_batch_size=1, seed=5, learning_rate=1e-2, flow_schedule_shift=3.0, optimizer="torch-adafactor", **kw)
    plugin = SD3(cfg, _acc())
    plugin.load_model(sample_size=32, num_layers=1, num_attention_heads=2, attention_head_dim=64, joint_attention_dim=128, caption_projection_dim=128,
                      pooled_projection_dim=64, pos_embed_max_size=24)
    if model_type == "lora":
        plugin.add_lora_adapter()
    else:
        plugin.freeze_components()
    trainer = Trainer(cfg, plugin, plugin.accelerator)
    _, devt = PU.make_inputs(1, 8, 8, 16, 128, 64, "cpu", seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


def test_host_loop_sd3_lora_steps_saves_and_resumes_bit_equal(monkeypatch, tmp_path):
    from simpletuner_amd.training.optimizer import St355Adafactor
    plugin, trainer, batch = _sd3(monkeypatch, "lora", lora_rank=6, lora_init_b_std=0.0)
    assert isinstance(trainer.optimizer, St355Adafactor)
    model = plugin.get_trained_component()
    start = model.lora_flat.clone()
    trainer.train_step(dict(batch))
    assert not torch.equal(model.lora_flat, start) and trainer.optimizer.abi_calls == 1          # B starts at zero: the eps2 floor moves it
    trainer.train_step(dict(batch))
    ck = str(tmp_path / "checkpoint-2")
    trainer.save_state(ck)
    tail_a = [trainer.train_step(dict(batch)).item() for _ in range(2)]
    plugin2, trainer2, _ = _sd3(monkeypatch, "lora", lora_rank=6, lora_init_b_std=0.0)
    trainer2.load_state(ck)
    tail_b = [trainer2.train_step(dict(batch)).item() for _ in range(2)]
    assert tail_a == tail_b and torch.equal(model.lora_flat, plugin2.get_trained_component().lora_flat)
    a, b = trainer.optimizer._flat[0], trainer2.optimizer._flat[0]
    assert a["step"] == b["step"] == 4 and all(torch.equal(a[k], b[k]) for k in ("row_var", "col_var", "variance"))


def test_host_loop_sd3_full_fine_tune_with_ema_steps_saves_and_resumes_bit_equal(monkeypatch, tmp_path):
    from simpletuner_amd.training.optimizer import St355Adafactor
    plugin, trainer, batch = _sd3(monkeypatch, "full", use_ema=True, ema_decay=0.9)
    assert isinstance(trainer.optimizer, St355Adafactor) and trainer.ema_model is not None
    model = plugin.get_trained_component()
    start = model.arena.clone()
    shadow0 = trainer.ema_model.shadow_flat.clone()
    for _ in range(2):
        trainer.train_step(dict(batch))
    assert not torch.equal(model.arena, start) and model.arena.dtype == BF16
    assert trainer.ema_model.optimization_step == 2 and not torch.equal(trainer.ema_model.shadow_flat, shadow0)      # the EMAModel.step fallback ran
    assert {AB.kind_of(tuple(p.shape)) for p in trainer.params} == {"vec", "mat", "small"}
    n = model.arena.numel()
    st = trainer.optimizer._flat[0]
    assert all(st[k].numel() < n for k in ("row_var", "col_var", "variance"))
    ck = str(tmp_path / "checkpoint-2")
    trainer.save_state(ck)
    tail_a = [trainer.train_step(dict(batch)).item() for _ in range(2)]
    plugin2, trainer2, _ = _sd3(monkeypatch, "full", use_ema=True, ema_decay=0.9)
    with torch.no_grad():
        plugin2.get_trained_component().arena.add_(0.25)
    trainer2.load_state(ck)
    tail_b = [trainer2.train_step(dict(batch)).item() for _ in range(2)]
    assert tail_a == tail_b and torch.equal(model.arena, plugin2.get_trained_component().arena)


def test_launch_trace_of_the_host_sequencing_tests_is_the_parents(tmp_path):
    """flag off, nothing moved: tools/launch_trace.py over the existing SD3 host-sequencing tests (`-k test_sd3_host_sequencing`: every emulated launch of
    the LoRA and full fine-tune steps with its operands' dtypes, shapes and strides, in order; the Flux stream is pinned the same way by tests/test_layersync_cpu.py) gives, byte for byte, the file it gave at the parent commit, whose
    digest was recorded there (tests/golden/adafactor_launch_trace.sha256)"""
    import hashlib
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "launch_trace.py"), str(out), "-k", "test_sd3_host_sequencing"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = (ROOT / "tests" / "golden" / "adafactor_launch_trace.sha256").read_text().strip()
    # A later change that legitimately alters what an SD3 step launches fails here by design.  It then records the digest anew — at ITS parent commit when it
    # must show "flag off, nothing moved" for a feature of its own (in a golden file and a test of its own), and deletes this test and its golden file with a
    # line in its list of removed tests: the property belongs to the commit that added Adafactor, not to the tree for ever.
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

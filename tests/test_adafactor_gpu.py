"""Adafactor on the MI355X (simpletuner_amd/csrc/adafactor.hip): the five launches through the C ABI on the mixed arena of tests/adafactor_ref.py, as
an fp32 and as a bf16 instance, bounded element-wise against the fp64 restatement (tests/adafactor_bounds.py), bit-identical run to run, pads
untouched; the CPU stand-in against the kernels op by op; and the optimizer through SD3 LoRA and SD3 full fine-tune + EMA train steps."""
import re
from pathlib import Path

import pytest
import torch

from simpletuner_amd import ops
from tests import adafactor_bounds as AB
from tests import adafactor_ref as AR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ROOT = Path(__file__).resolve().parent.parent
SENTINEL = 12345.0            # exactly representable in bf16 and fp32
TAIL = 24                     # sentinel elements behind every state buffer
HP = dict(beta2_decay=-0.8, eps2=1e-3, d=1.0)
_ARENAS = {}


def _arena(dtype):
    """the shared arena, made once per dtype and never modified (the tests clone it)"""
    if dtype not in _ARENAS:
        offs, n, p0, gs = AR.make_arena(dtype)
        pads = AR.pad_mask(offs, n)
        p0, gs = p0.clone(), [g.clone() for g in gs]
        p0[pads] = SENTINEL
        for g in gs:
            g[pads] = SENTINEL
        _ARENAS[dtype] = (offs, n, p0, gs, pads)
    return _ARENAS[dtype]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _state_views(plan, rv, cv, var):
    """torch's per-tensor layout over the flat state buffers (CPU clones)"""
    rv, cv, var = rv.cpu(), cv.cpu(), var.cpu()
    out = []
    for i, (b, R, C) in enumerate(plan.factors):
        if R == 0:
            out.append({"variance": var[plan.var_offsets[i]:plan.var_offsets[i] + C].clone()})
        else:
            out.append({"row_var": rv[plan.rv_offsets[i]:plan.rv_offsets[i] + b * R].view(b, R, 1).clone(),
                        "col_var": cv[plan.cv_offsets[i]:plan.cv_offsets[i] + b * C].view(b, 1, C).clone()})
    return out


def _fresh_state(plan):
    bufs = [torch.zeros(k + TAIL, dtype=F32, device=DEV) for k in (plan.rv_len, plan.cv_len, plan.var_len)]
    for b, k in zip(bufs, (plan.rv_len, plan.cv_len, plan.var_len)):
        b[k:] = SENTINEL
    return bufs


def _run(dtype, wd, gs, check):
    """three steps from the arena's start; returns the final (p, row_var, col_var, variance) and, if check, the worst |err| / bound"""
    offs, n, p0, grads, pads = _arena(dtype)
    plan = ops.AdafactorPlan(offs, AR.ARENA_SHAPES, DEV)
    p = p0.to(DEV)
    rv, cv, var = _fresh_state(plan)
    eps1 = torch.finfo(dtype).eps
    worst, inter = 0.0, []
    for k in range(AR.STEPS):
        g = grads[k].to(DEV)
        before_p, before_s = p.cpu(), _state_views(plan, rv, cv, var)
        ops.adafactor_step(plan, p, g, rv, cv, var, k + 1, AR.LR, weight_decay=wd, grad_scale=gs, **HP)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g.cpu()), _bits(grads[k])), "the gradient arena was written"
        if check:
            c = AB.consts(k + 1, AR.LR, HP["beta2_decay"], eps1, HP["eps2"], HP["d"], wd, gs)
            worst, xs = AB.check_step(f"{dtype} wd {wd} gs {gs} step {k + 1}", AR.ARENA_SHAPES, AR.tensors_of(before_p, offs), AR.tensors_of(grads[k], offs), before_s,
                                      AR.tensors_of(p.cpu(), offs), _state_views(plan, rv, cv, var), c, dtype, worst)
            inter.append(xs)
    out = (p.cpu(), rv.cpu(), cv.cpu(), var.cpu())
    assert bool((out[0][pads] == SENTINEL).all()), "a pad element of the arena was written"
    for buf, k in zip(out[1:], (plan.rv_len, plan.cv_len, plan.var_len)):
        assert bool((buf[k:] == SENTINEL).all()), "an element behind a state buffer was written"
    assert all(bool(torch.isfinite(t[:k].float()).all()) for t, k in zip(out[1:], (plan.rv_len, plan.cv_len, plan.var_len)))
    assert bool(torch.isfinite(out[0][~pads].float()).all())
    return out, worst, inter


@pytest.mark.parametrize("wd,gs", AR.CASES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_kernels_are_bounded_element_wise_deterministic_and_leave_the_pads_alone(dtype, wd, gs):
    first, worst, inter = _run(dtype, wd, gs, check=True)
    second, _, _ = _run(dtype, wd, gs, check=False)
    for a, b, what in zip(first, second, ("p", "row_var", "col_var", "variance")):
        assert torch.equal(_bits(a), _bits(b)), f"{what} differs between two runs from the same start"
    eps1 = torch.finfo(dtype).eps
    denoms = [float(x["denom"]) for xs in inter for x in xs]
    assert any(d > 1.0 for d in denoms) and any(d == 1.0 for d in denoms)                 # the clip acts on some tensors and not on others
    assert float(inter[0][AR.ZERO_TENSOR]["rms"]) == 0.0                                 # the eps2 floor decides alpha there
    v = inter[0][AR.PART_CLAMPED]["v"]
    assert bool((v < eps1 * eps1).any()) and bool((v > eps1 * eps1).any())                 # the eps1^2 clamp acts on part of a tensor
    assert bool((inter[0][AR.ROW_MEAN_CLAMPED]["rm"] == AB.f32(eps1)).all())               # the eps1 clamp on the row mean acts
    assert not torch.equal(first[0], _arena(dtype)[2])
    print(f"[adafactor] {dtype} weight_decay {wd} grad_scale {gs}: worst |err| / bound over {len(AR.ARENA_SHAPES)} tensors x {AR.STEPS} steps = {worst:.3f}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_stand_in_and_kernels_agree_op_by_op_within_the_same_bounds(dtype):
    """each of the three steps from the KERNELS' stored state: the stand-in's result and the kernels' result both lie inside the interval around the
    fp64 restatement of that step, so they differ by at most its width"""
    wd, gs = 0.01, 0.5
    offs, n, p0, grads, pads = _arena(dtype)
    plan, cpu_plan = ops.AdafactorPlan(offs, AR.ARENA_SHAPES, DEV), AR.AdafactorPlanCPU(offs, AR.ARENA_SHAPES, None)
    assert (plan.rv_len, plan.cv_len, plan.var_len) == (cpu_plan.rv_len, cpu_plan.cv_len, cpu_plan.var_len)
    assert (plan.rv_offsets, plan.cv_offsets, plan.var_offsets, plan.factors) == (cpu_plan.rv_offsets, cpu_plan.cv_offsets, cpu_plan.var_offsets, cpu_plan.factors)
    p = p0.to(DEV)
    rv, cv, var = _fresh_state(plan)
    eps1 = torch.finfo(dtype).eps
    worst_k = worst_s = 0.0
    for k in range(AR.STEPS):
        sp, srv, scv, svar = p.cpu().clone(), rv.cpu()[:plan.rv_len].clone(), cv.cpu()[:plan.cv_len].clone(), var.cpu()[:plan.var_len].clone()
        before_p, before_s = p.cpu(), _state_views(plan, rv, cv, var)
        AR.adafactor_step_cpu(cpu_plan, sp, grads[k], srv, scv, svar, k + 1, AR.LR, weight_decay=wd, grad_scale=gs, **HP)
        ops.adafactor_step(plan, p, grads[k].to(DEV), rv, cv, var, k + 1, AR.LR, weight_decay=wd, grad_scale=gs, **HP)
        torch.cuda.synchronize()
        c = AB.consts(k + 1, AR.LR, HP["beta2_decay"], eps1, HP["eps2"], HP["d"], wd, gs)
        args = (AR.ARENA_SHAPES, AR.tensors_of(before_p, offs), AR.tensors_of(grads[k], offs), before_s)
        worst_k, _ = AB.check_step(f"kernels step {k + 1}", *args, AR.tensors_of(p.cpu(), offs), _state_views(plan, rv, cv, var), c, dtype, worst_k)
        worst_s, _ = AB.check_step(f"stand-in step {k + 1}", *args, AR.tensors_of(sp, offs), _state_views(cpu_plan, srv, scv, svar), c, dtype, worst_s, any_order=True)
    print(f"[adafactor] {dtype} op by op: worst |err| / bound kernels {worst_k:.3f}, stand-in {worst_s:.3f}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_an_explicit_eps1_whose_square_is_zero_in_fp32_keeps_the_clip(dtype):
    """eps1 = 1e-30 (the paper's value) is used as given; its square is 0 in fp32, so a lane past the end of a tile row would compute u = 0 * rsq(0) = NaN: such
    lanes must not reach the sum of u^2, or max(1, NaN) silently switches the clip off.  Three tensors of the shared arena through a plan of their own —
    (40, 8), (4, 33) and (130, 257): every tile row of them has lanes past its end, and the clip acts on (130, 257) — against the fp64 restatement; the
    rest of the arena is not in the plan and must stay untouched"""
    eps1, wd, gs = 1e-30, 0.01, 1.0
    pick = [1, AR.PART_CLAMPED, 3]
    offs_all, n, p0, grads, pads = _arena(dtype)
    shapes, offs = [AR.ARENA_SHAPES[i] for i in pick], [offs_all[i] for i in pick]
    assert AB.f32(eps1 * eps1) == 0.0 and all(s[-1] % 256 for s in shapes)
    plan = ops.AdafactorPlan(offs, shapes, DEV)
    p = p0.to(DEV)
    rv, cv, var = _fresh_state(plan)
    outside = AR.pad_mask(offs, n, shapes)                     # pads and the tensors that are not in the plan
    worst, denoms = 0.0, []
    for k in range(AR.STEPS):
        before_p, before_s = p.cpu(), _state_views(plan, rv, cv, var)
        ops.adafactor_step(plan, p, grads[k].to(DEV), rv, cv, var, k + 1, AR.LR, eps1=eps1, weight_decay=wd, grad_scale=gs, **HP)
        torch.cuda.synchronize()
        c = AB.consts(k + 1, AR.LR, HP["beta2_decay"], eps1, HP["eps2"], HP["d"], wd, gs)
        worst, xs = AB.check_step(f"eps1 1e-30 {dtype} step {k + 1}", shapes, AR.tensors_of(before_p, offs, shapes), AR.tensors_of(grads[k], offs, shapes), before_s,
                                  AR.tensors_of(p.cpu(), offs, shapes), _state_views(plan, rv, cv, var), c, dtype, worst)
        denoms.append(float(xs[2]["denom"]))
        assert bool(torch.isfinite(p.cpu()[~outside].float()).all())
    assert max(denoms) > 1.0, denoms                            # the clip acts on (130, 257) in the restatement: a kernel without it leaves the bound
    assert torch.equal(_bits(p.cpu()[outside]), _bits(p0[outside]))
    print(f"[adafactor] {dtype} eps1 1e-30: worst |err| / bound = {worst:.3f}, denom of (130, 257) per step {[round(d, 3) for d in denoms]}")


# ---- through the trainer --------------------------------------------------------------------------------------------------------------------------
def _record(monkeypatch):
    calls = []
    real = ops.adafactor_step

    def rec(plan, p, g, rv, cv, var, step, lr, beta2_decay=-0.8, eps1=None, eps2=1e-3, d=1.0, weight_decay=0.0, grad_scale=1.0):
        before = dict(p=p.cpu(), g=g.cpu(), rv=rv.cpu(), cv=cv.cpu(), var=var.cpu())
        real(plan, p, g, rv, cv, var, step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale)
        torch.cuda.synchronize()
        calls.append(dict(plan=plan, before=before, hp=(step, lr, beta2_decay, eps1, eps2, d, weight_decay, grad_scale), after=dict(p=p.cpu(), rv=rv.cpu(), cv=cv.cpu(), var=var.cpu())))

    monkeypatch.setattr(ops, "adafactor_step", rec)
    return calls


def _check_calls(calls, params, what):
    """every recorded device step against (a) the fp64 restatement of its stored inputs and (b) the CPU stand-in run of the same step: both inside the
    derived interval, hence within its width of each other — tighter than any tolerance the SD3 step tests state"""
    shapes = [tuple(p.shape) for p in params]
    base, esz = params[0].data_ptr(), params[0].element_size()
    offs = [(p.data_ptr() - base) // esz for p in params]
    worst_k = worst_s = 0.0
    for k, cl in enumerate(calls):
        plan, b, a = cl["plan"], cl["before"], cl["after"]
        step, lr, b2d, eps1, eps2, d, wd, gs = cl["hp"]
        dtype = b["p"].dtype
        eps1 = torch.finfo(dtype).eps if eps1 is None else eps1
        assert step == k + 1 and plan.n == len(params)
        cpu_plan = AR.AdafactorPlanCPU(offs, shapes, None)
        sp, srv, scv, svar = b["p"].clone(), b["rv"].clone(), b["cv"].clone(), b["var"].clone()
        AR.adafactor_step_cpu(cpu_plan, sp, b["g"], srv, scv, svar, step, lr, b2d, eps1, eps2, d, wd, gs)
        c = AB.consts(step, lr, b2d, eps1, eps2, d, wd, gs)
        args = (shapes, AR.tensors_of(b["p"], offs, shapes), AR.tensors_of(b["g"], offs, shapes), _state_views(plan, b["rv"], b["cv"], b["var"]))
        worst_k, _ = AB.check_step(f"{what} step {step} kernels", *args, AR.tensors_of(a["p"], offs, shapes), _state_views(plan, a["rv"], a["cv"], a["var"]), c, dtype, worst_k)
        worst_s, _ = AB.check_step(f"{what} step {step} stand-in", *args, AR.tensors_of(sp, offs, shapes), _state_views(cpu_plan, srv, scv, svar), c, dtype, worst_s,
                                   any_order=True)
        assert not torch.equal(_bits(a["p"]), _bits(b["p"])), "the step moved nothing"
    print(f"[adafactor] {what}: {len(calls)} steps through the trainer, worst |err| / bound kernels {worst_k:.3f}, stand-in {worst_s:.3f}")


def _batch(devt):
    return {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}


def test_sd3_lora_steps_through_the_trainer(monkeypatch):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.optimizer import St355Adafactor
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    from tests.test_sd3_model_gpu import _arch
    cfg = default_config(model_family="sd3", lora_rank=6, seed=5, lora_init_b_std=0.0, learning_rate=1e-2, flow_schedule_shift=3.0, optimizer="torch-adafactor",
                         optimizer_config="weight_decay=0.01")
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(2))
    plugin.add_lora_adapter()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Adafactor)
    _, devt = PU.make_inputs(1, 16, 16, 24, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    calls = _record(monkeypatch)
    for _ in range(2):
        trainer.train_step(_batch(devt))
    torch.cuda.synchronize()
    model = plugin.get_trained_component()
    assert len(calls) == 2 and all(c["before"]["p"].dtype == F32 and c["before"]["p"].numel() == model.lora_flat.numel() for c in calls)
    assert trainer.optimizer.abi_calls == 2 and calls[0]["plan"].var_len == 0                     # rank 6: no dimension a multiple of 8; all 2-D
    _check_calls(calls, trainer.params, "sd3 lora r6")
    st = trainer.optimizer._flat[0]
    assert st["row_var"].numel() + st["col_var"].numel() == sum(p.shape[0] + p.shape[1] for p in trainer.params) < model.lora_flat.numel()


def test_sd3_full_finetune_with_ema_steps_through_the_trainer(monkeypatch):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.optimizer import St355Adafactor
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    from tests.test_sd3_model_gpu import _arch
    cfg = default_config(model_family="sd3", model_type="full", train_batch_size=1, seed=5, learning_rate=1e-2, flow_schedule_shift=3.0, use_ema=True, ema_decay=0.99,
                         optimizer="torch-adafactor")
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(2))
    plugin.enable_full_finetune()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Adafactor) and trainer.optimizer.fuses_ema is False
    _, devt = PU.make_inputs(1, 16, 16, 24, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    shadow0 = trainer.ema_model.shadow_flat.clone()
    calls = _record(monkeypatch)
    for _ in range(2):
        trainer.train_step(_batch(devt))
    torch.cuda.synchronize()
    n = sum(p.numel() for p in trainer.params)
    assert len(calls) == 2 and all(c["before"]["p"].dtype == BF16 and c["before"]["p"].numel() == n and c["hp"][3] is None for c in calls)
    kinds = {AB.kind_of(tuple(p.shape)) for p in trainer.params}
    assert kinds == {"vec", "mat", "small"}, kinds                                                # biases, matrices and the 2 x 2 patch embedding
    _check_calls(calls, trainer.params, "sd3 full")
    assert trainer.ema_model.optimization_step == 2 and not torch.equal(trainer.ema_model.shadow_flat, shadow0)      # EMAModel.step ran (no fused form)
    st = trainer.optimizer._flat[0]
    fac = [AR.factor_shape(tuple(p.shape)) for p in trainer.params]
    want = 4 * sum(b * (R + C) for b, R, C in fac if R) + 4 * sum(C for b, R, C in fac if not R)
    assert sum(st[k].numel() * st[k].element_size() for k in ("row_var", "col_var", "variance")) == want      # the state is exactly the factors and the 1-D variances
    assert all(st[k].numel() < n for k in ("row_var", "col_var", "variance"))                                 # no buffer of the arena's length


def test_abi_exports_the_adafactor_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    L = lib.load()
    for s in ("st355_adafactor_plan", "st355_adafactor_workspace_floats", "st355_adafactor_step"):
        assert re.search(r"\b(int|int64_t) " + s + r"\(", header), s
        assert s in lib.SYMBOLS and hasattr(L, s), s

"""TwinFlow (RCGM) on the CPU: the settings, the ValueErrors, the per-sample times, the loss and the UCGM sampler against the EXECUTED reference
(tests/golden/twinflow_vectors.pt, written by tools/gen_twinflow_golden.py), the stand-ins inside the kernels' derived bounds, the tiny SD3 and Flux plugins on the
kernel-contract emulator against an oracle step that composes the oracle model with the restated rule, the teacher's contract, the refusals, and the flag-absent
route."""
import hashlib
import logging
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from oracle import flux as OF
from oracle import sd3 as OS
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests import twinflow_bounds as TB
from tests import twinflow_ref as TR

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = SimpleNamespace
DT = {"torch.float64": F64, "torch.float32": F32, "torch.bfloat16": BF16}

# The fp64 restatement against the executed fp64 records.  The two sides differ only in how they round: the reference forms x_hat, z_hat and
# t_next z_hat + (1 - t_next) x_hat where the restatement forms x + (t_next - t_prev) F — at most ROUNDINGS = 6 roundings apart per element and step, each of
# relative size u64 = 2^-53 on quantities of magnitude at most MAG = 32 (|x|, |F|, |acc| of the recorded cases stay below it); a difference in x is carried into
# the next steps' teacher forwards, whose Lipschitz constant is at most sum |w + dw| = 2.6 of the stand-in model, so over the at most STEPS = 3 steps it grows by at
# most LIP2 = 2.6^2 < 7; the loss terms are squares (factor 2 MAG is inside MAG's margin: the residuals stay below 4).
ROUNDINGS, STEPS, LIP2, MAG = 6, 3, 7, 32
TOL64 = 2.0 ** -53 * ROUNDINGS * STEPS * LIP2 * MAG * 2
TOL32 = 2.0 ** -24 * ROUNDINGS * STEPS * LIP2 * MAG * 2          # the same count with the fp32 records' unit roundoff
# The reference casts the prediction and both targets to fp32 (`.float()`) before each mse_loss, in every run, so a record's loss, logs and gradient carry fp32
# roundings whatever the run's dtype: p and the target round by u32 (|p| + |target|) <= u32 * 2 * ELEM (ELEM = 8 bounds the recorded elements), their difference d
# (|d| <= RES = 8 covers the clamped and the unclamped residuals of the records) by u32 more; d^2 doubles it; torch's fp32 mean adds at most (1 + log2 N) u32 of the value (pairwise), the sum of the two terms and the fp32 log one u32 each.
ELEM, RES, U32 = 8.0, 8.0, 2.0 ** -24


def loss_tol(value, n):
    import math
    return U32 * (2 * RES * (2 * ELEM + RES) + (3 + math.ceil(math.log2(n))) * max(1.0, abs(value)))


def grad_tol(n):
    return U32 * 2 * (2 * ELEM + RES) * 2.0 / n * 2          # two terms, each (2 / N) d with d rounded as above


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(ROOT, "tests", "golden", "twinflow_vectors.pt"), weights_only=False)


# ------------------------------------------------------------------------------------------------
# (a) settings and the reference's ValueErrors
# ------------------------------------------------------------------------------------------------
def test_settings_defaults_and_none_handling_equal_the_executed_reference(G):
    from simpletuner_amd import twinflow as TW
    for name, rec in G["config"]["settings"].items():
        assert TW.settings(NS(**rec["config"])) == rec["settings"], name
    d = TW.settings(NS())
    assert (d["estimate_order"], d["enhanced_ratio"], d["target_step_count"], d["delta_t"], d["clamp_target"]) == (2, 0.5, 1, 0.01, 1.0)


def test_validation_raises_the_references_value_errors(G):
    from simpletuner_amd import twinflow as TW
    c = G["config"]
    for name in ("not_flow", "not_flow_one_flag", "no_ema"):
        rec = c["errors"][name]
        with pytest.raises(ValueError) as ei:
            TW.validate(NS(**rec["config"]), rec["prediction"] == "flow_matching")
        assert str(ei.value) == rec["message"], name
    assert c["errors"]["active_not_flow"]["message"].startswith("TwinFlow is only supported for flow-matching models.")
    assert TW.E_TEACHER_NO_EMA == c["errors"]["teacher_context_no_ema"]["message"]
    for name, rec in c["passes"].items():
        assert TW.validate(NS(**rec["config"]), rec["prediction"] == "flow_matching") == rec["bridge"], name


# ------------------------------------------------------------------------------------------------
# (b) the per-sample times
# ------------------------------------------------------------------------------------------------
def _times(case):
    from simpletuner_amd import twinflow as TW
    wd = DT[case["dtype"]]
    batch = {"sigmas": case["sigmas"].view(-1, 1, 1, 1).clone(), "timesteps": case["sigmas"] * 1000.0, "twinflow_uniforms": case["uniforms"]}
    TW.prepare_metadata(batch)
    tt1 = batch["twinflow_tt"]
    sw, tt2 = TW.cap_tt(tt1.reshape(-1), batch["sigmas"].reshape(-1), wd)
    sched = TW.time_schedule(sw, tt2, case["order"], 0.01)
    return tt1, sw, tt2, sched


@pytest.mark.parametrize("dt", ["fp64", "fp32", "bf16"])
def test_tt_rule_and_time_schedule_equal_the_executed_reference(G, dt):
    """both caps, with the eps of the dtype the reference has at each site (recorded: fp32 sigmas at site 1 whatever the weight dtype; the weight dtype at site 2, so a
    bf16 run caps at bf16(sigma) - 2^-7), tt going negative for a sigma below eps, and the timestep of every teacher forward.  Exact for all three dtypes: the times
    are [B]-sized torch expressions in the reference's own dtypes."""
    from simpletuner_amd import twinflow as TW
    for name, case in G["losses"].items():
        if not name.startswith(dt + ".") or name.endswith("student"):
            continue
        tt1, sw, tt2, sched = _times(case)
        assert tt1.dtype == case["tt_site1"].dtype and tt1.shape == case["tt_site1"].shape and torch.equal(tt1, case["tt_site1"]), name
        assert tt2.dtype == case["tt_site2"].dtype and torch.equal(tt2, case["tt_site2"].reshape(-1)), name
        r1, rsw, r2, rs = TR.times_ref(case["sigmas"], case["uniforms"], DT[case["dtype"]], case["order"], 0.01)
        assert torch.equal(r1, tt1.reshape(-1)) and torch.equal(r2, tt2) and all(torch.equal(a, b) for a, b in zip(rs, sched))
        rcgm_calls = [c for c in case["calls"] if c["cond"] == "cond"][(1 if case["negative"] and case["ratio"] > 0 else 0):]
        assert len(rcgm_calls) == case["order"]
        for c, t_prev in zip(rcgm_calls, [sw] + sched[:-1]):
            assert torch.equal(TW.teacher_timesteps(t_prev), c["timesteps"].to(F32)), name
            # the sign travels apart (-1 where a time below eps went negative) and indexes the zero-initialised table, frozen under LoRA: it adds nothing
            assert torch.equal(c["sign"].to(F64), torch.where(t_prev.to(F64) < 0, -1.0, 1.0).to(F64)), name
    eps32 = G["losses"]["fp32.order2.ratio0.0.neg0.clamp1.0"]
    assert eps32["site1"]["eps"] == 2.0 ** -23 and float(eps32["tt_site1"].reshape(-1)[3]) < 0.0          # the sigma below eps: tt = sigma - eps < 0
    b = G["losses"]["bf16.order2.ratio0.0.neg0.clamp1.0"]
    assert b["site1"]["dtype"] == "torch.float32" and b["site2"] == dict(dtype="torch.bfloat16", eps=2.0 ** -7, shape=(5, 1, 1, 1), tt_dtype="torch.float32")


def test_a_given_tt_is_clamped_and_tokenwise_timesteps_are_refused():
    from simpletuner_amd import twinflow as TW
    s = torch.tensor([0.5, 0.25, 0.75]).view(3, 1, 1, 1)
    batch = {"sigmas": s, "timesteps": s.reshape(3) * 1000.0, "twinflow_tt": torch.tensor([-0.1, 0.1, 0.9])}
    TW.prepare_metadata(batch)
    assert torch.equal(batch["twinflow_tt"].reshape(-1), torch.tensor([0.0, 0.1, 0.75 - 2.0 ** -23]))
    with pytest.raises(NotImplementedError, match=r"^twinflow_enabled with tokenwise timesteps \(3, 16\) is not built"):
        TW.prepare_metadata({"sigmas": s, "timesteps": torch.zeros(3, 16)})
    torch.manual_seed(1)
    batch = {"sigmas": s.clone(), "timesteps": s.reshape(3) * 1000.0}
    TW.prepare_metadata(batch)
    torch.manual_seed(1)
    assert torch.equal(batch["twinflow_tt"], TW.sample_tt(s, torch.rand_like(s)))          # torch's device RNG, one rand_like(sigmas)


# ------------------------------------------------------------------------------------------------
# (c) the restated rule against the executed loss
# ------------------------------------------------------------------------------------------------
def _restated(G, case, dtype=F64):
    """the fp64 restatement on a record's inputs: (twin, base, realvel, grad)"""
    teacher = case["teacher"] == "ema"
    enc, neg = case["enc"].to(dtype), None if case["neg"] is None else case["neg"].to(dtype)
    F = lambda x, t_prev: TR.stub_predict(G["stub"], x, t_prev.abs() * 1000.0, enc, teacher)
    _, sw, tt2, sched = TR.times_ref(case["sigmas"], case["uniforms"], DT[case["dtype"]], case["order"], 0.01)
    noisy = case["noisy"].to(dtype)
    cond = uncond = None
    if case["ratio"] > 0 and neg is not None:
        ts = sw.abs().to(dtype) * 1000.0
        cond, uncond = TR.stub_predict(G["stub"], noisy, ts, enc, teacher), TR.stub_predict(G["stub"], noisy, ts, neg, teacher)
    states = []
    acc, _ = TR.rcgm64(lambda x, t_prev: states.append(x) or F(x, t_prev), noisy, sw, sched)
    # the state the reference hands each teacher forward (recorded in the run's own dtype): the integration itself, without the fp32 cast of the loss
    rcgm_calls = [c for c in case["calls"] if c["cond"] == "cond"][(1 if cond is not None else 0):]
    for c, x in zip(rcgm_calls, states):
        if case["dtype"] == "torch.bfloat16":          # (the bf16 records round every intermediate: reported by the caller, not asserted)
            continue
        assert float((c["noisy"].to(F64) - x).abs().max()) <= (TOL64 if case["dtype"] == "torch.float64" else TOL32), case["name"]
    pred = case["pred"].to(dtype).clone().requires_grad_(True)
    target = (case["noise"].to(dtype) - case["latents"].to(dtype))
    twin, base, real = TR.loss64(pred, target, acc.to(dtype), cond, uncond, case["ratio"], case["clamp"])
    (grad,) = torch.autograd.grad(twin, pred)
    closed = TR.twinflow64(pred, target, acc, cond, uncond, case["ratio"], case["clamp"])
    assert torch.allclose(closed["dpred"], grad, rtol=0, atol=TOL64) and torch.allclose(closed["losses"], torch.stack([base, real]).detach(), rtol=0, atol=TOL64)
    return twin.detach(), base.detach(), real.detach(), grad


@pytest.mark.parametrize("dt,tol", [("fp64", TOL64), ("fp32", TOL32)])
def test_restatement_equals_the_executed_reference_loss_logs_and_gradient(G, dt, tol):
    """x + (t_next - t_prev) F_c against the reference's t_next z_hat + (1 - t_next) x_hat, the clamp's closed-form gradient against its autograd: the tolerance is
    the derived rounding distance TOL64 (TOL32 for the fp32 records) on the integration's states, plus the fp32 cast the reference itself applies before its
    mse_loss on the loss, the logs and the gradient (loss_tol / grad_tol), see the top of this file"""
    n = 0
    for name, case in G["losses"].items():
        if not name.startswith(dt + "."):
            continue
        twin, base, real, grad = _restated(G, case)
        N = case["pred"].numel()
        assert abs(float(twin) - float(case["loss"])) <= tol + loss_tol(float(twin), N), (name, float(twin), float(case["loss"]))
        assert abs(float(base) - case["logs"]["twinflow_base"]) <= tol + loss_tol(float(base), N), name
        assert abs(float(real) - case["logs"]["twinflow_realvel"]) <= tol + loss_tol(float(real), N), name
        assert set(case["logs"]) == {"twinflow_base", "twinflow_realvel"}
        assert float((grad - case["grad"].to(F64)).abs().max()) <= tol * 2.0 / N * 2 + grad_tol(N), name
        n += 1
    assert n == 9


def test_bf16_records_distance_is_printed_not_asserted(G):
    """the reference rounds x_hat, z_hat, x, acc and rcgm to bf16 separately (and promotes x to fp32 after the first step); the kernels keep fp32 with one rounding:
    the distance of the bf16 records from the fp64 restatement on the same inputs is reported (DESIGN.md §7 holds the figures)"""
    worst = 0.0
    for name, case in G["losses"].items():
        if name.startswith("bf16."):
            twin, base, real, _ = _restated(G, case)
            d = abs(float(twin) - float(case["loss"])) / max(1.0, abs(float(twin)))
            worst = max(worst, d)
            print(f"[bf16 record] {name}: executed {float(case['loss']):.6f} restated {float(twin):.6f} rel {d:.3e}")
    print(f"[bf16 record] worst relative distance {worst:.3e}")


def test_the_reference_calls_recorded_match_the_structure_this_path_builds(G):
    for name, case in G["losses"].items():
        pair = case["negative"] and case["ratio"] > 0
        conds = [c["cond"] for c in case["calls"]]
        assert conds == (["cond", "uncond"] if pair else []) + ["cond"] * case["order"], name
        assert all(c["teacher"] == (case["teacher"] == "ema") and not c["grad"] for c in case["calls"])


# ------------------------------------------------------------------------------------------------
# (d) the stand-ins inside the kernels' derived bounds
# ------------------------------------------------------------------------------------------------
def clamp_inputs(B, N, seed, pair):
    """operands of the loss with the residual r scaled so that a good share of the elements is clamped at clamp = 1 and a good share is not"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(B, N, generator=g)
    pred, target = rnd().to(BF16), rnd().to(BF16)
    cond, uncond = (rnd().to(BF16), rnd().to(BF16)) if pair else (None, None)
    # r = pred - t' - acc is set per element: every other one inside both clamps used (|r| in [0.05, 0.2]), the rest outside both (|r| in [1.5, 3])
    mag = torch.where(torch.arange(N) % 2 == 0, 0.05 + 0.15 * torch.rand(B, N, generator=g), 1.5 + 1.5 * torch.rand(B, N, generator=g))
    r = mag * torch.where(torch.rand(B, N, generator=g) < 0.5, -1.0, 1.0)
    t = target.float() + (0.5 * (cond.float() - uncond.float()) if pair else 0.0)
    return pred, target, (pred.float() - t - r).contiguous(), cond, uncond


@pytest.mark.parametrize("B,N", [(1, 8), (2, 4104), (3, 16 * 16 * 16)])
def test_stand_ins_sit_inside_the_derived_bounds_and_round_once(B, N):
    g = torch.Generator().manual_seed(B * 1000 + N)
    x, fc = torch.randn(B, N, generator=g).to(BF16), torch.randn(B, N, generator=g).to(BF16)
    acc = torch.randn(B, N, generator=g)
    t_prev, t_next = torch.rand(B, generator=g) * 0.5 + 0.5, torch.rand(B, generator=g) * 0.5
    for first in (True, False):
        ref = TB.rcgm_step_ref(x, acc, fc, t_prev, t_next, first)
        x2, a2 = TR.twinflow_rcgm_step(x.clone(), acc.clone(), fc, t_prev, t_next, first)
        assert TB.inside(x2, *ref["x"])[0] and TB.inside(a2, *ref["acc"])[0]
        assert torch.equal(x2, ref["x"][0].to(BF16)) and torch.equal(a2, ref["acc"][0].to(F32))
    for pair in (False, True):
        pred, target, a, cond, uncond = clamp_inputs(B, N, 7 + B, pair)
        for clamp in (1.0, 0.25):
            ref = TB.loss_ref(pred, target, a, cond, uncond, 0.5, clamp, 1.0)
            losses, dpred = TR.twinflow_loss(pred, target, a, cond, uncond, 0.5, clamp)
            assert TB.inside(losses, *ref["losses"])[0] and TB.inside(dpred, *ref["dpred"])[0]
            assert 0.1 <= ref["clamped"] <= 0.9, ref["clamped"]          # at least 10 % clamped and at least 10 % not, on the fp64 reference
    noise = torch.randn(B, N, generator=g).to(BF16)
    for rho, nz in ((1.0, noise), (0.375, noise), (0.0, None)):
        ref, tol = TB.ucgm_step_ref(x, fc, 0.75, 0.25, rho, nz)
        assert TB.inside(TR.twinflow_ucgm_step(x.clone(), fc, 0.75, 0.25, rho, nz), ref, tol)[0]


# ------------------------------------------------------------------------------------------------
# (e) the plugins on the emulator against the oracle step
# ------------------------------------------------------------------------------------------------
def _acc():
    return NS(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
              backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    TR.install(monkeypatch)
    cfg = default_config(model_family="sd3" if family == "sd35" else family, train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(2, **(dict(qk_norm="rms_norm", dual=(0,)) if family == "sd35" else {})))          # (sd35: the SD3.5 block forms)
    return plugin


UNIFORMS = torch.tensor([0.4, 0.7])


def _trainer(monkeypatch, family, negative=True, perturb_teacher=True, **cfg_kw):
    """the two-block SD3 / the 1 + 1 Flux of tests/test_lora_dropout_cpu.py::_trainer with its inputs (B = 2, 16 x 8 latents, seed 3)"""
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, family, **cfg_kw)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"], "twinflow_uniforms": UNIFORMS}
    if negative:
        g = torch.Generator().manual_seed(99)
        cpu["negative"] = torch.randn(devt["prompt"].shape, generator=g).to(BF16).float()
        batch["negative_prompt_embeds"] = cpu["negative"].to(BF16)
    if perturb_teacher and trainer.ema_model is not None:          # a teacher that is not the student: the shadow moved off the masters
        g = torch.Generator().manual_seed(5)
        trainer.ema_model.shadow_flat.add_(0.02 * torch.randn(trainer.ema_model.shadow_flat.shape, generator=g))
    return plugin, trainer, batch, cpu


def _capture_grads(trainer):
    got = {}
    comp = trainer.model.get_trained_component()
    step = trainer.optimizer.step

    def wrapped(*a, **k):
        got.update({n: p.grad.detach().clone() for n, p in comp.named_parameters() if ".lora_" in n and p.grad is not None})
        return step(*a, **k)
    trainer.optimizer.step = wrapped
    return got


def _teacher_lora(comp, shadow):
    """{target: (A, B)} read from a flat buffer laid out like the adapter arena"""
    base = comp.lora_flat
    view = lambda p: shadow[(p.data_ptr() - base.data_ptr()) // 4:][:p.numel()].view(p.shape).detach().float().cpu().clone()
    A, Bm = {}, {}
    for k, v in comp.named_parameters():
        if ".lora_A." in k:
            A[k.split(".lora_A.")[0]] = view(v)
        elif ".lora_B." in k:
            Bm[k.split(".lora_B.")[0]] = view(v)
    return {k: (A[k], Bm[k]) for k in A}


def oracle_twinflow_step(family, comp, cpu, shadow, order=2, ratio=0.5, clamp=1.0, delta=0.01):
    """the same step in plain torch: oracle forwards (fp32) for every teacher forward with the adapters read from `shadow` (None: the student's), states and
    predictions rounded to bf16 where the engine holds bf16 tensors, the times by tests/twinflow_ref.times_ref in the bf16 weight dtype, the twin term by
    tests/twinflow_ref.loss64 with autograd through the training forward.  Returns (loss, prediction, {target: (dA, dB)}, base, realvel, forwards)."""
    r16 = lambda t: t.to(BF16).float()
    P, lora, scale = PU.oracle_state(comp)
    tl = lora if shadow is None else _teacher_lora(comp, shadow)
    if family in ("sd3", "sd35"):
        P["pos_embed.pos_embed"] = comp.pos_embed.pos_embed.detach().float().cpu()
        ocfg = SH._ocfg(comp)
        fwd = lambda lp, x, prompt, pooled, t: OS.sd3_forward(P, ocfg, x, prompt, pooled, t, lora=lp, lora_scale=scale)
    else:
        ocfg = PU.oracle_cfg(comp)
        fwd = lambda lp, x, prompt, pooled, t: OF.flux_model_predict(P, ocfg, x, prompt, pooled, t, 1.0, lora=lp, lora_scale=scale)
    x, n, sig = cpu["latents"], cpu["noise"], cpu["sigmas"]
    B = x.shape[0]
    s4 = sig.view(B, 1, 1, 1)
    noisy, target = r16((1 - s4) * x + s4 * n), r16(n - x)
    _, sw, tt, sched = TR.times_ref(sig, UNIFORMS, BF16, order, delta)
    ts = lambda s: (s.abs() * 1000.0).float()
    forwards = 0
    cond = uncond = None
    with torch.no_grad():
        if ratio > 0 and cpu.get("negative") is not None:
            cond, uncond = r16(fwd(tl, noisy, cpu["prompt"], cpu["pooled"], ts(sw))), r16(fwd(tl, noisy, cpu["negative"], cpu["pooled"], ts(sw)))
            forwards += 1
        xt, acc, t_prev = noisy.clone(), torch.zeros_like(noisy, dtype=F64), sw
        for t_next in sched:
            fc = r16(fwd(tl, xt, cpu["prompt"], cpu["pooled"], ts(t_prev)))
            h = (t_next.float() - t_prev.float()).double().view(B, 1, 1, 1)
            xt = r16((xt.double() + h * fc.double()).float())
            acc = acc - h * fc.double()
            t_prev = t_next
            forwards += 1
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    pred = fwd(lp, noisy, cpu["prompt"], cpu["pooled"], sig * 1000.0)
    base_loss = ((pred.double() - target.double()) ** 2).reshape(B, -1).mean(1).mean()
    dbl = lambda t: None if t is None else t.double()
    twin, tb, trv = TR.loss64(pred.double(), target.double(), acc.float().double(), dbl(cond), dbl(uncond), ratio, clamp)
    loss = base_loss + twin
    loss.backward()
    return loss.detach(), pred.detach(), {k: (a.grad, b.grad) for k, (a, b) in lp.items()}, float(tb.detach()), float(trv.detach()), forwards


def _compare_grads(got, ref, tol=5e-2):
    worst = 0.0
    assert got
    for name, g in got.items():
        key, which = name.split(".lora_")
        want = ref[key][0 if which.startswith("A") else 1]
        worst = max(worst, PU.rel_l2(g, want))
        assert PU.rel_l2(g, want) < tol, (name, PU.rel_l2(g, want))
    return worst


def _count_forwards(plugin):
    calls = []
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: calls.append((pb["noisy_latents"].shape[0], torch.is_grad_enabled())) or predict(pb)
    return calls


@pytest.mark.parametrize("family,order,ratio,clamp", [("sd3", 2, 0.5, 1.0), ("sd3", 3, 0.0, 0.25), ("flux", 2, 0.5, 1.0), ("flux", 3, 0.0, 0.25), ("sd35", 1, 0.5, 1.0)])
def test_train_step_matches_the_twinflow_oracle(monkeypatch, family, order, ratio, clamp):
    """The tolerances are those the Self-Flow and scheduled-sampling tiny-step tests state for the same quantities: prediction rel-L2 2e-2, loss and logs
    2e-3 * max(1, value), adapter gradients rel-L2 5e-2.  The trace's forward count is 1 + order (+ 1 at batch 2B)."""
    plugin, trainer, batch, cpu = _trainer(monkeypatch, family, twinflow_enabled=True, use_ema=True, twinflow_estimate_order=order, twinflow_enhanced_ratio=ratio,
                                           twinflow_target_clamp=clamp)
    comp = plugin.get_trained_component()
    masters = comp.lora_flat.clone()
    o_loss, o_pred, o_grads, o_base, o_real, o_fwd = oracle_twinflow_step(family, comp, cpu, trainer.ema_model.shadow_flat, order, ratio, clamp)
    calls = _count_forwards(plugin)
    seen = {}
    counted = plugin.model_predict

    def keep(pb):
        out = counted(pb)
        if torch.is_grad_enabled():
            seen["pred"] = out
        return out
    plugin.model_predict = keep
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    pair = ratio > 0
    assert calls == [(2, True)] + ([(4, False)] if pair else []) + [(2, False)] * order and len(calls) == 1 + o_fwd
    assert PU.rel_l2(seen["pred"]["model_prediction"].detach(), o_pred) < 2e-2
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item()), (loss.item(), o_loss.item())
    logs = trainer.last_aux_logs
    assert set(logs) == {"twinflow_base", "twinflow_realvel"} and all(isinstance(v, float) for v in logs.values())
    assert abs(logs["twinflow_base"] - o_base) < 2e-3 * max(1.0, o_base) and abs(logs["twinflow_realvel"] - o_real) < 2e-3 * max(1.0, o_real), (logs, o_base, o_real)
    worst = _compare_grads(grads, o_grads)
    print(f"[emu] {family} order {order} ratio {ratio} clamp {clamp}: loss {loss.item():.5f} vs oracle {o_loss.item():.5f}, logs {logs} vs ({o_base:.5f}, {o_real:.5f}), "
          f"worst adapter gradient rel-L2 {worst:.3e}")


def test_twinflow_adds_its_logs_and_changes_the_loss(monkeypatch):
    """FAILS ON THE PARENT COMMIT (the flag is ignored there: no logs, the flag-off loss)"""
    plugin0, trainer0, batch0, _ = _trainer(monkeypatch, "sd3", use_ema=True)
    l0 = trainer0.train_step(dict(batch0))
    assert trainer0.last_aux_logs is None
    monkeypatch.undo()
    plugin, trainer, batch, _ = _trainer(monkeypatch, "sd3", twinflow_enabled=True, use_ema=True)
    l1 = trainer.train_step(dict(batch))
    logs = trainer.last_aux_logs or {}
    assert "twinflow_base" in logs and "twinflow_realvel" in logs, logs
    assert l1.item() != l0.item() and l1.item() > l0.item()


def test_the_teacher_reads_the_shadow_and_never_writes_the_masters(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", perturb_teacher=False, twinflow_enabled=True, use_ema=True)
    trainer.ema_model.warmup_steps = 1          # the EMA's own decay from its first update on (its default first update has decay 0: a copy of the masters)
    comp = plugin.get_trained_component()
    from simpletuner_amd import twinflow as TW
    masters, shadow = comp.lora_flat.clone(), trainer.ema_model.shadow_flat
    assert torch.equal(shadow, masters)
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    sig = prepared["sigmas"].reshape(-1)

    def teacher():
        with TW.teacher_context(plugin, TW.settings(plugin.config)) as is_ema:
            assert is_ema
            return TW.teacher_forward(plugin, prepared, prepared["noisy_latents"], sig)
    with torch.no_grad():
        student = plugin.model_predict(dict(prepared))["model_prediction"].to(BF16)
    assert torch.equal(teacher(), student)                                   # the shadow equals the masters: the teacher is the student
    assert torch.equal(comp.lora_flat, masters)
    trainer.train_step(dict(batch))                                          # one optimizer step: the masters move, the EMA lags
    assert not torch.equal(comp.lora_flat, masters) and not torch.equal(trainer.ema_model.shadow_flat, comp.lora_flat)
    now = comp.lora_flat.clone()
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 1})
    t = teacher()
    with torch.no_grad():
        s = plugin.model_predict(dict(prepared))["model_prediction"].to(BF16)
    assert not torch.equal(t, s)
    assert torch.equal(comp.lora_flat, now) and all(p.grad is None for p in comp.parameters())          # bit-identical masters, nothing accumulated


def test_ratio_zero_or_missing_negative_embeds_launch_no_pair_forward(monkeypatch, caplog):
    for kw, negative in ((dict(twinflow_enhanced_ratio=0.0), True), ({}, False)):
        plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", negative=negative, twinflow_enabled=True, use_ema=True, **kw)
        calls = _count_forwards(plugin)
        from simpletuner_amd import twinflow as TW
        TW._logged.discard("no_negative")
        with caplog.at_level(logging.INFO, logger="simpletuner_amd.twinflow"):
            trainer.train_step(dict(batch))
        assert calls == [(2, True), (2, False), (2, False)]
        assert ("the target is not enhanced" in caplog.text) == (not negative)
        caplog.clear()
        monkeypatch.undo()


def test_the_student_is_the_teacher_only_under_the_opt_out_flags(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", twinflow_enabled=True, twinflow_allow_no_ema_teacher=True)
    assert trainer.ema_model is None
    o_loss, *_ = oracle_twinflow_step("sd3", plugin.get_trained_component(), cpu, None)
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    from simpletuner_amd import twinflow as TW
    plugin.config.twinflow_allow_no_ema_teacher = False
    with pytest.raises(ValueError) as ei:
        with TW.teacher_context(plugin, TW.settings(plugin.config)):
            pass
    assert str(ei.value) == TW.E_TEACHER_NO_EMA


# ------------------------------------------------------------------------------------------------
# (f) refusals, by exact message
# ------------------------------------------------------------------------------------------------
NB = " is not built on the st355 path; set "
REFUSALS = [
    (dict(twinflow_adversarial_enabled=True), "twinflow_enabled with twinflow_adversarial_enabled (the adversarial and rectify terms need negative-time forwards and a "
     "trained sign embedding)" + NB + "--twinflow_adversarial_enabled=false"),
    (dict(model_type="full"), "twinflow_enabled with model_type=full (under a full fine-tune the time-sign embedding table would be trainable)" + NB + "--model_type=lora"),
    (dict(lora_type="lycoris"), "twinflow_enabled with lora_type=lycoris (the teacher forward packs standard LoRA operands from the EMA shadow)" + NB + "--lora_type=standard"),
    (dict(use_dora=True), "twinflow_enabled with use_dora (the DoRA fold does not take the EMA shadow)" + NB + "--use_dora=false"),
    (dict(lora_dropout=0.1), "twinflow_enabled with lora_dropout=0.1 (the reference aligns the teacher's dropout masks by restoring the RNG state, which has no counterpart "
     "here)" + NB + "--lora_dropout=0"),
    (dict(hip_graph=True), "twinflow_enabled with hip_graph (the two logs are read on the host every step)" + NB + "--hip_graph=false"),
    (dict(tread_config={"routes": [{"selection_ratio": 0.5}]}), "twinflow_enabled with TREAD routing (the teacher forwards of the no-grad route do not route tokens)" + NB
     + "tread_config without routes"),
    (dict(mixflow_enabled=True), "twinflow_enabled with mixflow_enabled (MixFlow interpolates at a slowed time the RCGM integration does not know)" + NB + "--mixflow_enabled=false"),
    (dict(controlnet=True), "twinflow_enabled with controlnet (teacher forwards through controlnet_predict)" + NB + "--controlnet=false"),
    (dict(distillation_method="dmd"), "twinflow_enabled with distillation_method=dmd (a distiller owns the step's loss)" + NB + "--distillation_method=None"),
]


@pytest.mark.parametrize("family", ["sd3", "flux"])
@pytest.mark.parametrize("kw,message", REFUSALS)
def test_sd3_and_flux_refuse_what_is_not_built_by_exact_message(family, kw, message):
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.sd3.model import SD3
    Plug = {"sd3": SD3, "flux": Flux}[family]
    plug = Plug.__new__(Plug)
    plug.config = NS(model_type="lora", twinflow_enabled=True, use_ema=True, **{k: v for k, v in kw.items() if k != "model_type"})
    if "model_type" in kw:
        plug.config.model_type = kw["model_type"]
    with pytest.raises(NotImplementedError) as ei:
        plug.twinflow_value()
    assert str(ei.value) == message
    plug.config = NS(model_type="lora", twinflow_enabled=True, use_ema=True)
    assert plug.twinflow_value() is True
    plug.config = NS(model_type="lora", **kw) if "model_type" not in kw else NS(**kw)
    assert plug.twinflow_value() is False                                    # flag absent: nothing is checked


@pytest.mark.parametrize("cls_path", ["simpletuner_amd.pixart.model.PixartSigma", "simpletuner_amd.sdxl.model.SDXL", "simpletuner_amd.sd1x.model.StableDiffusion1"])
def test_the_epsilon_and_v_families_raise_the_references_error_and_refuse_the_bridge(G, cls_path):
    import importlib
    mod, cls = cls_path.rsplit(".", 1)
    Plug = getattr(importlib.import_module(mod), cls)
    plug = Plug.__new__(Plug)
    plug.config = NS(model_type="lora", twinflow_enabled=True, use_ema=True)
    with pytest.raises(ValueError) as ei:
        plug.twinflow_value()
    assert str(ei.value) == G["config"]["errors"]["not_flow"]["message"]
    plug.config = NS(model_type="lora", twinflow_enabled=True, use_ema=True, diff2flow_enabled=True, twinflow_allow_diff2flow=True)
    with pytest.raises(NotImplementedError) as ei:
        plug.twinflow_value()
    assert str(ei.value) == (f"twinflow_enabled with diff2flow_enabled + twinflow_allow_diff2flow (the diff2flow bridge) is not built for {Plug.NAME} on the st355 path "
                             "(built: SD3, Flux); set --twinflow_enabled=false")


def test_construction_validates_and_the_trainer_refuses_and_the_sign_table_is_checked(monkeypatch, G):
    from simpletuner_amd import twinflow as TW
    from simpletuner_amd.training.trainer import Trainer
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, "sd3", twinflow_enabled=True)                   # no EMA teacher, at construction
    assert str(ei.value) == G["config"]["errors"]["no_ema"]["message"]
    for kw in (dict(twinflow_allow_no_ema_teacher=True), dict(twinflow_require_ema=False), dict(use_ema=True)):
        _plugin(monkeypatch, "sd3", twinflow_enabled=True, **kw)
    plugin = _plugin(monkeypatch, "sd3", twinflow_enabled=True, use_ema=True)
    plugin.add_lora_adapter()
    plugin.config.hip_graph = True
    with pytest.raises(NotImplementedError, match=r"^twinflow_enabled with hip_graph "):
        Trainer(plugin.config, plugin, plugin.accelerator)
    sd = {"a.weight": torch.ones(2), "time_sign_embed.weight": torch.zeros(2, 4)}
    assert set(TW.drop_sign_embedding(sd)) == {"a.weight"} and TW.drop_sign_embedding({"a.weight": sd["a.weight"]}).keys() == {"a.weight"}
    sd["time_sign_embed.weight"][1, 2] = 0.5
    with pytest.raises(NotImplementedError) as ei:
        TW.drop_sign_embedding(sd)
    assert str(ei.value) == ("twinflow_enabled with a checkpoint that carries a non-zero time_sign_embed.weight (a trained time-sign embedding: the adversarial branch's "
                             "product) is not built on the st355 path; set --twinflow_enabled=false or load the base checkpoint")


def test_the_three_existing_combinations_stay_refused_with_their_own_messages():
    from simpletuner_amd.sd3.model import SD3
    plug = SD3.__new__(SD3)
    plug.config = NS(model_type="lora", scheduled_sampling_max_step_offset=2, twinflow_enabled=True, use_ema=True)
    with pytest.raises(NotImplementedError) as ei:
        plug.scheduled_sampling_value()
    assert str(ei.value) == "scheduled_sampling_max_step_offset=2 with twinflow_enabled: TwinFlow is not built on the st355 path"


def test_abi_exports_the_twinflow_symbols():
    """include/st355.h declares, lib.py lists and types, and (when it is built) the library exports the four new entries"""
    from simpletuner_amd import lib
    names = ["st355_twinflow_workspace", "st355_twinflow_rcgm_step", "st355_twinflow_loss", "st355_twinflow_ucgm_step"]
    header = open(os.path.join(ROOT, "include", "st355.h")).read()
    for n in names:
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    assert "twinflow.hip" in open(os.path.join(ROOT, "simpletuner_amd", "csrc", "Makefile")).read()
    if lib.is_built():
        L = lib.load()
        assert all(hasattr(L, n) for n in names)


# ------------------------------------------------------------------------------------------------
# (g) the UCGM sampler
# ------------------------------------------------------------------------------------------------
def test_ucgm_grid_equals_the_executed_scheduler(G):
    from simpletuner_amd import twinflow as TW
    for n, rec in G["sampler"]["grids"].items():
        sig = TW.ucgm_sigmas(n)
        assert sig.dtype == F32 and torch.equal(sig, rec["sigmas"]) and torch.equal(sig[:-1] * 1000.0, rec["timesteps"]), n
    assert abs(float(TW.ucgm_sigmas(2)[1]) - 0.6) < 1e-6 and abs(float(TW.ucgm_sigmas(4)[3]) - 0.5) < 1e-6 and abs(float(TW.ucgm_sigmas(6)[5]) - 0.3) < 1e-6


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_ucgm_step_equals_the_executed_scheduler(G, dt):
    """the fp64 restatement of the step against every recorded chain state (7 roundings per element of magnitude below 16: TOL), then the bf16 stand-in chain of
    ucgm_sample inside its derived bound of the fp64 step"""
    tol = (2.0 ** -53 if dt == "fp64" else 2.0 ** -24) * 7 * 16
    for name, ch in G["sampler"]["chains"].items():
        if not name.startswith(dt + "."):
            continue
        x, sig = ch["x0"].to(F64), ch["sigmas"].to(F64)
        for i in range(ch["steps"]):
            want = TR.ucgm64(ch["states"][i - 1] if i else x, ch["v"][i], float(sig[i]), float(sig[i + 1]), ch["rho"], ch["noise"][i])
            assert float((want - ch["states"][i].to(F64)).abs().max()) <= tol, (name, i)


def test_ucgm_sample_runs_the_grid_through_the_step_op(monkeypatch, G):
    from simpletuner_amd import twinflow as TW
    TR.install(monkeypatch)
    ch = G["sampler"]["chains"]["bf16.steps2.rho1.0"]
    seen = []

    def predict(x, t):
        seen.append(t.clone())
        return ch["v"][len(seen) - 1]
    states = []
    out = TW.ucgm_sample(predict, ch["x0"], 2, 1.0, noises=ch["noise"], on_step=lambda i, x: states.append(x.clone()))
    assert [float(t[0]) for t in seen] == (ch["sigmas"][:-1] * 1000.0).tolist() and out.dtype == BF16
    x = ch["x0"].clone()
    for i in range(2):
        ref, tol = TB.ucgm_step_ref(x, ch["v"][i], float(ch["sigmas"][i]), float(ch["sigmas"][i + 1]), 1.0, ch["noise"][i])
        assert TB.inside(states[i], ref, tol)[0]
        x = states[i]
        print(f"[bf16 record] ucgm step {i}: executed-vs-kernel-contract max |d| {float((states[i].double() - ch['states'][i].double()).abs().max()):.3e}")


def test_sample_images_takes_the_ucgm_sampler_at_guidance_zero(monkeypatch, caplog):
    from simpletuner_amd import sampling
    plugin = _plugin(monkeypatch, "sd3", twinflow_enabled=True, use_ema=True, twinflow_target_step_count=2)
    plugin.add_lora_adapter()
    _, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    calls = _count_forwards(plugin)
    with caplog.at_level(logging.INFO, logger="simpletuner_amd.sampling"):
        x = sampling.sample_images(plugin, devt["prompt"], devt["pooled"], 16, 8, num_inference_steps=20, decode=False, guidance_scale=5.0,
                                   negative_prompt_embeds=torch.zeros_like(devt["prompt"]), generator=torch.Generator().manual_seed(0))
    assert calls == [(2, False), (2, False)] and x.shape == (2, 16, 16, 8) and bool(torch.isfinite(x.float()).all())
    assert "TwinFlow validation: 2 steps, guidance_scale=0.0" in caplog.text


# ------------------------------------------------------------------------------------------------
# (h) flag absent
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_flag_absent_or_off_takes_todays_route_and_imports_nothing(monkeypatch, family):
    from simpletuner_amd import ops
    results = []
    for kw in ({}, dict(twinflow_enabled=False), dict(twinflow_enabled=None)):
        sys.modules.pop("simpletuner_amd.twinflow", None)
        plugin, trainer, batch, cpu = _trainer(monkeypatch, family, use_ema=True, **kw)
        for name in TR.STAND_INS:
            monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a TwinFlow op ran with the flag absent"))
        loss = trainer.train_step(dict(batch))
        assert trainer.last_aux_logs is None and "simpletuner_amd.twinflow" not in sys.modules
        results.append((loss.clone(), plugin.get_trained_component().lora_flat.clone()))
        monkeypatch.undo()
    assert all(torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) for r in results[1:])


TRACE_K = "(test_sd3_host_sequencing_cpu or test_flux_host_sequencing_cpu) and lora_path"


def test_the_launch_trace_with_the_flag_absent_is_todays(tmp_path):
    """tools/launch_trace.py over the Flux and SD3 LoRA host-sequencing tests gives, byte for byte, the file whose digest tests/golden/ has held since before
    scheduled sampling (the same selection and digest tests/test_scheduled_sampling_cpu.py pins)"""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_trace.py"), str(out), "-k", TRACE_K], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = open(os.path.join(ROOT, "tests", "golden", "scheduled_sampling_flag_off_launch_trace.sha256")).read().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want

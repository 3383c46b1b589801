"""Scheduled sampling with ReflexFlow on the CPU: the plan, the probability ramp, the flow rollout and the loss against the EXECUTED reference
(tests/golden/scheduled_sampling_vectors.pt, written by tools/gen_scheduled_sampling_golden.py), the fp64 restatement against autograd, the tiny SD3 and Flux
plugins on the kernel-contract emulator against an oracle step that does the same rollout, the refusals, and the flags-absent route."""
import hashlib
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from oracle import flux as OF
from oracle import sd3 as OS
from tests import parity_utils as PU
from tests import reflexflow_ref as RR
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = SimpleNamespace


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(ROOT, "tests", "golden", "scheduled_sampling_vectors.pt"), weights_only=False)


# ------------------------------------------------------------------------------------------------
# (a) the ramp and the plan: exact
# ------------------------------------------------------------------------------------------------
def test_probability_ramp_equals_the_executed_reference(G):
    from simpletuner_amd.scheduled_sampling import effective_probability
    for si, step, want in G["ramp"]["rows"]:
        cfg = NS(scheduled_sampling_max_step_offset=3, **G["ramp"]["settings"][si])
        assert effective_probability(cfg, step) == want, (G["ramp"]["settings"][si], step)
    quirk = NS(scheduled_sampling_probability=0.3, scheduled_sampling_prob_start=0.0, scheduled_sampling_prob_end=0.9, scheduled_sampling_ramp_steps=10)
    assert effective_probability(quirk, 0) == 0.3          # an explicit prob_start of 0.0 falls back to the plain probability


def test_rollout_schedule_equals_the_executed_reference_draw_for_draw(G):
    from simpletuner_amd.scheduled_sampling import build_rollout_schedule
    for rec in G["plan"]:
        st = rec["settings"]
        torch.manual_seed(st["seed"])
        p = build_rollout_schedule(num_train_timesteps=st["T"], batch_size=st["B"], max_step_offset=st["off"], device="cpu", base_timesteps=rec["base"],
                                   strategy=st["strategy"], apply_probability=st["prob"])
        for got, want in ((p.target_timesteps, rec["target"]), (p.source_timesteps, rec["source"]), (p.rollout_steps, rec["steps"])):
            assert got.dtype == want.dtype == torch.long and torch.equal(got, want), st
        assert torch.equal(p.target_timesteps, rec["base"].long()) and int(p.source_timesteps.max()) <= st["T"] - 1
    with pytest.raises(ValueError, match="scheduled_sampling_strategy .nope. is not built"):
        build_rollout_schedule(num_train_timesteps=10, batch_size=1, max_step_offset=1, device="cpu", base_timesteps=torch.zeros(1), strategy="nope")


# ------------------------------------------------------------------------------------------------
# (b) the rollout over the stub model
# ------------------------------------------------------------------------------------------------
def _stub_predict(batch):
    """the generator's stub (G["stub_model"]): 0.5 * tanh(x) + sin(t / 100) * mean(enc) + 0.1 * flip(x, -1)"""
    x, t, enc = batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"]
    assert x.shape[0] == 1 and t.shape[0] == 1 and enc.shape[0] == 1 and set(batch) == {"noisy_latents", "timesteps", "encoder_hidden_states"}
    return {"model_prediction": (0.5 * torch.tanh(x) + torch.sin(t.float() / 100.0).view(1, 1, 1, 1) * enc.float().mean() + 0.1 * x.flip(-1)).to(x.dtype)}


def _fp32_noise_mix(x, sigma, noise=None, seed=0, offset=0, want_target=True):
    s = sigma.to(F64).view(-1, *([1] * (x.dim() - 1)))
    return ((1 - s) * x.to(F64) + s * noise.to(F64)).to(x.dtype), None, noise


def _fp32_euler(x, v, dt):
    x.copy_(RR.euler64(x, v, dt).to(x.dtype))
    return x


@pytest.mark.parametrize("name", ["table.reflex1", "table.reflex0", "no_table.reflex1", "no_table.reflex0"])
def test_flow_rollout_equals_the_executed_reference(monkeypatch, G, name):
    """the host logic on fp32 tensors, as the reference ran it: the two streaming ops are replaced by fp64-then-fp32 forms of their contract.  Tolerance: at most 3
    Euler steps, each a handful of fp32 roundings of values below 8 through a map of Lipschitz constant about 1: 3 * 8 * 8 * 2^-24 < 2e-5."""
    from simpletuner_amd import ops, scheduled_sampling as SS
    monkeypatch.setattr(ops, "flow_noise_mix", _fp32_noise_mix)
    monkeypatch.setattr(ops, "flow_euler_step", _fp32_euler)
    rec = G["rollout"][name]
    reflex = name.endswith("1")
    batch = {k: v.clone() for k, v in rec["inputs"].items()}
    batch["scheduled_sampling_plan"] = SS.ScheduledSamplingPlan(*rec["plan"])
    sched = NS(config=NS(num_train_timesteps=1000), **({"sigmas": rec["sigmas_table"]} if rec["sigmas_table"] is not None else {}))
    model = NS(model_predict=_stub_predict, ROLLOUT_BATCH_KEYS=("encoder_hidden_states", "not_in_the_batch"), config=NS(scheduled_sampling_reflexflow=reflex))
    out = SS.apply_flow_rollout(model, batch, sched)
    tol = 2e-5
    assert (out["noisy_latents"] - rec["noisy_latents"]).abs().max().item() < tol
    assert torch.equal(out["timesteps"], rec["timesteps"]) and out["timesteps"].dtype == rec["timesteps"].dtype
    assert torch.equal(out["sigmas"], rec["sigmas"])
    tgt, src, steps = rec["plan"]
    alone = [i for i in range(4) if int(steps[i]) <= 0 or int(src[i]) <= int(tgt[i])]
    assert alone == [0]
    for i in range(4):          # which samples were left alone: bit for bit the pre-rollout state and the fractional timestep
        same = torch.equal(out["noisy_latents"][i], rec["inputs"]["noisy_latents"][i])
        assert same == (i in alone) == torch.equal(rec["noisy_latents"][i], rec["inputs"]["noisy_latents"][i])
        assert (out["timesteps"][i] == rec["inputs"]["timesteps"][i]).item() == (i in alone)
    if reflex:
        for k, key in (("clean", "_reflexflow_clean_pred"), ("biased", "_reflexflow_biased_pred")):
            assert (out[key] - rec[k]).abs().max().item() < tol
        assert torch.equal(out["_reflexflow_clean_pred"][0], out["_reflexflow_biased_pred"][0])
        assert torch.equal(out["_reflexflow_pre_rollout_noisy"], rec["inputs"]["noisy_latents"])
    else:
        assert "_reflexflow_clean_pred" not in out and rec["clean"] is None


# ------------------------------------------------------------------------------------------------
# (c) the loss: restatement == executed reference; closed-form gradient == autograd
# ------------------------------------------------------------------------------------------------
def _params(kw):
    """the reference's `or` idiom, as ModelFoundation._reflexflow_loss reads the three options"""
    beta2 = kw.get("beta2", 1.0)
    return dict(alpha=float(kw.get("alpha", 1.0) or 0.0), beta1=float(kw.get("beta1", 10.0) or 0.0), beta2=1.0 if beta2 is None else float(beta2))


def _fixture_mask(G, mask):
    from simpletuner_amd.foundation import ModelFoundation
    I = G["loss"]["inputs"]
    if not mask:
        return None
    return ModelFoundation._conditioning_loss_mask(NS(config=NS()), {"loss_mask_type": "mask", "conditioning_pixel_values": I["conditioning_pixel_values"]}, I["pred"], True)


def test_restatement_equals_the_executed_reference_loss_and_gradient(G):
    """the reference ran in fp32 on [3, 4, 4, 6] tensors: sums of 96 terms, values of order 10 -> 1e-5 relative to the loss; the gradient likewise, relative to its
    largest element"""
    I = G["loss"]["inputs"]
    flat = lambda k: RR._flat(I[k])
    n = 0
    for (lt, mask, cached, pi), rec in G["loss"]["cases"].items():
        kw = _params(rec["params"])
        em = _fixture_mask(G, mask)
        c, b = (I["clean"], I["biased"]) if cached else (None, None)
        r = RR.reflexflow64(I["pred"], I["target"], I["noisy"], I["latents"], c, b, lt, 0.1, em, **kw)
        assert abs(r["loss"].item() - rec["loss"].item()) < 1e-5 * max(1.0, abs(rec["loss"].item())), (lt, mask, cached, rec["params"])
        assert (r["dpred"] - rec["grad"].to(F64)).abs().max().item() < 1e-5 * max(1e-3, rec["grad"].abs().max().item()), (lt, mask, cached, rec["params"])
        p = flat("pred").clone().requires_grad_(True)
        loss, _, _ = RR.loss64(p, flat("target"), flat("noisy"), flat("latents"), None if c is None else flat("clean"), None if b is None else flat("biased"), lt, 0.1, em, **kw)
        loss.backward()
        assert abs(loss.item() - r["loss"].item()) < 1e-12 * max(1.0, abs(loss.item()))
        assert (p.grad.reshape(I["pred"].shape) - r["dpred"]).abs().max().item() < 1e-12 * max(1.0, p.grad.abs().max().item())
        n += 1
    assert n == 96


def test_closed_form_gradient_equals_autograd_with_a_zero_prediction_and_grad_scale():
    g = torch.Generator().manual_seed(2)
    B, N = 3, 64
    rn = lambda: torch.randn(B, N, generator=g, dtype=F64)
    pred, target, noisy, latents, clean, biased = rn(), rn(), rn(), rn(), rn(), rn()
    em = torch.rand(B, 16, generator=g, dtype=F64)
    hc = torch.tensor([0.1, 0.03, 0.5], dtype=F64)
    for lt in ("l2", "huber", "smooth_l1"):
        p = pred.clone().requires_grad_(True)
        loss, per, adr = RR.loss64(p, target, noisy, latents, clean, biased, lt, hc, em, 0.7, 3.0, 0.5)
        (2.5 * loss).backward()
        r = RR.reflexflow64(pred, target, noisy, latents, clean, biased, lt, hc, em, 0.7, 3.0, 0.5, grad_scale=2.5)
        assert (p.grad - r["dpred"]).abs().max().item() < 1e-13 * p.grad.abs().max().item() + 1e-15
        assert torch.allclose(per, r["per_sample"], rtol=1e-13, atol=0) and torch.allclose(adr, r["adr"], rtol=1e-13, atol=0)
    z = pred.clone(); z[1] = 0.0          # a sample with p == 0: the clamped norm; autograd's subgradient there is 0, the closed form's is finite
    r = RR.reflexflow64(z, target, noisy, latents, None, None, "l2", None, None, 1.0, 10.0, 1.0)
    assert bool(torch.isfinite(r["dpred"]).all())
    tau = noisy[1] - latents[1]
    want = 2.0 * (z[1] - target[1]) / (N * B) + 2.0 * 10.0 * (0.0 - tau / tau.norm()) / (B * 1e-6)
    assert torch.allclose(r["dpred"][1], want, rtol=1e-12, atol=0)


def test_stand_ins_follow_the_restatement_and_round_once():
    g = torch.Generator().manual_seed(4)
    rb = lambda *s: torch.randn(*s, generator=g).to(BF16)
    pred, target, noisy, latents, clean, biased = (rb(2, 4, 4, 4) for _ in range(6))
    st = RR.reflexflow_stats(pred, noisy, latents, clean, biased)
    assert st.dtype == F32 and torch.equal(st, RR.stats64(pred, noisy, latents, clean, biased).to(F32))
    loss, per, adr, dpred = RR.reflexflow_loss(pred, target, noisy, latents, st, "huber", 0.1, clean, biased, emask=torch.rand(2, 16, generator=g))
    assert loss.shape == (1,) and per.shape == (2,) and adr.shape == (2,) and dpred.dtype == BF16 and dpred.shape == pred.shape
    assert abs(loss.item() - per.mean().item()) < 1e-6
    x0 = rb(2, 4, 4, 4); x = x0.clone(); v = rb(2, 4, 4, 4); dt = torch.tensor([-0.001, 0.25])
    assert RR.flow_euler_step(x, v, dt) is x
    assert torch.equal(x, (x0.double() + dt.double().view(2, 1, 1, 1) * v.double()).to(BF16))
    with pytest.raises(Exception):
        RR.flow_euler_step(x, x, dt)


# ------------------------------------------------------------------------------------------------
# (d) the plugins on the emulator against the rollout oracle
# ------------------------------------------------------------------------------------------------
def _acc():
    return NS(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
              backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    RR.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=3, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(2))
    return plugin


OFFSETS = (0, 1, 2)


def _plan(sigmas, offsets=OFFSETS):
    from simpletuner_amd.scheduled_sampling import ScheduledSamplingPlan
    base = (sigmas * 1000.0).long()
    off = torch.tensor(offsets[:base.numel()])
    return ScheduledSamplingPlan(target_timesteps=base, source_timesteps=torch.clamp(base + off, max=999), rollout_steps=off)


def _trainer(monkeypatch, family, B=3, seed=3, plan=True, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, family, **cfg_kw)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(B, 8, 8, 24, 128, 64, "cpu", seed=seed)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    if plan:
        batch["scheduled_sampling_plan"] = _plan(devt["sigmas"])
    return plugin, trainer, batch, cpu


def _capture_grads(trainer):
    """the gradients train_step hands to the optimizer (it clears them afterwards)"""
    got = {}
    comp = trainer.model.get_trained_component()
    step = trainer.optimizer.step

    def wrapped(*a, **k):
        got.update({n: p.grad.detach().clone() for n, p in comp.named_parameters() if ".lora_" in n and p.grad is not None})
        return step(*a, **k)
    trainer.optimizer.step = wrapped
    return got


def oracle_rollout_step(family, comp, cpu, plan, loss_type="l2", alpha=1.0, beta1=10.0, beta2=1.0, reflex=True):
    """the same step in plain torch: oracle forwards (fp32) for every rollout forward, states and predictions rounded to bf16 where the engine holds bf16 tensors,
    the loss by tests/reflexflow_ref.loss64 with autograd through the final forward.  Returns (loss, prediction, {target: (dA, dB)}, post-rollout batch tensors)."""
    r16 = lambda t: t.to(BF16).float()
    P, lora, scale = PU.oracle_state(comp)
    if family == "sd3":
        P["pos_embed.pos_embed"] = comp.pos_embed.pos_embed.detach().float().cpu()
        ocfg = SH._ocfg(comp)
        fwd = lambda lp, x, sl, t: OS.sd3_forward(P, ocfg, x, cpu["prompt"][sl], cpu["pooled"][sl], t, lora=lp, lora_scale=scale)
    else:
        ocfg = PU.oracle_cfg(comp)
        fwd = lambda lp, x, sl, t: OF.flux_model_predict(P, ocfg, x, cpu["prompt"][sl], cpu["pooled"][sl], t, 1.0, lora=lp, lora_scale=scale)
    x, n, sig = cpu["latents"], cpu["noise"], cpu["sigmas"]
    B = x.shape[0]
    s4 = sig.view(B, 1, 1, 1)
    noisy, target, t = r16((1 - s4) * x + s4 * n), r16(n - x), sig * 1000.0
    clean, biased = torch.zeros_like(x), torch.zeros_like(x)
    new_noisy, new_t = noisy.clone(), t.clone()
    steps, src, tgt = (v.tolist() for v in (plan.rollout_steps, plan.source_timesteps, plan.target_timesteps))
    with torch.no_grad():
        for i in range(B):
            sl = slice(i, i + 1)
            if reflex:
                clean[sl] = r16(fwd(lora, noisy[sl], sl, t[sl]))
            if steps[i] <= 0 or src[i] <= tgt[i]:
                biased[sl] = clean[sl]
                continue
            f = torch.tensor(src[i] / 999.0, dtype=F32)
            cur = r16((1 - f) * x[sl] + f * n[sl])
            frac = src[i] / 999.0
            for tt in range(src[i], tgt[i], -1):
                nxt = max(tgt[i], tt - 1) / 999.0
                pred = r16(fwd(lora, cur, sl, torch.tensor([float(tt)])))
                cur = r16(cur + torch.tensor(nxt - frac, dtype=F32) * pred)
                frac = nxt
            if reflex:
                biased[sl] = r16(fwd(lora, cur, sl, torch.tensor([float(tgt[i])])))
            new_noisy[sl], new_t[i] = cur, float(tgt[i])
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    pred = fwd(lp, new_noisy, slice(0, B), new_t)
    fl = lambda v: v.double().reshape(B, -1)
    if reflex:
        loss, _, adr = RR.loss64(fl(pred), fl(target), fl(new_noisy), fl(x), fl(clean), fl(biased), loss_type, 0.1, None, alpha, beta1, beta2)
    else:
        loss, adr = RR.element_loss(fl(pred) - fl(target), loss_type, RR._huber(0.1, B)).mean(1).mean(), None
    loss.backward()
    return loss.detach(), pred.detach(), {k: (a.grad, b.grad) for k, (a, b) in lp.items()}, dict(noisy=new_noisy, t=new_t, clean=clean, biased=biased, adr=adr)


def _compare_grads(got, ref, tol=5e-2):
    worst = 0.0
    assert got
    for name, g in got.items():
        key, which = name.split(".lora_")
        want = ref[key][0 if which.startswith("A") else 1]
        worst = max(worst, PU.rel_l2(g, want))
        assert PU.rel_l2(g, want) < tol, (name, PU.rel_l2(g, want))
    return worst


@pytest.mark.parametrize("loss_type", ["l2", "huber"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_train_step_with_an_injected_plan_matches_the_rollout_oracle(monkeypatch, family, loss_type):
    """B = 3, offsets (0, 1, 2), a positive scheduled_sampling_max_step_offset alone (ReflexFlow comes on by the default rule).  The tolerances are those of the
    families' host-sequencing tests: prediction rel-L2 2e-2, loss 2e-3 * max(1, loss), adapter gradients rel-L2 5e-2.  FAILS WITHOUT THE FEATURE: a step that
    ignores the flags returns the un-rolled loss without the ADR term (checked at the end: that loss is far outside the tolerance)."""
    plugin, trainer, batch, cpu = _trainer(monkeypatch, family, scheduled_sampling_max_step_offset=2, loss_type=loss_type)
    assert plugin.config.scheduled_sampling_reflexflow is True
    comp = plugin.get_trained_component()
    plan = batch["scheduled_sampling_plan"]
    o_loss, o_pred, o_grads, o_post = oracle_rollout_step(family, comp, cpu, plan, loss_type)
    seen = {}
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: seen.setdefault("last", predict(pb)) if pb["noisy_latents"].shape[0] == 3 else predict(pb)
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    pred = seen["last"]["model_prediction"].detach()
    assert PU.rel_l2(pred, o_pred) < 2e-2
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item()), (loss.item(), o_loss.item())
    worst = _compare_grads(grads, o_grads)
    logs = trainer.last_aux_logs
    assert abs(logs["reflexflow_adr"] - o_post["adr"].mean().item()) < 2e-3 * max(1.0, o_post["adr"].mean().item()) and 0.0 < logs["reflexflow_weight_deviation"] < 1.0
    # the un-rolled, un-weighted loss of a step that ignores the flags
    plain = ((o_pred - (cpu["noise"] - cpu["latents"]).to(BF16).float()) ** 2).mean().item()
    assert abs(loss.item() - plain) > 10 * 2e-3 * max(1.0, o_loss.item())
    print(f"[emu] {family} {loss_type}: loss {loss.item():.5f} vs oracle {o_loss.item():.5f} (plain {plain:.5f}), worst adapter gradient rel-L2 {worst:.3e}, logs {logs}")


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_rollout_without_reflexflow_rolls_and_keeps_todays_loss(monkeypatch, family):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, family, scheduled_sampling_max_step_offset=2, scheduled_sampling_reflexflow=False)
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "reflexflow_loss", lambda *a, **k: pytest.fail("the ReflexFlow loss must not run with the flag off"))
    o_loss, _, o_grads, _ = oracle_rollout_step(family, plugin.get_trained_component(), cpu, batch["scheduled_sampling_plan"], reflex=False)
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    _compare_grads(grads, o_grads)
    assert trainer.last_aux_logs is None


def test_the_flag_alone_adds_the_adr_term_without_a_plan(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", plan=False, scheduled_sampling_reflexflow=True)
    plan0 = _plan(cpu["sigmas"], (0, 0, 0))
    o_loss, _, o_grads, post = oracle_rollout_step("sd3", plugin.get_trained_component(), cpu, plan0, reflex=True)
    # no plan: no cached predictions, so no exposure weight (e == 0 in the oracle above gives weight 1 as well)
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    _compare_grads(grads, o_grads)
    assert set(trainer.last_aux_logs) == {"reflexflow_adr"}


def test_prepare_batch_attaches_a_plan_after_the_noisy_latents_and_the_rollout_touches_no_step_state(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", plan=False, scheduled_sampling_max_step_offset=3, scheduled_sampling_probability=1.0, layersync_enabled=True,
                                           layersync_student_block=1, layersync_teacher_block=2)
    torch.manual_seed(0)
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    plan = prepared["scheduled_sampling_plan"]
    assert torch.equal(plan.target_timesteps, prepared["timesteps"].long()) and int(plan.rollout_steps.max()) <= 3 and "noisy_latents" in prepared
    comp = plugin.get_trained_component()
    before = {n: p.detach().clone() for n, p in comp.named_parameters()}
    target = prepared["flow_target"].clone()
    calls = []
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: calls.append((tuple(pb["noisy_latents"].shape), torch.is_grad_enabled(), sorted(pb))) or predict(pb)
    out = plugin.apply_scheduled_sampling_rollout(prepared)
    rolled = [i for i in range(3) if int(plan.rollout_steps[i]) > 0 and int(plan.source_timesteps[i]) > int(plan.target_timesteps[i])]
    want_calls = 3 + sum(int(plan.source_timesteps[i] - plan.target_timesteps[i]) + 1 for i in rolled)
    assert len(calls) == want_calls and all(s[0] == 1 and not g for s, g, _ in calls)
    assert all(keys == ["add_text_embeds", "encoder_hidden_states", "noisy_latents", "timesteps"] for _, _, keys in calls)
    assert torch.equal(out["flow_target"], target)
    assert all(p.grad is None for p in comp.parameters()) and all(torch.equal(p.detach(), before[n]) for n, p in comp.named_parameters())
    for i in rolled:
        assert float(out["timesteps"][i]) == float(plan.target_timesteps[i])


# ------------------------------------------------------------------------------------------------
# (e) refusals, by name
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,flag", [(dict(scheduled_sampling_max_step_offset=2), "scheduled_sampling_max_step_offset=2"),
                                        (dict(scheduled_sampling_reflexflow=True), "scheduled_sampling_reflexflow")])
@pytest.mark.parametrize("cls_path", ["simpletuner_amd.pixart.model.PixartSigma", "simpletuner_amd.sdxl.model.SDXL", "simpletuner_amd.sd1x.model.StableDiffusion1"])
def test_families_without_the_rollout_refuse_both_flags_by_name(cls_path, flags, flag):
    import importlib
    mod, cls = cls_path.rsplit(".", 1)
    Plug = getattr(importlib.import_module(mod), cls)
    plug = Plug.__new__(Plug)
    plug.config = NS(model_type="lora", **flags)
    with pytest.raises(NotImplementedError) as ei:
        plug.scheduled_sampling_value()
    assert str(ei.value).startswith(f"{flag}: scheduled sampling is not built for {Plug.NAME} on the st355 path (built: Flux, SD3)")
    assert getattr(plug.config, "scheduled_sampling_reflexflow", None) is flags.get("scheduled_sampling_reflexflow")          # the default-on rule did not fire
    for cfg in (NS(), NS(scheduled_sampling_max_step_offset=0), NS(scheduled_sampling_max_step_offset=None, scheduled_sampling_reflexflow=False)):
        plug.config = cfg
        assert plug.scheduled_sampling_value() == (0, False)


@pytest.mark.parametrize("family", ["sd3", "flux"])
@pytest.mark.parametrize("flags", [dict(scheduled_sampling_max_step_offset=2), dict(scheduled_sampling_reflexflow=True)])
@pytest.mark.parametrize("kw,pat", [(dict(hip_graph=True), "with hip_graph"), (dict(tread_config={"routes": [{"selection_ratio": 0.5, "start_layer_idx": 0, "end_layer_idx": 1}]}), "with TREAD routing"),
                                    (dict(lora_dropout=0.1), r"with lora_dropout=0\.1"), (dict(twinflow_enabled=True), "with twinflow_enabled"), (dict(controlnet=True), "with controlnet")])
def test_flux_and_sd3_refuse_the_combinations_that_are_not_built(family, flags, kw, pat):
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.sd3.model import SD3
    Plug = {"sd3": SD3, "flux": Flux}[family]
    plug = Plug.__new__(Plug)
    plug.config = NS(model_type="lora", **flags, **kw)
    name = "scheduled_sampling_max_step_offset=2" if "scheduled_sampling_max_step_offset" in flags else "scheduled_sampling_reflexflow"
    with pytest.raises(NotImplementedError, match="^" + name + " " + pat):
        plug.scheduled_sampling_value()
    plug.config = NS(model_type="lora", **flags)
    assert plug.scheduled_sampling_value() == (flags.get("scheduled_sampling_max_step_offset", 0), True)


def test_the_flag_alone_refuses_tokenwise_timesteps_in_prepare_batch_and_in_loss(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", plan=False, scheduled_sampling_reflexflow=True)
    sig = cpu["sigmas"]
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})          # per-sample timesteps: taken
    pred = {"model_prediction": torch.zeros_like(prepared["latents"])}
    prepared["timesteps"] = prepared["timesteps"][:, None].expand(-1, 16).contiguous()
    with pytest.raises(NotImplementedError, match="scheduled_sampling_reflexflow with tokenwise timesteps"):
        plugin.loss(prepared, pred)
    plugin.sample_flow_sigmas = lambda batch, state: (sig, (sig * 1000.0)[:, None].expand(-1, 16).contiguous())
    with pytest.raises(NotImplementedError, match="scheduled_sampling_reflexflow with tokenwise timesteps"):
        plugin.prepare_batch(dict(batch), {"global_step": 0})


def test_lycoris_and_a_full_fine_tune_ignore_lora_dropout_and_tread_config_may_be_an_object():
    from simpletuner_amd.sd3.model import SD3
    plug = SD3.__new__(SD3)
    for kw in (dict(model_type="lora", lora_type="lycoris"), dict(model_type="full")):          # as lora_dropout_value: no dropout would run
        plug.config = NS(scheduled_sampling_max_step_offset=2, lora_dropout=0.1, **kw)
        assert plug.scheduled_sampling_value() == (2, True)
    plug.config = NS(model_type="lora", lora_type="standard", scheduled_sampling_max_step_offset=2, lora_dropout=0.1)
    with pytest.raises(NotImplementedError, match=r"with lora_dropout=0\.1"):
        plug.scheduled_sampling_value()
    plug.config = NS(model_type="lora", scheduled_sampling_max_step_offset=2, tread_config=NS(routes=[{"selection_ratio": 0.5}]))
    with pytest.raises(NotImplementedError, match="with TREAD routing"):
        plug.scheduled_sampling_value()
    plug.config = NS(model_type="lora", scheduled_sampling_max_step_offset=2, tread_config=NS(routes=None))
    assert plug.scheduled_sampling_value() == (2, True)


def test_logs_travel_through_loss_with_logs_and_nothing_is_parked_on_the_plugin(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", scheduled_sampling_max_step_offset=2)
    prepared = plugin.apply_scheduled_sampling_rollout(plugin.prepare_batch(dict(batch), {"global_step": 0}))
    pred = plugin.model_predict(prepared)
    attrs = set(vars(plugin))
    loss = plugin.loss(prepared, pred)                      # loss() alone: a scalar, no logs, no state left behind
    loss2, logs = plugin.loss_with_logs(prepared, pred)
    assert set(vars(plugin)) == attrs and torch.equal(loss.detach(), loss2.detach())
    assert set(logs) == {"reflexflow_adr", "reflexflow_weight_deviation"} and all(isinstance(v, float) for v in logs.values())


def test_the_trainer_refuses_at_construction_and_tokenwise_timesteps_refuse_at_the_plan(monkeypatch):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, "sd3", scheduled_sampling_max_step_offset=2, hip_graph=True)
    plugin.add_lora_adapter()
    with pytest.raises(NotImplementedError, match="scheduled_sampling_max_step_offset=2 with hip_graph"):
        Trainer(plugin.config, plugin, plugin.accelerator)
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", plan=False, scheduled_sampling_max_step_offset=2)
    sig = cpu["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, (sig * 1000.0)[:, None].expand(-1, 16).contiguous())
    with pytest.raises(NotImplementedError, match="scheduled_sampling_max_step_offset / scheduled_sampling_reflexflow with tokenwise timesteps"):
        plugin.prepare_batch(dict(batch), {"global_step": 0})
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    with pytest.raises(RuntimeError, match="scheduled_sampling_max_step_offset: the batch carries a scheduled_sampling_plan but the rollout has not run"):
        plugin.model_predict(prepared)          # a step loop that skips the rollout is refused, not trained on silently
    xm = _plugin(monkeypatch, "sd3", scheduled_sampling_max_step_offset=2, xm_enabled=True, xm_candidate_count=2)
    if getattr(xm.xm_config, "enabled", False):          # XM stays refused where it already is (xm.py)
        with pytest.raises(ValueError, match="not compatible with scheduled sampling"):
            xm._validate_xm_support()


# ------------------------------------------------------------------------------------------------
# (f) flags absent
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_flags_absent_or_off_take_todays_route_bit_for_bit(monkeypatch, family):
    from simpletuner_amd import ops
    results = []
    for kw in ({}, dict(scheduled_sampling_max_step_offset=0, scheduled_sampling_reflexflow=False), dict(scheduled_sampling_max_step_offset=None, scheduled_sampling_reflexflow=None)):
        plugin, trainer, batch, cpu = _trainer(monkeypatch, family, plan=False, **kw)
        for name in ("reflexflow_stats", "reflexflow_loss", "flow_euler_step"):
            monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a ReflexFlow op ran with the flags absent"))
        seen = {}
        mse = ops.mse_loss
        monkeypatch.setattr(ops, "mse_loss", lambda *a, **k: seen.setdefault("mse", mse(*a, **k)))
        loss = trainer.train_step(dict(batch))
        assert trainer.last_aux_logs is None
        assert torch.equal(loss.reshape(()), seen["mse"][0].reshape(()))          # the parent's route: ops.mse_loss through _MSELossFn, nothing after it
        results.append((loss.clone(), plugin.get_trained_component().lora_flat.clone()))
        monkeypatch.undo()
    assert all(torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) for r in results[1:])


TRACE_K = "(test_sd3_host_sequencing_cpu or test_flux_host_sequencing_cpu) and lora_path"


def test_the_launch_trace_with_the_flags_absent_is_the_one_recorded_before_the_feature(tmp_path):
    """tools/launch_trace.py over the Flux and SD3 LoRA host-sequencing tests; the digest under tests/golden/ was recorded on the commit before scheduled sampling"""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_trace.py"), str(out), "-k", TRACE_K], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = open(os.path.join(ROOT, "tests", "golden", "scheduled_sampling_flag_off_launch_trace.sha256")).read().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want


# ------------------------------------------------------------------------------------------------
# (g) gradient accumulation
# ------------------------------------------------------------------------------------------------
def test_gradient_accumulation_of_two_adds_two_rolled_micro_steps(monkeypatch):
    singles = []
    for seed in (3, 4):
        plugin, trainer, batch, cpu = _trainer(monkeypatch, "sd3", seed=seed, scheduled_sampling_max_step_offset=2)
        g = _capture_grads(trainer)
        trainer.train_step(dict(batch))
        singles.append(g)
        monkeypatch.undo()
    plugin, trainer, b1, _ = _trainer(monkeypatch, "sd3", seed=3, scheduled_sampling_max_step_offset=2, gradient_accumulation_steps=2)
    _, devt = PU.make_inputs(3, 8, 8, 24, 128, 64, "cpu", seed=4)
    b2 = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"], "scheduled_sampling_plan": _plan(devt["sigmas"])}
    sigs = iter([PU.make_inputs(3, 8, 8, 24, 128, 64, "cpu", seed=3)[1]["sigmas"], devt["sigmas"]])
    plugin.sample_flow_sigmas = lambda batch, state: (lambda s: (s, s * 1000.0))(next(sigs))
    got = _capture_grads(trainer)
    trainer.train_step(dict(b1))
    assert not got and trainer.state["global_step"] == 0
    trainer.train_step(dict(b2))
    assert got and trainer.state["global_step"] == 1
    for n, g in got.items():
        assert PU.rel_l2(g, 0.5 * (singles[0][n] + singles[1][n])) < 5e-2, n

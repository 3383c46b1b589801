"""Scheduled sampling with ReflexFlow on the MI355X: the three kernels of simpletuner_amd/csrc/reflexflow.hip element-wise inside the derived bounds of
tests/reflexflow_bounds.py (fp64 on the same operands) and bit-identical run to run, the stand-ins of tests/reflexflow_ref.py op by op inside the same bounds, the
rollout on the device against a loop written here, and the tiny SD3 / Flux steps against the rollout oracle of tests/test_scheduled_sampling_cpu.py."""
from types import SimpleNamespace

import pytest
import torch

from simpletuner_amd import lib as _lib
from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from tests import parity_utils as PU
from tests import reflexflow_bounds as RB
from tests import reflexflow_ref as RR
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_scheduled_sampling_cpu import OFFSETS, _capture_grads, _compare_grads, _plan, oracle_rollout_step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
SHAPES = [8, 64, 128, 960, 30720]          # one vector | one partial workgroup | the smallest masked size | a ragged tail | several first-stage partials per sample


def _guarded(t, sentinel=-7.0):
    """a contiguous copy of t at the head of a larger buffer whose tail holds a sentinel: (tensor, tail)"""
    buf = torch.full((t.numel() + GUARD,), sentinel, dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape), buf[t.numel():]


def _operands(B, N, seed, e_zero=False, p_zero=None):
    g = torch.Generator().manual_seed(seed)
    rb = lambda: torch.randn(B, N, generator=g).to(BF16)
    d = SimpleNamespace(pred=rb(), target=rb(), noisy=rb(), latents=rb(), clean=rb(), biased=rb())
    if e_zero:
        d.biased = d.clean.clone()
    if p_zero is not None:
        d.pred[p_zero] = 0.0
    d.huber_c = torch.tensor([0.1, 0.03, 0.5])[:B].contiguous()
    d.emask = torch.rand(B, N // 16, generator=g) if (N // 16) % 8 == 0 and N % 16 == 0 else None
    return d


def _variants(B, N):
    base = dict(cached=True, alpha=1.0, beta1=10.0, beta2=1.0, want_grad=True, grad_scale=1.0, mask=False, e_zero=False, p_zero=None)
    out = [dict(base), dict(base, cached=False), dict(base, e_zero=True), dict(base, p_zero=B // 2), dict(base, alpha=0.0), dict(base, beta1=0.0), dict(base, beta2=0.0),
           dict(base, want_grad=False), dict(base, grad_scale=0.5), dict(base, alpha=0.5, beta1=2.0, beta2=0.25, grad_scale=3.0)]
    if (N // 16) % 8 == 0 and N % 16 == 0:
        out += [dict(base, mask=True), dict(base, mask=True, cached=False, beta1=0.0)]
    return out


def run_loss(fns, d, v, loss_type, dev):
    to = lambda t: None if t is None else t.to(dev)
    c, b = (to(d.clean), to(d.biased)) if v["cached"] else (None, None)
    stats = fns.reflexflow_stats(to(d.pred), to(d.noisy), to(d.latents), c, b)
    out = fns.reflexflow_loss(to(d.pred), to(d.target), to(d.noisy), to(d.latents), stats, loss_type, to(d.huber_c), clean=c, biased=b, alpha=v["alpha"], beta1=v["beta1"],
                              beta2=v["beta2"], want_grad=v["want_grad"], grad_scale=v["grad_scale"], emask=to(d.emask) if v["mask"] else None)
    return stats, out


def check_loss(fns, d, v, loss_type, dev, tag):
    c, b = (d.clean, d.biased) if v["cached"] else (None, None)
    assert RB.check_inputs(d.pred, d.noisy, d.latents, c, b), "the bounds assume norms and sum |e| that are 0 or >= 1e-2"
    stats, (loss, per, adr, dpred) = run_loss(fns, d, v, loss_type, dev)
    ref_s, tol_s = RB.stats_ref(d.pred, d.noisy, d.latents, c, b)
    ok, worst = RB.inside(stats, ref_s, tol_s)
    assert ok, (tag, "stats", worst)
    ref = RB.loss_ref(d.pred, d.target, d.noisy, d.latents, stats, c, b, loss_type, d.huber_c, d.emask if v["mask"] else None, v["alpha"], v["beta1"], v["beta2"], v["grad_scale"])
    worsts = {"stats": worst}
    for name, got in (("loss", loss), ("per_sample", per), ("adr", adr), ("dpred", dpred)):
        if got is None:
            assert name == "dpred" and not v["want_grad"]
            continue
        ok, worsts[name] = RB.inside(got, *ref[name])
        assert ok, (tag, name, worsts[name])
    if dpred is not None:
        assert bool(torch.isfinite(dpred).all())
    if v["beta1"] == 0.0:
        assert bool((adr == 0).all())
    if v["e_zero"] or not v["cached"]:
        assert bool((stats[:, 0] == 0).all())
    return stats, (loss, per, adr, dpred), worsts


@pytest.mark.parametrize("loss_type", ["l2", "huber", "smooth_l1"])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_stats_and_loss_are_inside_the_derived_bounds_and_repeat_bit_for_bit(B, N, loss_type):
    worst_all = {}
    for vi, v in enumerate(_variants(B, N)):
        d = _operands(B, N, seed=100 * B + vi, e_zero=v["e_zero"], p_zero=v["p_zero"])
        tag = (B, N, loss_type, vi)
        s1, o1, worsts = check_loss(ops, d, v, loss_type, DEV, tag)
        s2, o2 = run_loss(ops, d, v, loss_type, DEV)
        assert torch.equal(s1, s2) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(o1, o2)), tag
        check_loss(SimpleNamespace(**RR.STAND_INS), d, v, loss_type, torch.device("cpu"), tag + ("stand-in",))          # the stand-ins, inside the same bounds
        for k, w in worsts.items():
            worst_all[k] = max(worst_all.get(k, 0.0), w)
    print(f"[reflexflow B={B} N={N} {loss_type}] worst error / bound: " + ", ".join(f"{k} {w:.3f}" for k, w in worst_all.items()))


@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_euler_step_is_inside_the_derived_bounds_repeats_and_writes_nothing_else(B, N):
    g = torch.Generator().manual_seed(7 * B + N)
    x0, v = torch.randn(B, N, generator=g).to(BF16), torch.randn(B, N, generator=g).to(BF16)
    dt = torch.tensor([-1.0 / 999.0, 0.37, -0.0625])[:B].contiguous()
    ref, tol = RB.euler_ref(x0, v, dt)
    outs = []
    for _ in range(2):
        x, tail = _guarded(x0)
        assert ops.flow_euler_step(x, v.to(DEV), dt.to(DEV)) is x
        ok, worst = RB.inside(x, ref, tol)
        assert ok, worst
        assert bool((tail.float() == -7.0).all()), "guard elements written"
        outs.append(x.clone())
    assert torch.equal(outs[0], outs[1])
    xs = x0.clone()
    RR.flow_euler_step(xs, v, dt)
    assert RB.inside(xs, ref, tol)[0]
    print(f"[flow_euler_step B={B} N={N}] worst error / bound = {worst:.3f}")


def test_input_guard_elements_and_bad_arguments():
    d = _operands(3, 960, seed=1)
    to = lambda t: t.to(DEV)
    stats = ops.reflexflow_stats(to(d.pred), to(d.noisy), to(d.latents), to(d.clean), to(d.biased))
    pred, tail = _guarded(d.pred)
    loss, per, adr, dpred = ops.reflexflow_loss(pred, to(d.target), to(d.noisy), to(d.latents), stats, "l2", clean=to(d.clean), biased=to(d.biased))
    assert bool((tail.float() == -7.0).all()) and dpred.shape == pred.shape
    with pytest.raises(St355Error):          # N % 8 != 0
        ops.reflexflow_stats(to(d.pred)[:, :7], to(d.noisy)[:, :7], to(d.latents)[:, :7])
    with pytest.raises(St355Error):          # clean without biased
        ops.reflexflow_stats(to(d.pred), to(d.noisy), to(d.latents), to(d.clean), None)
    with pytest.raises(St355Error):          # a mask period (60) that is no multiple of 8: N / 16 of this shape is not a period the contract takes
        ops.reflexflow_loss(to(d.pred), to(d.target), to(d.noisy), to(d.latents), stats, "l2", emask=torch.rand(3, 60, device=DEV))
    with pytest.raises(St355Error):          # x and v the same buffer
        ops.flow_euler_step(pred, pred, torch.zeros(3, device=DEV))
    L = _lib.load()
    ws = torch.empty(L.st355_reflexflow_workspace(3, 960), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert L.st355_reflexflow_loss(s, pred.data_ptr(), to(d.target).data_ptr(), None, 1, None, 0, None, None, None, None, None, 0.0, 0.0, 1.0, loss.data_ptr(), per.data_ptr(),
                                   None, None, ws.data_ptr(), 3, 960, 1.0) != 0          # huber without huber_c: refused through ST_REQUIRE
    assert L.st355_reflexflow_loss(s, pred.data_ptr(), to(d.target).data_ptr(), None, 0, None, 0, None, None, None, None, None, 0.0, 10.0, 1.0, loss.data_ptr(), per.data_ptr(),
                                   None, None, ws.data_ptr(), 3, 960, 1.0) != 0          # beta1 != 0 without noisy / latents / stats


# ------------------------------------------------------------------------------------------------
# the plugins on the device
# ------------------------------------------------------------------------------------------------
def _gpu_trainer(family, plan=True, **cfg_kw):
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family=family, lora_rank=8, seed=5, lora_init_b_std=0.02, learning_rate=1e-3, train_batch_size=3, **cfg_kw)
    acc = St355Accelerator(DEV)
    if family == "flux":
        from simpletuner_amd.flux.model import Flux
        plugin = Flux(cfg, acc)
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, acc)
        plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(3, 8, 8, 24, 128, 64, DEV, seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    if plan:
        batch["scheduled_sampling_plan"] = _plan(cpu["sigmas"])
    return plugin, trainer, batch, cpu


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_the_rollout_on_the_device_equals_the_loop_written_here_bit_for_bit(monkeypatch, family):
    """same launches, same order: the clean forward, flow_noise_mix at the source, one model_predict + flow_euler_step per integer timestep, the biased forward.
    Nothing of the step's state moves: parameters, buffers, gradients, the gradient arena, the noise counters, LayerSync's tap.  The tap's buffers (G, cos, sim) belong
    to a LayerSyncTap object that a SAVING forward creates in its context — none persists on the component — so "no tap buffer changed" is checked as: the rollout
    constructs no tap and calls none.  There is no dropout counter to compare: `lora_dropout > 0` is refused with scheduled sampling, so the component has no
    LoraDropout (asserted)."""
    from simpletuner_amd import engine
    plugin, trainer, batch, cpu = _gpu_trainer(family, scheduled_sampling_max_step_offset=2, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=2)
    comp = plugin.get_trained_component()
    assert comp._layersync is not None and getattr(comp, "lora_dropout", None) is None
    taps = []
    tap_init, tap_tap = engine.LayerSyncTap.__init__, engine.LayerSyncTap.tap
    monkeypatch.setattr(engine.LayerSyncTap, "__init__", lambda self, *a: (taps.append("init"), tap_init(self, *a))[1])
    monkeypatch.setattr(engine.LayerSyncTap, "tap", lambda self, *a: (taps.append("tap"), tap_tap(self, *a))[1])
    buffers = {n: b.detach().clone() for n, b in comp.named_buffers()}
    held = {k: v.clone() for k, v in vars(comp).items() if torch.is_tensor(v)}          # every tensor the component holds as a plain attribute (arenas, scratch views)
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    keep = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in prepared.items()}
    before = {n: p.detach().clone() for n, p in comp.named_parameters()}
    arena = comp.lora_grad_flat.clone()
    counters = (plugin._noise_step, plugin._noise_offset)
    out = plugin.apply_scheduled_sampling_rollout(prepared)
    assert (plugin._noise_step, plugin._noise_offset) == counters and torch.equal(comp.lora_grad_flat, arena)
    assert all(p.grad is None for p in comp.parameters()) and all(torch.equal(p.detach(), before[n]) for n, p in comp.named_parameters())
    assert torch.equal(out["flow_target"], keep["flow_target"]) and torch.equal(out["latents"], keep["latents"])
    assert taps == [], taps
    assert all(torch.equal(b, buffers[n]) for n, b in comp.named_buffers()) and all(torch.equal(getattr(comp, k), v) for k, v in held.items())
    # (the taps do work on a saving forward of this component: the check above is not vacuous)
    plugin.model_predict({k: v for k, v in keep.items() if k != "scheduled_sampling_plan"})
    assert taps.count("init") == 1 and taps.count("tap") >= 2
    taps.clear()
    # the loop
    plan = batch["scheduled_sampling_plan"]
    noisy, t = keep["noisy_latents"].clone(), keep["timesteps"].clone()
    clean, biased = torch.zeros_like(noisy), torch.zeros_like(noisy)

    def predict(x, i, ts):
        mini = {k: keep[k][i:i + 1] for k in plugin.ROLLOUT_BATCH_KEYS if torch.is_tensor(keep.get(k))}
        mini["noisy_latents"], mini["timesteps"] = x, ts
        with torch.no_grad():
            res = plugin.model_predict(mini)
        assert "layersync_similarity" not in res          # the no-grad route taps nothing
        return res["model_prediction"].contiguous()
    for i, off in enumerate(OFFSETS):
        tgt, src = int(plan.target_timesteps[i]), int(plan.source_timesteps[i])
        clean[i:i + 1] = predict(keep["noisy_latents"][i:i + 1], i, keep["timesteps"][i:i + 1])
        if off == 0:
            biased[i:i + 1] = clean[i:i + 1]
            continue
        cur = ops.flow_noise_mix(keep["latents"][i:i + 1], torch.tensor([src / 999.0], dtype=F32, device=DEV), noise=keep["input_noise"][i:i + 1], want_target=False)[0]
        frac = src / 999.0
        for tt in range(src, tgt, -1):
            nxt = max(tgt, tt - 1) / 999.0
            ops.flow_euler_step(cur, predict(cur, i, torch.tensor([float(tt)], device=DEV)), torch.tensor([nxt - frac], dtype=F32, device=DEV))
            frac = nxt
        biased[i:i + 1] = predict(cur, i, torch.tensor([float(tgt)], device=DEV))
        noisy[i:i + 1], t[i] = cur, float(tgt)
    assert torch.equal(out["noisy_latents"], noisy) and torch.equal(out["timesteps"], t)
    assert torch.equal(out["_reflexflow_clean_pred"], clean) and torch.equal(out["_reflexflow_biased_pred"], biased)
    assert torch.equal(out["noisy_latents"][0], keep["noisy_latents"][0]) and not torch.equal(out["noisy_latents"][2], keep["noisy_latents"][2])


@pytest.mark.parametrize("loss_type", ["l2", "smooth_l1"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_the_tiny_step_with_the_feature_on_matches_the_rollout_oracle(family, loss_type):
    """tolerances of the tiny-step GPU tests (tests/test_sd3_model_gpu.py, tests/test_flux_model_gpu.py): prediction rel-L2 <= 2e-2, loss |delta| <= 1e-3 max(1, |loss|),
    adapter gradients rel-L2 <= 5e-2 per matrix"""
    plugin, trainer, batch, cpu = _gpu_trainer(family, scheduled_sampling_max_step_offset=2, loss_type=loss_type)
    comp = plugin.get_trained_component()
    o_loss, o_pred, o_grads, o_post = oracle_rollout_step(family, comp, cpu, batch["scheduled_sampling_plan"], loss_type)
    seen = {}
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: seen.setdefault("last", predict(pb)) if pb["noisy_latents"].shape[0] == 3 else predict(pb)
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    torch.cuda.synchronize()
    r = PU.rel_l2(seen["last"]["model_prediction"].detach(), o_pred)
    print(f"[scheduled sampling] {family} {loss_type}: pred rel_l2={r:.3e} loss hip={loss.item():.6f} oracle={o_loss.item():.6f} logs={trainer.last_aux_logs}")
    assert r < 2e-2 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))
    _compare_grads({k: v.cpu() for k, v in grads.items()}, o_grads, 5e-2)
    assert abs(trainer.last_aux_logs["reflexflow_adr"] - o_post["adr"].mean().item()) < 1e-3 * max(1.0, o_post["adr"].mean().item())


def test_the_terms_compose_with_layersync():
    """the same SD3 step with and without LayerSync: the rollout (no-grad forwards, never tapped) leaves the same bits, and the LayerSync step's loss is the plain
    step's loss minus lambda * similarity, the similarity as logged (fp32 rounding of a sum of two terms of order 20)"""
    lam = 0.5
    pa, ta, batch_a, _ = _gpu_trainer("sd3", scheduled_sampling_max_step_offset=2)
    pb, tb, batch_b, _ = _gpu_trainer("sd3", scheduled_sampling_max_step_offset=2, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=2, layersync_lambda=lam)
    seen = []
    for plug in (pa, pb):
        roll = plug.apply_scheduled_sampling_rollout
        plug.apply_scheduled_sampling_rollout = lambda p, roll=roll: seen.append(roll(p)) or seen[-1]
    la, lb = ta.train_step(dict(batch_a)).item(), tb.train_step(dict(batch_b)).item()
    assert torch.equal(seen[0]["noisy_latents"], seen[1]["noisy_latents"]) and torch.equal(seen[0]["_reflexflow_biased_pred"], seen[1]["_reflexflow_biased_pred"])
    logs = tb.last_aux_logs
    assert {"reflexflow_adr", "layersync_similarity", "layersync_loss"} <= set(logs)
    assert abs(lb - (la - lam * logs["layersync_similarity"])) < 1e-5 * max(1.0, abs(la))

"""Flow-DPO on the MI355X: the three kernels of simpletuner_amd/csrc/flow_dpo.hip element-wise inside the derived bounds of tests/flow_dpo_bounds.py (fp64 on the
same operands), bit-identical run to run, guard elements intact around every output; the EMA over three calls, an all-masked sample, a saturated logit; the tiny
SD3 / Flux steps against the oracle of tests/test_flow_dpo_cpu.py and one Trainer step on cuda:0."""
import ctypes as C

import pytest
import torch

from simpletuner_amd import lib as _lib
from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from tests import flow_dpo_bounds as FB
from tests import flow_dpo_ref as FR
from tests import parity_utils as PU
from tests import test_flow_dpo_cpu as TC
from tests import test_sd3_host_sequencing_cpu as SH

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64
SENTINEL = -7.0
SIZES = [8, 1024, 2056, 16384]          # one 16-byte group | a whole number of blocks | a ragged tail | several workgroups per sample


def _guarded(shape, dtype):
    """an output of `shape` in the middle of a larger buffer whose head and tail hold a sentinel: (tensor, (head, tail))"""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(shape), (buf[:GUARD], buf[GUARD + n:])


def _intact(guards):
    return all(bool((g.float() == SENTINEL).all()) for pair in guards for g in pair)


def _raw_chain(d, v, ema_state=None, upstream=None, grad_scale=1.0):
    """the three C entry points on guarded outputs (the ops wrappers allocate their own): (stats, loss, pair, logs, dpred, guards intact)"""
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    to = lambda t: None if t is None else t.to(DEV).contiguous()
    pol, ref, tw, tl, em = to(d.policy), to(d.ref), to(d.tw), to(d.tl), to(d.emask)
    p = lambda t: None if t is None else t.data_ptr()
    B, N = d.B, d.N
    period = 0 if em is None else em.shape[1]
    ws = torch.empty(L.st355_flow_dpo_workspace(B, N), dtype=torch.uint8, device=DEV)
    stats, g1 = _guarded((B, 9), F32)
    _lib.check(L.st355_flow_dpo_stats(st, p(pol), p(ref), p(tw), p(tl), p(em), period, p(stats), p(ws), B, N), "flow_dpo_stats")
    loss, g2 = _guarded((1,), F32)
    pair, g3 = _guarded((B, 4), F32)
    logs, g4 = _guarded((16,), F32)
    absmean, g5 = _guarded((1,), F32)
    inf = float("inf")
    _lib.check(L.st355_flow_dpo_head(st, p(stats), ops.FLOW_DPO_NORMS[v["norm_type"]], int(em is not None), 0, p(absmean), p(ema_state), int(ema_state is not None),
                                     v["beta"], v.get("auto_num", 0.0), v.get("decay", 0.99), v.get("beta_min", -inf), v.get("beta_max", inf), 1e-6, v["loss_weight"],
                                     v["anchor_alpha"], None, 0.0, p(pair), p(loss), p(logs), B, N), "flow_dpo_head")
    dpred, g6 = _guarded(tuple(pol.shape), BF16)
    _lib.check(L.st355_flow_dpo_grad(st, p(pol), p(ref), p(tw), p(tl), p(em), period, p(pair), p(dpred), B, N, v["anchor_alpha"], grad_scale, p(upstream)), "flow_dpo_grad")
    torch.cuda.synchronize()
    return stats, loss, pair, logs, dpred, _intact([g1, g2, g3, g4, g5, g6])


def _check_chain(d, v, outs, grad_scale=1.0, ema_state=None):
    stats, loss, pair, logs, dpred = outs
    worst = {}
    ref_s, tol_s = FB.stats_ref(d.policy, d.ref, d.tw, d.tl, d.emask)
    ok, worst["stats"] = FB.inside(stats, ref_s, tol_s)
    assert ok, ("stats", worst)
    hkw = dict(norm_type=v["norm_type"], has_mask=d.emask is not None, beta=v["beta"], loss_weight=v["loss_weight"], anchor_alpha=v["anchor_alpha"])
    if ema_state is not None:
        hkw.update(ema_state=ema_state, auto_num=v["auto_num"], decay=v["decay"], beta_min=v["beta_min"], beta_max=v["beta_max"])
    hr = FB.head_ref(stats, d.N, **hkw)
    # the input condition: every margin decided — above the head's bound on the kernel's stats AND above the stats' own bound
    nu = hr["pair"][0][:, 3]
    assert bool((hr["pair"][0][:, 0].abs() > hr["margin_bound"] + nu * (tol_s[:, 7] + tol_s[:, 8])).all()), "undecided margin"
    for name, got in (("loss", loss), ("pair", pair), ("logs", logs)):
        ok, worst[name] = FB.inside(got, *hr[name])
        assert ok, (name, worst)
    ok, worst["dpred"] = FB.inside(dpred, *FB.grad_ref(d.policy, d.ref, d.tw, d.tl, pair, d.emask, v["anchor_alpha"], grad_scale))
    assert ok, ("dpred", worst)
    assert bool(torch.isfinite(dpred).all())
    return worst


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_kernels_are_inside_the_derived_bounds_repeat_bit_for_bit_and_write_nothing_else(B, N):
    """norm_type x anchor on / off x mask none / [B, H W] broadcast over 16 channels (N = 1024, 16384).  FAILS WITHOUT THE FEATURE: the entry points do not exist."""
    worst_all = {}
    up = torch.tensor([0.5], device=DEV)
    for vi, tv in enumerate(TC.VARIANTS):
        period = N // 16 if tv["mask"] else None
        if tv["mask"] and N not in (1024, 16384):
            continue
        d = FR.operands(B, N, seed=1000 * B + vi, period=period)
        v = dict(norm_type=tv["norm_type"], beta=FR.f32(0.03 if tv["norm_type"] == "sum" else 4.0), loss_weight=FR.f32(0.7), anchor_alpha=FR.f32(tv["anchor_alpha"]))
        *o1, intact = _raw_chain(d, v, upstream=up, grad_scale=2.0)
        assert intact, ("guard elements written", B, N, tv)
        worst = _check_chain(d, v, o1, grad_scale=1.0)
        *o2, _ = _raw_chain(d, v, upstream=up, grad_scale=2.0)
        assert all(torch.equal(a, b) for a, b in zip(o1, o2)), ("not bit-identical", B, N, tv)
        # the ops wrappers launch the same thing
        to = lambda t: None if t is None else t.to(DEV)
        s3 = ops.flow_dpo_stats(to(d.policy), to(d.ref), to(d.tw), to(d.tl), to(d.emask))
        l3, p3, g3 = ops.flow_dpo_head(s3, N, norm_type=v["norm_type"], has_mask=d.emask is not None, beta=v["beta"], loss_weight=v["loss_weight"], anchor_alpha=v["anchor_alpha"])
        d3 = ops.flow_dpo_grad(to(d.policy), to(d.ref), to(d.tw), to(d.tl), p3, to(d.emask), anchor_alpha=v["anchor_alpha"], grad_scale=2.0, upstream=up)
        assert torch.equal(s3, o1[0]) and torch.equal(l3, o1[1]) and torch.equal(p3, o1[2]) and torch.equal(g3, o1[3]) and torch.equal(d3, o1[4])
        for k, w in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), w)
    print(f"[flow_dpo B={B} N={N}] worst error / bound: " + ", ".join(f"{k} {w:.3f}" for k, w in worst_all.items()))


def test_ema_over_three_calls_stays_on_the_device_and_inside_its_bound():
    B, N = 3, 1024
    state = torch.zeros(2, dtype=F32, device=DEV)
    v = dict(norm_type="mean", beta=1.0, loss_weight=1.0, anchor_alpha=0.0, auto_num=FR.f32(FR.auto_num(0.2, 1e-6)), decay=FR.f32(0.5), beta_min=FR.f32(1e-3),
             beta_max=FR.f32(50.0))
    betas = []
    for k in range(3):
        d = FR.operands(B, N, seed=40 + k, delta=0.1 * (k + 1))
        before = state.tolist()
        *o, intact = _raw_chain(d, v, ema_state=state)
        assert intact
        _check_chain(d, v, o, ema_state=before)
        hr = FB.head_ref(o[0], N, norm_type="mean", ema_state=before, auto_num=v["auto_num"], decay=v["decay"], beta_min=v["beta_min"], beta_max=v["beta_max"])
        ema, tol = hr["ema"]
        assert abs(float(state[0]) - float(ema)) <= float(tol) and float(state[1]) == 1.0
        betas.append(float(o[3][1]))
    assert len(set(betas)) == 3 and all(1e-3 < b < 50.0 for b in betas)          # the EMA moved beta, away from the clamps


def test_an_all_masked_sample_clamps_the_masked_mean_denominator_and_stays_finite():
    B, N = 3, 1024
    d = FR.operands(B, N, seed=7, period=64, all_masked=1)
    v = dict(norm_type="masked_mean", beta=4.0, loss_weight=1.0, anchor_alpha=0.5)
    stats, loss, pair, logs, dpred, intact = _raw_chain(d, v)
    assert intact and float(stats[1, 6]) == 0.0 and float(pair[1, 3]) == 1.0 and float(pair[1, 0]) == 0.0          # nu = 1 / max(0, 1), margin 0
    assert bool(torch.isfinite(loss).all() and torch.isfinite(logs).all() and torch.isfinite(dpred).all())
    hr = FB.head_ref(stats, N, norm_type="masked_mean", has_mask=True, beta=4.0, anchor_alpha=0.5)
    assert FB.inside(loss, *hr["loss"])[0] and FB.inside(pair, *hr["pair"])[0]
    assert FB.inside(dpred, *FB.grad_ref(d.policy, d.ref, d.tw, d.tl, pair, d.emask, 0.5, 1.0))[0]
    anchor_only = 0.5 / (B * N) * (d.policy.double() - d.ref.double())
    rows = dpred.cpu().double()
    assert torch.allclose(rows[1], anchor_only[1], rtol=2.0 ** -7, atol=1e-30) and torch.allclose(rows[B + 1], anchor_only[B + 1], rtol=2.0 ** -7, atol=1e-30)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_saturated_logit_keeps_log_sigma_and_sigma_finite(sign):
    """|logit| = 80: stats written by hand so that margin = +-160 at beta = 1"""
    B, N = 2, 1024
    stats = torch.zeros(B, 9, dtype=F32)
    stats[:, 7] = sign * 160.0
    stats[:, 0:4] = 100.0
    loss, pair, logs = ops.flow_dpo_head(stats.to(DEV), N, norm_type="sum", beta=1.0)
    assert bool(torch.isfinite(loss).all() and torch.isfinite(pair).all() and torch.isfinite(logs).all())
    assert pair[:, 1].tolist() == [sign * 80.0] * B
    hr = FB.head_ref(stats, N, norm_type="sum", beta=1.0)
    assert FB.inside(loss, *hr["loss"])[0] and FB.inside(pair, *hr["pair"])[0] and FB.inside(logs, *hr["logs"])[0]
    if sign > 0:
        assert 0.0 <= float(loss) < 1e-30 and 0.0 <= float(pair[0, 2]) < 1e-30
    else:
        assert abs(float(loss) - 80.0) < 1e-4 and abs(float(pair[0, 2]) - 0.5 / B) < 1e-6


def test_bad_arguments_are_refused():
    d = FR.operands(2, 64, seed=1)
    to = lambda t: t.to(DEV)
    with pytest.raises(St355Error):
        ops.flow_dpo_stats(to(d.policy)[:, :60], to(d.ref)[:, :60], to(d.tw)[:, :60], to(d.tl)[:, :60])          # per-sample size no multiple of 8
    with pytest.raises(St355Error):
        ops.flow_dpo_stats(to(d.policy), to(d.ref), to(d.tw), to(d.tl), torch.ones(2, 12, device=DEV))           # mask period no multiple of 8
    with pytest.raises(St355Error):
        ops.flow_dpo_stats(to(d.policy)[:3], to(d.ref)[:3], to(d.tw), to(d.tl))
    s = ops.flow_dpo_stats(to(d.policy), to(d.ref), to(d.tw), to(d.tl))
    _, pair, _ = ops.flow_dpo_head(s, 64)
    with pytest.raises(St355Error):
        ops.flow_dpo_grad(to(d.policy), None, to(d.tw), to(d.tl), pair, anchor_alpha=0.5)                         # the anchor needs the reference prediction
    assert ops.flow_dpo_grad(to(d.policy), None, to(d.tw), to(d.tl), pair).shape == d.policy.shape


# ------------------------------------------------------------------------------------------------
# the tiny SD3 / Flux steps against the oracle, one Trainer step
# ------------------------------------------------------------------------------------------------
def _gpu_trainer(family, ckpt, dcfg, B=2):
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family=family, train_batch_size=B, seed=3, lora_rank=8, lora_init_b_std=TC.B_STD, learning_rate=1e-3, distillation_method="flow_dpo",
                         distillation_config={"flow_dpo": dcfg}, **(dict(gradient_checkpointing=True, gradient_checkpointing_interval=1) if ckpt else {}))
    acc = St355Accelerator(DEV)
    if family == "flux":
        from simpletuner_amd.flux.model import Flux
        plugin = Flux(cfg, acc)
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, acc)
        plugin.load_model(**SH._arch(2))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, acc)
    cpu, devt, batch = TC._pairs(B)
    sig = devt["sigmas"].to(DEV)
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return plugin, trainer, batch, cpu


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "per-block-checkpointing"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_tiny_step_matches_the_oracle_on_the_device(family, ckpt):
    """one Trainer.train_step on cuda:0, B = 2 pairs, at the GPU parity tolerances of the families' LoRA tests: prediction rel-L2 2e-2, adapter gradients rel-L2 5e-2;
    the loss and beta against the fp64 head on the device's own two predictions, inside the kernels' derived bounds"""
    dcfg = TC.DCFGS[1]
    plugin, trainer, batch, cpu = _gpu_trainer(family, ckpt, dcfg)
    comp = plugin.get_trained_component()
    snap = TC.oracle_snapshot(comp)
    seen = []
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: (seen.append(predict(pb)), seen[-1])[1]
    grads = TC._capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    logs = trainer.last_aux_logs
    assert len(seen) == 2 and set(ops.FLOW_DPO_LOGS[:12]) <= set(logs) and "flow_dpo_anchor_loss" in logs
    o_loss, o_pred, o_grads, o_margin, o_beta, _, o_orig = TC.oracle_dpo_step(family, comp, cpu, dcfg, state=snap, beta_given=logs["flow_dpo_beta"])
    pred, ref = seen[0]["model_prediction"].detach().cpu(), seen[1]["model_prediction"].detach().cpu()
    assert pred.shape[0] == 4 and PU.rel_l2(pred, o_pred) < 2e-2
    e_loss, e_tol, e_beta, e_beta_tol = TC._head_on(pred, ref, cpu, dcfg)
    # (the plugin's own loss on the device sums in its kernel's order: the same fp32 bound)
    assert abs(loss.item() - e_loss) <= e_tol, (loss.item(), e_loss, e_tol)
    assert abs(logs["flow_dpo_beta"] - e_beta) <= e_beta_tol
    worst = TC._compare_grads({k: g.cpu() for k, g in grads.items()}, o_grads)
    assert comp.lora_groups and getattr(comp, "_lora_off", None) is None
    print(f"[gpu] {family} ckpt={ckpt}: loss {loss.item():.5f} (fp64 head on the device's predictions {e_loss:.5f}), oracle {o_loss.item():.5f}, worst adapter gradient "
          f"rel-L2 {worst:.3e}, beta {logs['flow_dpo_beta']:.4f}")

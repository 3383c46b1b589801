"""TwinFlow on the MI355X: the three kernels of simpletuner_amd/csrc/twinflow.hip element-wise inside the derived bounds of tests/twinflow_bounds.py (fp64 on the
same operands), bit-identical across two launches, with guard elements around every output and one refused call per precondition; the stand-ins of
tests/twinflow_ref.py op by op inside the same bounds; the tiny SD3 and Flux steps against the oracle of tests/test_twinflow_cpu.py with its tolerances; a 2-step
UCGM sample against the CPU path."""
import pytest
import torch

from simpletuner_amd import lib as _lib
from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests import twinflow_bounds as TB
from tests import twinflow_ref as TR
from tests.test_twinflow_cpu import UNIFORMS, _capture_grads, _compare_grads, clamp_inputs, oracle_twinflow_step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
SENTINEL = -7.0
BATCHES = [1, 2, 3]
SIZES = [8, 4104, 16 * 16 * 16]          # one vector | a sample that ends inside a lane group's last chunk (513 vectors) | several workgroup parts per sample


def guarded(t=None, shape=None, dtype=None):
    """a tensor in the middle of a larger buffer whose head and tail hold a sentinel: (view, whole buffer).  GUARD elements keep the view 16-byte aligned."""
    shape, dtype = (t.shape, t.dtype) if t is not None else (shape, dtype)
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if t is not None:
        view.copy_(t.to(DEV))
    return view, buf


def untouched(buf):
    return bool((buf[:GUARD].float() == SENTINEL).all()) and bool((buf[-GUARD:].float() == SENTINEL).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_rcgm_step_is_inside_the_derived_bounds_repeats_and_writes_nothing_else(B, N, first):
    g = torch.Generator().manual_seed(31 * B + N + int(first))
    x0, fc, acc0 = torch.randn(B, N, generator=g).to(BF16), torch.randn(B, N, generator=g).to(BF16), torch.randn(B, N, generator=g)
    t_prev = torch.tensor([0.62, 0.305, 0.97])[:B].contiguous()
    t_next = torch.tensor([0.61, 2.98e-7, 0.4])[:B].contiguous()
    ref = TB.rcgm_step_ref(x0, acc0, fc, t_prev, t_next, first)
    outs = []
    for _ in range(2):
        x, xbuf = guarded(x0)
        acc, abuf = guarded(acc0)
        rx, ra = ops.twinflow_rcgm_step(x, acc, fc.to(DEV), t_prev.to(DEV), t_next.to(DEV), first)
        assert rx is x and ra is acc
        okx, wx = TB.inside(x, *ref["x"])
        oka, wa = TB.inside(acc, *ref["acc"])
        assert okx and oka, (wx, wa)
        assert untouched(xbuf) and untouched(abuf), "guard elements written"
        outs.append((x.clone(), acc.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xs, accs = TR.twinflow_rcgm_step(x0.clone(), acc0.clone(), fc, t_prev, t_next, first)          # the stand-in, inside the same bounds
    assert TB.inside(xs, *ref["x"])[0] and TB.inside(accs, *ref["acc"])[0]
    print(f"[twinflow_rcgm_step B={B} N={N} first={first}] worst error / bound: x {wx:.3f}, acc {wa:.3f}")


def _loss_abi(pred, target, acc, cond, uncond, ratio, clamp, want_grad, grad_scale=1.0):
    """st355_twinflow_loss through the C ABI on guarded outputs: (losses, dpred, [buffers])"""
    L = _lib.load()
    B, N = pred.shape
    to = lambda t: None if t is None else t.to(DEV).contiguous()
    p, t, a, c, u = to(pred), to(target), to(acc), to(cond), to(uncond)
    losses, lbuf = guarded(shape=(2,), dtype=F32)
    dpred, dbuf = guarded(shape=(B, N), dtype=BF16) if want_grad else (None, None)
    ws, wbuf = guarded(shape=(max(int(L.st355_twinflow_workspace(B, N)) // 4, 1),), dtype=F32)
    _lib.check(L.st355_twinflow_loss(_stream(), _ptr(p), _ptr(t), _ptr(a), _ptr(c), _ptr(u), float(ratio), float(clamp), _ptr(losses), _ptr(dpred), _ptr(ws), B, N,
                                     float(grad_scale)), "twinflow_loss")
    return losses, dpred, [b for b in (lbuf, dbuf, wbuf) if b is not None]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_loss_is_inside_the_derived_bounds_repeats_and_writes_nothing_else(B, N):
    worst = {}
    for pair in (False, True):
        pred, target, acc, cond, uncond = clamp_inputs(B, N, 7 + B, pair)
        for clamp, want_grad, gs in ((1.0, True, 1.0), (0.25, True, 3.0), (1.0, False, 1.0)):
            ref = TB.loss_ref(pred, target, acc, cond, uncond, 0.5, clamp, gs)
            assert 0.1 <= ref["clamped"] <= 0.9, ref["clamped"]          # at least 10 % clamped and at least 10 % not, on the fp64 reference
            runs = []
            for _ in range(2):
                losses, dpred, bufs = _loss_abi(pred, target, acc, cond, uncond, 0.5, clamp, want_grad, gs)
                ok, w = TB.inside(losses, *ref["losses"])
                assert ok, ("losses", B, N, pair, clamp, w)
                worst["losses"] = max(worst.get("losses", 0.0), w)
                if want_grad:
                    ok, w = TB.inside(dpred, *ref["dpred"])
                    assert ok, ("dpred", B, N, pair, clamp, w)
                    worst["dpred"] = max(worst.get("dpred", 0.0), w)
                assert all(untouched(b) for b in bufs), "guard elements written"
                runs.append((losses.clone(), None if dpred is None else dpred.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and (runs[0][1] is None or torch.equal(runs[0][1], runs[1][1]))
            # the wrapper gives the ABI's bits; the stand-in sits inside the same bounds
            to = lambda t: None if t is None else t.to(DEV)
            wl, wd = ops.twinflow_loss(to(pred), to(target), to(acc), to(cond), to(uncond), 0.5, clamp, want_grad=want_grad, grad_scale=gs)
            assert torch.equal(wl, runs[0][0]) and ((wd is None) == (not want_grad)) and (wd is None or torch.equal(wd, runs[0][1]))
            sl, sd = TR.twinflow_loss(pred, target, acc, cond, uncond, 0.5, clamp, want_grad=want_grad, grad_scale=gs)
            assert TB.inside(sl, *ref["losses"])[0] and (sd is None or TB.inside(sd, *ref["dpred"])[0])
    print(f"[twinflow_loss B={B} N={N}] worst error / bound: " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_ucgm_step_is_inside_the_derived_bounds_repeats_and_writes_nothing_else(B, N):
    g = torch.Generator().manual_seed(5 * B + N)
    x0, v, noise = (torch.randn(B, N, generator=g).to(BF16) for _ in range(3))
    for (s_cur, s_next), (rho, nz) in zip(((0.999, 0.6), (0.6, 0.25), (0.25, 0.0)), ((1.0, noise), (0.375, noise), (0.0, None))):
        s_cur, s_next = float(torch.tensor(s_cur)), float(torch.tensor(s_next))
        ref, tol = TB.ucgm_step_ref(x0, v, s_cur, s_next, rho, nz)
        outs = []
        for _ in range(2):
            x, xbuf = guarded(x0)
            assert ops.twinflow_ucgm_step(x, v.to(DEV), s_cur, s_next, rho, None if nz is None else nz.to(DEV)) is x
            ok, worst = TB.inside(x, ref, tol)
            assert ok, (B, N, rho, worst)
            assert untouched(xbuf), "guard elements written"
            outs.append(x.clone())
        assert torch.equal(outs[0], outs[1])
        assert TB.inside(TR.twinflow_ucgm_step(x0.clone(), v, s_cur, s_next, rho, nz), ref, tol)[0]
        print(f"[twinflow_ucgm_step B={B} N={N} rho={rho}] worst error / bound = {worst:.3f}")


def test_every_precondition_refuses():
    """one refused call per ST_REQUIRE of csrc/twinflow.hip, through the C ABI (the wrappers check the same conditions first: a few of those below, too)"""
    L = _lib.load()
    B, N = 2, 64
    x, fc, nz = (torch.randn(B, N, device=DEV).to(BF16) for _ in range(3))
    acc, tp, tn = torch.zeros(B, N, device=DEV), torch.rand(B, device=DEV), torch.rand(B, device=DEV)
    losses, ws = torch.zeros(2, device=DEV), torch.zeros(int(L.st355_twinflow_workspace(B, N)) // 4 + 4, device=DEV)
    s, P = _stream(), _ptr
    step = lambda *a: _lib.check(L.st355_twinflow_rcgm_step(s, *a), "twinflow_rcgm_step")
    for args, what in (((None, P(acc), P(fc), P(tp), P(tn), 1, B, N), "null pointer"), ((P(x), P(acc), P(x), P(tp), P(tn), 1, B, N), "different buffers"),
                       ((P(x), P(acc), P(fc), P(tp), P(tn), 1, B, 60), "multiple of 8"), ((P(x) + 2, P(acc), P(fc), P(tp), P(tn), 1, B, 56), "16-byte aligned")):
        with pytest.raises(St355Error, match=what):
            step(*args)
    loss = lambda *a: _lib.check(L.st355_twinflow_loss(s, *a), "twinflow_loss")
    ok = (P(x), P(fc), P(acc), None, None, 0.5, 1.0, P(losses), None, P(ws), B, N, 1.0)
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, what in ((sub(7, None), "null pointer"), (sub(3, P(nz)), "come together"), (sub(11, 60), "bad shape"), (sub(6, -1.0), "must not be negative"),
                       (sub(2, P(acc) + 4), "16-byte aligned")):
        with pytest.raises(St355Error, match=what):
            loss(*args)
    ucgm = lambda *a: _lib.check(L.st355_twinflow_ucgm_step(s, *a), "twinflow_ucgm_step")
    for args, what in (((P(x), None, P(nz), 0.5, 0.25, 1.0, B * N), "null pointer"), ((P(x), P(x), P(nz), 0.5, 0.25, 1.0, B * N), "different buffers"),
                       ((P(x), P(fc), P(nz), 0.5, 0.25, 1.0, 60), "multiple of 8"), ((P(x), P(fc), P(nz), 0.5, 0.25, 1.5, B * N), r"must lie in \[0, 1\]"),
                       ((P(x), P(fc), None, 0.5, 0.25, 1.0, B * N), "needs noise")):
        with pytest.raises(St355Error, match=what):
            ucgm(*args)
    assert int(L.st355_twinflow_workspace(0, 64)) == 0 and int(L.st355_twinflow_workspace(3, 4096)) == 4 * 2 * 3 * 2
    # the wrappers
    with pytest.raises(St355Error):
        ops.twinflow_rcgm_step(x, acc, x, tp, tn, True)
    with pytest.raises(St355Error):
        ops.twinflow_loss(x, fc, acc, cond=nz)
    with pytest.raises(St355Error):
        ops.twinflow_loss(x[:, :60], fc[:, :60], acc[:, :60].contiguous())
    with pytest.raises(St355Error):
        ops.twinflow_ucgm_step(x, fc, 0.5, 0.25, 1.0, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# the plugins on the device
# ------------------------------------------------------------------------------------------------
def _trainer(family, negative=True, **cfg_kw):
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, **cfg_kw)
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
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"], "twinflow_uniforms": UNIFORMS}
    if negative:
        g = torch.Generator().manual_seed(99)
        cpu["negative"] = torch.randn(devt["prompt"].shape, generator=g).to(BF16).float()
        batch["negative_prompt_embeds"] = cpu["negative"].to(BF16).to(DEV)
    if trainer.ema_model is not None:
        g = torch.Generator().manual_seed(5)
        trainer.ema_model.shadow_flat.add_((0.02 * torch.randn(trainer.ema_model.shadow_flat.shape, generator=g)).to(DEV))
    return plugin, trainer, batch, cpu


@pytest.mark.parametrize("order,ratio,clamp", [(2, 0.5, 1.0), (3, 0.0, 0.25)])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_train_step_matches_the_twinflow_oracle_on_the_device(family, order, ratio, clamp):
    """the CPU test's oracle and tolerances: loss and logs 2e-3 * max(1, value), adapter gradients rel-L2 5e-2"""
    plugin, trainer, batch, cpu = _trainer(family, twinflow_enabled=True, use_ema=True, twinflow_estimate_order=order, twinflow_enhanced_ratio=ratio, twinflow_target_clamp=clamp)
    comp = plugin.get_trained_component()
    masters = comp.lora_flat.clone()

    o_loss, o_pred, o_grads, o_base, o_real, _ = oracle_twinflow_step(family, comp, cpu, trainer.ema_model.shadow_flat, order, ratio, clamp)
    assert torch.equal(comp.lora_flat, masters)
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    logs = trainer.last_aux_logs
    assert abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item()), (loss.item(), o_loss.item())
    assert abs(logs["twinflow_base"] - o_base) < 2e-3 * max(1.0, o_base) and abs(logs["twinflow_realvel"] - o_real) < 2e-3 * max(1.0, o_real), (logs, o_base, o_real)
    worst = _compare_grads({k: v.cpu() for k, v in grads.items()}, o_grads)
    print(f"[gpu] {family} order {order} ratio {ratio} clamp {clamp}: loss {loss.item():.5f} vs oracle {o_loss.item():.5f}, logs {logs} vs ({o_base:.5f}, {o_real:.5f}), "
          f"worst adapter gradient rel-L2 {worst:.3e}")


def test_two_step_ucgm_sample_matches_the_cpu_path():
    """the UCGM loop under the flag (2 steps, stochast_ratio 1, given start latents and per-step noise) on the device against the same loop on the CPU: the fp32
    oracle model with the component's weights and the fp64 step of tests/twinflow_ref.py, states rounded to bf16 where the device holds bf16.  Each of the two model
    calls enters the sample with a coefficient below 1 ((1 - s_next) s_cur), so the sample is held to twice the tiny SD3's prediction tolerance (rel-L2 2e-2)."""
    from oracle import sd3 as OS
    from simpletuner_amd import twinflow as TW
    plugin, trainer, batch, cpu = _trainer("sd3", twinflow_enabled=True, use_ema=True, twinflow_target_step_count=2)
    comp = plugin.get_trained_component()
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, 16, 16, 8, generator=g).to(BF16)
    noises = [torch.randn(2, 16, 16, 8, generator=g).to(BF16) for _ in range(2)]
    _, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    seen = []

    def predict(xt, t):
        seen.append(t.clone())
        b = {"latents": xt, "noisy_latents": xt, "timesteps": t, "prompt_embeds": devt["prompt"], "encoder_hidden_states": devt["prompt"], "add_text_embeds": devt["pooled"]}
        return plugin.model_predict(b)["model_prediction"]
    got = TW.ucgm_sample(predict, x0.to(DEV), 2, 1.0, noises=[n.to(DEV) for n in noises])
    sig = TW.ucgm_sigmas(2)
    assert [float(t[0]) for t in seen] == (sig[:-1] * 1000.0).tolist()
    P, lora, scale = PU.oracle_state(comp)
    P["pos_embed.pos_embed"] = comp.pos_embed.pos_embed.detach().float().cpu()
    ocfg = SH._ocfg(comp)
    x = x0.float()
    with torch.no_grad():
        for i in range(2):
            v = OS.sd3_forward(P, ocfg, x, cpu["prompt"], cpu["pooled"], torch.full((2,), float(sig[i] * 1000.0)), lora=lora, lora_scale=scale).to(BF16)
            x = TR.ucgm64(x, v, float(sig[i]), float(sig[i + 1]), 1.0, noises[i]).to(BF16).float()
    d = PU.rel_l2(got.cpu().float(), x)
    assert d < 2 * 2e-2, d
    print(f"[gpu] 2-step UCGM sample vs the CPU path: rel-L2 {d:.3e}")

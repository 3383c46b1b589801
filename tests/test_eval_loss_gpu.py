"""Evaluation loss on the MI355X: the two kernels of simpletuner_amd/csrc/eval_loss.hip — the views bit-equal to ops.flow_noise_mix slab by slab, the loss
element-wise inside the derived bounds of tests/eval_loss_bounds.py (fp64 on the same operands) and independent of K and of a slab's position, both bit-identical
across two launches, with guard elements around every output and one refused call per precondition; the tiny SD3 and Flux passes against the fp64 oracle of
tests/test_eval_loss_cpu.py under the loss tolerance of the families' forward-parity GPU tests; eval interleaved with training leaves training bit-equal."""
import pytest
import torch

from simpletuner_amd import lib as _lib
from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from tests import eval_loss_bounds as EB
from tests import eval_loss_ref as ER
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_eval_loss_cpu import _raw, _table, oracle_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
SENTINEL = -7.0
BATCHES = [1, 3]
SIZES = [8, 2056]          # a single vector | one full workgroup stride (256 lanes x 8) plus a tail vector


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


def _sigmas(K, g):
    s = torch.rand(K, generator=g)
    s[-1] = 1.0
    s[0] = 0.0
    if K > 2:
        s[1] = 0.98828125          # a value of the default grid's dtype chain
    return s


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_views_equal_flow_noise_mix_slab_by_slab_repeat_and_write_nothing_else(B, n, K):
    g = torch.Generator().manual_seed(17 * B + n + K)
    lat, noise = torch.randn(B, n, generator=g).to(BF16).to(DEV), torch.randn(B, n, generator=g).to(BF16).to(DEV)
    sig = _sigmas(K, g).to(DEV)
    runs = []
    for _ in range(2):
        out, obuf = guarded(shape=(K, B, n), dtype=BF16)
        assert ops.eval_flow_views(lat, noise, sig, out=out) is out
        assert untouched(obuf), "guard elements written"
        runs.append(out.clone())
    assert torch.equal(runs[0], runs[1])
    for k in range(K):
        want = ops.flow_noise_mix(lat, sig[k].expand(B).contiguous(), noise=noise)[0]
        assert torch.equal(runs[0][k], want), (B, n, K, k)
    assert torch.equal(ops.eval_flow_views(lat, noise, sig), runs[0])
    ref, tol = EB.views_ref(lat, noise, sig)
    ok, worst = EB.inside(runs[0], ref, tol)
    assert ok, worst
    assert EB.inside(ER.eval_flow_views(lat.cpu(), noise.cpu(), sig.cpu()), ref, tol)[0]          # the stand-in, inside the same bound
    print(f"[eval_flow_views B={B} n={n} K={K}] bit-equal to flow_noise_mix; worst error / bound {worst:.3f}")


def _loss_abi(pred, target, loss_type, huber_c):
    """st355_eval_loss through the C ABI on guarded outputs, the losses written into the middle of a longer table row: (loss [K], per_sample, buffers)"""
    L = _lib.load()
    K, B, n = pred.shape
    table, tbuf = guarded(shape=(K + 2,), dtype=F32)
    table.fill_(SENTINEL)
    per, pbuf = guarded(shape=(K, B), dtype=F32)
    ws, wbuf = guarded(shape=(max(int(L.st355_eval_loss_workspace(B, n, K)) // 4, 1),), dtype=F32)
    _lib.check(L.st355_eval_loss(_stream(), _ptr(pred), _ptr(target), ops.LOSS_TYPES[loss_type], _ptr(huber_c), _ptr(per), table.data_ptr() + 4, _ptr(ws), B, n, K),
               "eval_loss")
    assert float(table[0]) == SENTINEL and float(table[-1]) == SENTINEL, "the table row's neighbours were written"
    return table[1:K + 1], per, [tbuf, pbuf, wbuf]


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_loss_is_inside_the_derived_bounds_independent_of_the_chunk_repeats_and_writes_nothing_else(B, n, K):
    g = torch.Generator().manual_seed(3 * B + n + K)
    lat, noise = torch.randn(B, n, generator=g).to(BF16), torch.randn(B, n, generator=g).to(BF16)
    target = (noise.float() - lat.float()).to(BF16)
    pred = (target.float()[None] * 0.7 + torch.randn(K, B, n, generator=g)).to(BF16)
    pred[0, 0, :4] = target[0, :4]          # exact zeros of the difference (the huber cancellation's far end)
    pd, td = pred.to(DEV).contiguous(), target.to(DEV).contiguous()
    worst = {}
    cases = [("l2", None), ("huber", 0.1), ("smooth_l1", 0.1), ("huber", torch.rand(K * B, generator=g) * 0.5 + 0.01), ("smooth_l1", torch.rand(K * B, generator=g) + 0.01)]
    for lt, c in cases:
        ref = EB.loss_ref(pred, target, lt, c)
        c_dev = None if lt == "l2" else (c.to(DEV) if torch.is_tensor(c) else torch.full((K * B,), c, dtype=F32, device=DEV))
        runs = []
        for _ in range(2):
            loss, per, bufs = _loss_abi(pd, td, lt, c_dev)
            okl, wl = EB.inside(loss, *ref["loss"])
            okp, wp = EB.inside(per, *ref["per_sample"])
            assert okl and okp, (lt, B, n, K, wl, wp)
            worst[lt] = max(worst.get(lt, 0.0), wl, wp)
            assert all(untouched(b) for b in bufs), "guard elements written"
            runs.append((loss.clone(), per.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        wl_, wp_ = ops.eval_loss(pd, td, lt, c_dev if torch.is_tensor(c) else (c if c is not None else 0.1))          # the wrapper gives the ABI's bits
        assert torch.equal(wl_, runs[0][0]) and torch.equal(wp_, runs[0][1])
        for k in range(K):          # a slab alone (K = 1) gives the chunk's bits
            one_l, one_p = ops.eval_loss(pd[k:k + 1], td, lt, None if c_dev is None else c_dev[k * B:(k + 1) * B].contiguous())
            assert torch.equal(one_l[0], runs[0][0][k]) and torch.equal(one_p[0], runs[0][1][k]), (lt, k)
        sl, sp = ER.eval_loss(pred, target, lt, c)          # the stand-in, inside the same bounds
        assert EB.inside(sl, *ref["loss"])[0] and EB.inside(sp, *ref["per_sample"])[0]
    if n >= 2056:          # l2 against cond_loss: the same quantity from the training kernel, inside the same bound
        cl, cp, _ = ops.cond_loss(pd[0], td, "l2", want_grad=False)
        r = EB.loss_ref(pred[:1], target, "l2", None)
        assert EB.inside(cl, *r["loss"])[0]
    print(f"[eval_loss B={B} n={n} K={K}] worst error / bound: " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))


def test_every_precondition_refuses_and_writes_nothing():
    """one refused call per ST_REQUIRE of csrc/eval_loss.hip, through the C ABI (the wrappers check the same conditions first: a few of those below, too)"""
    L = _lib.load()
    B, n, K = 2, 64, 3
    lat, noise = (torch.randn(B, n, device=DEV).to(BF16) for _ in range(2))
    sig = torch.rand(K, device=DEV)
    sig65 = torch.rand(65, device=DEV)
    out, obuf = guarded(shape=(K, B, n), dtype=BF16)
    out.fill_(SENTINEL)
    s, P = _stream(), _ptr
    views = lambda *a: _lib.check(L.st355_eval_flow_views(s, *a), "eval_flow_views")
    for args, what in (((None, P(noise), P(sig), P(out), B, n, K), "null pointer"), ((P(lat), P(noise), P(sig), P(out), B, 60, K), "multiple of 8"),
                       ((P(lat), P(noise), P(sig), P(out), B, n, 0), r"must lie in \[1, 64\]"), ((P(lat), P(noise), P(sig65), P(out), B, n, 65), r"must lie in \[1, 64\]"),
                       ((P(lat), P(noise), P(sig), P(out) + 2, B, 56, K), "16-byte aligned"), ((P(lat) + 2, P(noise), P(sig), P(out), B, 56, K), "16-byte aligned"),
                       ((P(lat), P(noise), P(sig), P(lat), B, n, 1), "must not overlap"), ((P(lat), P(noise), P(sig), P(noise), B, n, 1), "must not overlap"),
                       ((P(out), P(noise), P(sig), P(out) + 2 * B * n, B, n, 1), None)):
        if what is None:          # (adjacent, not overlapping: accepted — the check is on the ranges, not on the pointers' order)
            views(*args)
            out.fill_(SENTINEL)
            continue
        with pytest.raises(St355Error, match=what):
            views(*args)
    torch.cuda.synchronize()
    assert bool((out.float() == SENTINEL).all()) and untouched(obuf), "a refused call wrote"
    pred = torch.randn(K, B, n, device=DEV).to(BF16)
    per, loss = torch.full((K, B), SENTINEL, device=DEV), torch.full((K,), SENTINEL, device=DEV)
    c = torch.full((K * B,), 0.1, device=DEV)
    ws = torch.zeros(int(L.st355_eval_loss_workspace(B, n, K)) // 4 + 4, device=DEV)
    call = lambda *a: _lib.check(L.st355_eval_loss(s, *a), "eval_loss")
    ok = (P(pred), P(lat), 1, P(c), P(per), P(loss), P(ws), B, n, K)
    sub = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, what in ((sub(5, None), "null pointer"), (sub(6, None), "null pointer"), (sub(2, 3), "loss_type"), (sub(3, None), "need huber_c"), (sub(8, 60), "bad shape"),
                       (sub(7, 65536), "bad shape"), (sub(9, 0), r"must lie in \[1, 64\]"), (sub(9, 65), r"must lie in \[1, 64\]"), (sub(0, P(pred) + 2), "16-byte aligned")):
        with pytest.raises(St355Error, match=what):
            call(*args)
    torch.cuda.synchronize()
    assert bool((per == SENTINEL).all()) and bool((loss == SENTINEL).all()), "a refused call wrote"
    assert int(L.st355_eval_loss_workspace(0, 64, 1)) == 0 and int(L.st355_eval_loss_workspace(3, 2056, 5)) == 4 * 5 * 3 * 2
    # the wrappers
    with pytest.raises(St355Error):
        ops.eval_flow_views(lat, noise[:, :56], sig)
    with pytest.raises(St355Error):
        ops.eval_flow_views(lat, noise, sig65)
    with pytest.raises(St355Error):
        ops.eval_flow_views(lat, noise, sig[:1], out=lat)
    with pytest.raises(St355Error):
        ops.eval_flow_views(lat.float(), noise, sig)
    with pytest.raises(St355Error):
        ops.eval_loss(pred, lat[:, :56])
    with pytest.raises(St355Error):
        ops.eval_loss(pred, lat, "huber", c[:4])
    with pytest.raises(St355Error):
        ops.eval_loss(pred, lat, "l1")
    with pytest.raises(St355Error):
        ops.eval_loss(pred, lat, loss_out=torch.zeros(K + 1, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# the plugins on the device
# ------------------------------------------------------------------------------------------------
def _trainer(family, eval_noise=True, fix_sigmas=True, **cfg_kw):
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
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    evals = [PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=s) for s in (4, 6)]
    trainer = Trainer(cfg, plugin, acc, eval_sets={"val": [_raw(e[1], eval_noise) for e in evals]})
    if fix_sigmas:
        plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    return plugin, trainer, _raw(devt), [e[0] for e in evals]


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_eval_table_matches_the_fp64_oracle_on_the_device_stacked_and_not(family):
    """the loss tolerance of tests/test_sd3_model_gpu.py / tests/test_flux_model_gpu.py: |d| < 1e-3 max(1, |loss|), for stack 1 and stack 4; the oracle table is
    computed once and shared"""
    want = None
    tables = {}
    for k in (1, 4):
        plugin, trainer, batch, eval_cpu = _trainer(family, eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=k)
        if want is None:
            grid = trainer.evaluation.get_timestep_schedule(trainer.evaluation.noise_scheduler_of(plugin), model=plugin)
            want = oracle_table(family, plugin.get_trained_component(), eval_cpu, grid)
        logs = trainer.evaluate()
        got = tables[k] = _table(trainer)
        worst = float(((got - want).abs() / want.clamp_min(1.0)).max())
        print(f"[gpu] {family} stack {k}: table {got.flatten().tolist()} vs oracle {want.flatten().tolist()}, worst |d| / max(1, loss) {worst:.3e}")
        assert got.shape == want.shape == (2, 4) and worst < 1e-3, (k, worst)
        assert abs(logs["loss/val/val"] - float(want.mean())) < 1e-3 * max(1.0, float(want.mean()))
    assert float(((tables[4] - tables[1]).abs() / tables[1].clamp_min(1.0)).max()) < 1e-3


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip_graph"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_eval_interleaved_with_three_steps_leaves_training_bit_equal(family, graph):
    """sigmas from torch's device generator, noise from the in-kernel counter stream: an eval after every step moves none of them.  Under hip_graph the eval runs
    eager between replays of the captured step and touches none of its static buffers: the replayed steps give the bits of the run without eval, and the eval logs
    are those of the eager run."""
    runs = {}
    for name, kw in (("plain", {}), ("eval", dict(eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=4))):
        plugin, trainer, batch, _ = _trainer(family, eval_noise=False, fix_sigmas=False, hip_graph=graph, **kw)
        batch.pop("noise")
        torch.manual_seed(77)
        losses = torch.stack([l.detach().reshape(()) for l in trainer.train([dict(batch) for _ in range(3)], 3)]).cpu()
        runs[name] = (losses, plugin.get_trained_component().lora_flat.clone().cpu(), plugin._noise_step, plugin._noise_offset, torch.cuda.get_rng_state().clone(),
                      len(trainer.eval_history))
        if name == "eval":
            _EVAL_LOGS[(family, graph)] = [logs for _, logs in trainer.eval_history]
        if name == "eval":
            a = trainer.evaluate()
            t1 = _table(trainer)
            assert a == trainer.evaluate() and torch.equal(t1, _table(trainer))          # the eval noise stream is fixed
            assert (plugin._noise_step, plugin._noise_offset) == runs[name][2:4] and not hasattr(plugin, "_eval_noise_seed")
    p, e = runs["plain"], runs["eval"]
    assert p[5] == 0 and e[5] == 3
    assert torch.equal(p[0], e[0]) and torch.equal(p[1], e[1]) and p[2:4] == e[2:4] and torch.equal(p[4], e[4])
    assert len(set(p[0].tolist())) == 3
    if graph and (family, False) in _EVAL_LOGS:          # the same weights and the same eval noise: the eval under replay logs what the eager run logged
        assert _EVAL_LOGS[(family, True)] == _EVAL_LOGS[(family, False)]


_EVAL_LOGS = {}

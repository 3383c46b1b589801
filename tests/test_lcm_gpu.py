"""LCM distillation on the device: the four kernels of csrc/lcm.hip inside their derived bounds (tests/lcm_bounds.py) against the fp64 restatement (tests/lcm_ref.py),
bit-identical across launches, guard bytes around every output; the tiny SDXL LoRA step and the three-step trajectory against the oracle; the sampler."""
import pytest
import torch

from tests import lcm_bounds as LB
from tests import lcm_ref as LR

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda:0"
GUARD = 64          # elements on either side of an output: a multiple of 16 bytes in both dtypes, so the guarded output keeps its alignment
SENTINEL = {BF16: -1.75, F32: -12345.5}


class Guarded:
    """an output carved out of a larger buffer filled with a sentinel: the kernel gets the inner pointer, the test checks the rims afterwards"""

    def __init__(self, shape, dtype, shift=0):
        n = 1
        for s in shape:
            n *= s
        self.n, self.shift = n, shift
        self.buf = torch.full((n + 2 * GUARD + shift,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[GUARD + shift:GUARD + shift + n].view(shape)

    def intact(self):
        lo, hi = self.buf[:GUARD + self.shift], self.buf[GUARD + self.shift + self.n:]
        want = SENTINEL[self.buf.dtype]
        return bool((lo == want).all()) and bool((hi == want).all())


def _d(t):
    return None if t is None else t.to(DEV)


def _abi():
    from simpletuner_amd import lib as _l
    from simpletuner_amd import ops
    return _l.load(), _l, ops


def _solver(o, mode, shift=0):
    L, _l, ops = _abi()
    x, pair, w, idx, start, sched, prev = _d(o.x_s), _d(o.pair), _d(o.w), _d(o.index), _d(o.start), _d(o.tb.sched), _d(o.tb.prev)
    g32, g16 = Guarded(o.shape, F32, shift), Guarded(o.shape, BF16, shift)
    _l.check(L.st355_lcm_solver_step(torch.cuda.current_stream().cuda_stream, x.data_ptr(), pair.data_ptr(), w.data_ptr(), idx.data_ptr(), start.data_ptr(), sched.data_ptr(),
                                     sched.shape[0], prev.data_ptr(), prev.shape[0], ops.LCM_MODES[mode], g32.view.data_ptr(), g16.view.data_ptr(), o.B, o.n), "lcm_solver_step")
    torch.cuda.synchronize()
    return g32, g16


def _target(o, mode, x32, shift=0):
    L, _l, ops = _abi()
    p, t, sched = _d(o.p_t), _d(o.t), _d(o.tb.sched)
    g = Guarded(o.shape, F32, shift)
    _l.check(L.st355_lcm_target(torch.cuda.current_stream().cuda_stream, x32.data_ptr(), p.data_ptr(), t.data_ptr(), sched.data_ptr(), sched.shape[0], ops.LCM_MODES[mode], 10.0,
                                g.view.data_ptr(), o.B, o.n), "lcm_target")
    torch.cuda.synchronize()
    return g


def _loss(o, mode, target, loss_type, grad_scale, shift=0):
    L, _l, ops = _abi()
    p, x, start, sched = _d(o.student), _d(o.x_s), _d(o.start), _d(o.tb.sched)
    gl, gp, gd = Guarded((1,), F32), Guarded((o.B,), F32), Guarded(o.shape, BF16, shift)
    ws = torch.empty(max(int(L.st355_lcm_workspace(o.B, o.n)), 4), dtype=torch.uint8, device=DEV)
    _l.check(L.st355_lcm_loss(torch.cuda.current_stream().cuda_stream, p.data_ptr(), x.data_ptr(), target.data_ptr(), start.data_ptr(), sched.data_ptr(), sched.shape[0],
                              ops.LCM_MODES[mode], 10.0, ops.LCM_LOSSES[loss_type], 0.001, gl.view.data_ptr(), gp.view.data_ptr(), gd.view.data_ptr(), ws.data_ptr(), o.B, o.n,
                              grad_scale), "lcm_loss")
    torch.cuda.synchronize()
    return gl, gp, gd


def _report(name, got, ref, tol):
    ok, worst = LB.inside(got, ref, tol)
    print(f"[lcm kernel] {name}: worst |err| / bound = {worst:.3f}")
    assert ok, (name, worst)


@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("shape", list(LR.SHAPES))
def test_kernels_inside_the_bounds_bit_identical_and_within_their_outputs(shape, mode):
    """[3,4,8,8], [2,4,6,10] (n = 240: thirty 16-byte groups), [1,4,8,8], [2,4,64,64] (8 workgroups per sample: the two-stage reduction) and [3,4,5,7] (n = 140: the
    scalar walk and its tail); indices 0 and N - 1 in every batch of more than one sample (the t = 0 boundary, the smallest alpha)"""
    _, _, ops = _abi()
    o = LR.operands(shape, seed=21, mode=mode)
    if o.B > 1:
        assert 0 in o.index.tolist() and 49 in o.index.tolist()
    else:
        assert o.index.tolist() == [49]
    a32, a16 = _solver(o, mode)
    b32, b16 = _solver(o, mode)
    assert torch.equal(a32.view, b32.view) and torch.equal(a16.view, b16.view) and all(g.intact() for g in (a32, a16, b32, b16))
    ref = LB.solver_ref(o.x_s, o.pair, o.w, o.index, o.start, o.tb.sched, o.tb.prev, mode)
    _report(f"{shape} {mode} x_prev32", a32.view, *ref["x_prev32"])
    _report(f"{shape} {mode} x_prev16", a16.view, *ref["x_prev16"])
    assert torch.equal(a16.view, a32.view.to(BF16))                                                  # the bf16 copy is the fp32 value rounded once
    w32, w16 = ops.lcm_solver_step(_d(o.x_s), _d(o.pair), _d(o.w), _d(o.index), _d(o.start), _d(o.tb.sched), _d(o.tb.prev), mode)
    assert torch.equal(w32, a32.view) and torch.equal(w16, a16.view)                                 # the wrapper launches the same kernel
    x32 = a32.view.contiguous()
    ta, tb_ = _target(o, mode, x32), _target(o, mode, x32)
    assert torch.equal(ta.view, tb_.view) and ta.intact() and tb_.intact()
    tref = LB.target_ref(x32.cpu(), o.p_t, o.t, o.tb.sched, mode)
    _report(f"{shape} {mode} target", ta.view, *tref["target"])
    zero = (o.t == 0).to(DEV)
    assert torch.equal(ta.view[zero], x32[zero])                                                     # t = 0: target = x_prev exactly
    assert torch.equal(ops.lcm_target(x32, _d(o.p_t), _d(o.t), _d(o.tb.sched), mode), ta.view)
    target = ta.view.contiguous()
    for lt in LR.LOSSES:
        la, lb = _loss(o, mode, target, lt, 0.5), _loss(o, mode, target, lt, 0.5)
        assert all(torch.equal(x.view, y.view) for x, y in zip(la, lb)) and all(g.intact() for g in la + lb)
        lref = LB.loss_ref(o.student, o.x_s, target.cpu(), o.start, o.tb.sched, mode, loss_type=lt, grad_scale=0.5)
        for nm, g in zip(("loss", "per_sample", "dpred"), la):
            _report(f"{shape} {mode} {lt} {nm}", g.view, *lref[nm])
        wl = ops.lcm_loss(_d(o.student), _d(o.x_s), target, _d(o.start), _d(o.tb.sched), mode, loss_type=lt, grad_scale=0.5)
        assert all(torch.equal(x, g.view) for x, g in zip(wl, la))
        assert ops.lcm_loss(_d(o.student), _d(o.x_s), target, _d(o.start), _d(o.tb.sched), mode, loss_type=lt, want_grad=False)[2] is None


@pytest.mark.parametrize("mode", LR.MODES)
def test_misaligned_outputs_take_the_scalar_walk(mode):
    """n % 8 == 0 but the outputs start 4 (fp32) / 2 (bf16) bytes off a 16-byte boundary: the scalar instantiation (the compiler may fuse its multiply-adds otherwise
    than the vector one's, so its values are held to the same bounds, not to the same bits), the same bits across two launches, and the rims untouched"""
    o = LR.operands("small", seed=22, mode=mode)
    s32, s16 = _solver(o, mode, shift=1)
    r32, r16 = _solver(o, mode, shift=1)
    assert s32.view.data_ptr() % 16 == 4 and s16.view.data_ptr() % 16 == 2
    assert torch.equal(s32.view, r32.view) and torch.equal(s16.view, r16.view) and s32.intact() and s16.intact()
    ref = LB.solver_ref(o.x_s, o.pair, o.w, o.index, o.start, o.tb.sched, o.tb.prev, mode)
    _report(f"misaligned {mode} x_prev32", s32.view, *ref["x_prev32"])
    _report(f"misaligned {mode} x_prev16", s16.view, *ref["x_prev16"])
    x32 = s32.view.contiguous()
    ts, tr = _target(o, mode, x32, shift=1), _target(o, mode, x32, shift=1)
    assert torch.equal(ts.view, tr.view) and ts.intact()
    _report(f"misaligned {mode} target", ts.view, *LB.target_ref(x32.cpu(), o.p_t, o.t, o.tb.sched, mode)["target"])
    target = ts.view.contiguous()
    ls, lr = _loss(o, mode, target, "l2", 1.0, shift=1), _loss(o, mode, target, "l2", 1.0, shift=1)
    assert all(torch.equal(x.view, y.view) for x, y in zip(ls, lr)) and all(g.intact() for g in ls)
    lref = LB.loss_ref(o.student, o.x_s, target.cpu(), o.start, o.tb.sched, mode)
    for nm, g in zip(("loss", "per_sample", "dpred"), ls):
        _report(f"misaligned {mode} {nm}", g.view, *lref[nm])


def test_out_of_range_indices_clamp_to_their_tables():
    _, _, ops = _abi()
    o = LR.operands("small", seed=23, mode="epsilon")
    run = lambda idx, start: ops.lcm_solver_step(_d(o.x_s), _d(o.pair), _d(o.w), _d(idx), _d(start), _d(o.tb.sched), _d(o.tb.prev), "epsilon")
    a = run(torch.tensor([50, -3, 25]), torch.tensor([1000, -1, 519]))
    b = run(torch.tensor([49, 0, 25]), torch.tensor([999, 0, 519]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    tg = ops.lcm_target(a[0], _d(o.p_t), _d(torch.tensor([5000, -7, 499])), _d(o.tb.sched), "epsilon")
    assert torch.equal(tg, ops.lcm_target(a[0], _d(o.p_t), _d(torch.tensor([999, 0, 499])), _d(o.tb.sched), "epsilon"))


@pytest.mark.parametrize("mode", LR.MODES)
@pytest.mark.parametrize("shape", ["small", "tail"])
def test_sample_step_inside_the_bounds(shape, mode):
    L, _l, ops = _abi()
    o = LR.operands(shape, seed=24, mode=mode)
    sched, x, p = _d(o.tb.sched), _d(o.x_s), _d(o.student)
    for t, tn, nz in ((999, 759, o.noise), (259, -1, None)):
        outs = []
        nd = _d(nz)
        for _ in range(2):
            g = Guarded(o.shape, BF16)
            _l.check(L.st355_lcm_sample_step(torch.cuda.current_stream().cuda_stream, x.data_ptr(), p.data_ptr(), None if nd is None else nd.data_ptr(),
                                             sched.data_ptr(), sched.shape[0], ops.LCM_MODES[mode], 10.0, t, tn, g.view.data_ptr(), o.B * o.n), "lcm_sample_step")
            torch.cuda.synchronize()
            outs.append(g)
        assert torch.equal(outs[0].view, outs[1].view) and outs[0].intact() and outs[1].intact()
        _report(f"{shape} {mode} sample step t={t}", outs[0].view, *LB.sample_ref(o.x_s, o.student, nz, o.tb.sched, t, tn, mode)["out"])
        assert torch.equal(ops.lcm_sample_step(_d(o.x_s), _d(o.student), _d(nz), sched, t, tn, mode=mode), outs[0].view)


# ---- the step ----
def _sdxl(**over):
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import St355Accelerator, default_config
    from tests import test_unet_host_sequencing_cpu as UN
    cfg = default_config(model_family="sdxl", model_type="lora", lora_rank=16, lora_alpha=16.0, lora_init_b_std=0.05, train_batch_size=2, learning_rate=1e-3,
                         distillation_method="lcm", **over)
    acc = St355Accelerator(torch.device(DEV))
    pl = SDXL(cfg, acc)
    pl.load_model(**UN.SMALL)
    pl.add_lora_adapter()
    return pl, UN.SMALL, cfg, acc


def _on(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def test_tiny_sdxl_lora_step_equals_the_oracle_and_the_restatement():
    """the CPU test's step on the device (tests/test_lcm_cpu.py): teacher forwards against the base oracle at 2e-2, every kernel stage inside its bound on the step's own
    operands, adapter gradients against autograd through the oracle UNet + the restated loss at 6e-2"""
    from simpletuner_amd.lcm import LCMDistiller
    from tests import test_lcm_cpu as TC
    from tests import test_unet_host_sequencing_cpu as UN
    pl, arch, cfg, acc = _sdxl()
    dist = LCMDistiller(pl)
    batch = TC._batch("sdxl")
    prepared, pred, loss, logs, calls = TC._run_step(pl, dist, _on(batch))
    torch.cuda.synchronize()
    B, mode = 2, "epsilon"
    tb = LR.tables(pl.noise_schedule.alphas_cumprod, 50)
    idx = batch["lcm_index"]
    start, t = tb.ddim_t[idx], (tb.ddim_t[idx] - 20).clamp_min(0)
    c = lambda x: x.detach().cpu()
    x_s = c(prepared["noisy_latents"])
    (tb2, pair), (tb1, p_t) = calls
    base, _ = TC._oracle(pl, arch, True, with_lora=False)
    adapted, lora = TC._oracle(pl, arch, True, with_lora=True)
    ack = lambda b: {k: c(v) for k, v in b["added_cond_kwargs"].items()}
    with torch.no_grad():
        o_pair = base(c(tb2["noisy_latents"]), c(tb2["timesteps"]), c(tb2["encoder_hidden_states"]), ack(tb2))
        o_pt = base(c(tb1["noisy_latents"]), c(tb1["timesteps"]), c(tb1["encoder_hidden_states"]), ack(tb1))
    r_pair, r_pt = UN._rel(c(pair), o_pair), UN._rel(c(p_t), o_pt)
    print(f"[lcm gpu] teacher pair vs base oracle {r_pair:.3e}, target forward {r_pt:.3e}")
    assert r_pair < 2e-2 and r_pt < 2e-2
    sched, prev = c(dist.sched_table), c(dist.prev_table)
    ref = LB.solver_ref(x_s, c(pair), c(prepared["guidance_scale"]), idx, start, sched, prev, mode)
    assert LB.inside(prepared["_lcm"]["x_prev"], *ref["x_prev32"])[0] and LB.inside(tb1["noisy_latents"], *ref["x_prev16"])[0]
    assert LB.inside(prepared["target"], *LB.target_ref(c(prepared["_lcm"]["x_prev"]), c(p_t), t, sched, mode)["target"])[0]
    assert torch.equal(prepared["target"][1], prepared["_lcm"]["x_prev"][1])
    lref = LB.loss_ref(c(pred).to(BF16), x_s, c(prepared["target"]), start, sched, mode)
    assert LB.inside(loss.detach().reshape(1), lref["loss"][0].reshape(1), lref["loss"][1].reshape(1))[0]
    assert float(logs["lcm_loss"]) == float(loss.detach())
    flat = lambda x: x.to(F64).reshape(B, -1)
    o_pred = adapted(x_s, start, c(prepared["encoder_hidden_states"]), ack(prepared))
    o_loss = LR.loss64(o_pred.reshape(B, -1), flat(x_s), flat(c(prepared["target"])), start, sched, mode)
    o_loss.backward()
    worst = max((UN._rel(c(p.grad), lora[n].grad), n) for n, p in pl.model.named_parameters() if ".lora_" in n)
    print(f"[lcm gpu] student vs oracle {UN._rel(c(pred), o_pred.detach()):.3e}; loss {float(loss.detach()):.6f} (oracle {float(o_loss.detach()):.6f}); worst gradient {worst}")
    assert UN._rel(c(pred), o_pred.detach()) < 2e-2 and worst[0] < 6e-2


def test_three_step_trajectory_follows_the_oracle():
    """tests/test_lcm_cpu.py's trajectory on the device: |loss difference| <= 2e-3 max(1, |loss|) per step, adapters within 6e-2 of the oracle's after three steps"""
    import simpletuner_amd.training.trainer as TR
    from tests import test_lcm_cpu as TC
    from tests import test_unet_host_sequencing_cpu as UN
    pl, arch, cfg, acc = _sdxl()
    tr = TR.Trainer(cfg, pl, acc)
    base, _ = TC._oracle(pl, arch, True, with_lora=False)
    adapted, lora = TC._oracle(pl, arch, True, with_lora=True)
    names = sorted(lora)
    for n in names:
        lora[n] = torch.nn.Parameter(lora[n].detach().clone())
    opt = torch.optim.AdamW([lora[n] for n in names], lr=cfg.learning_rate, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon, weight_decay=cfg.adam_weight_decay)
    tb = LR.tables(pl.noise_schedule.alphas_cumprod, 50)
    hip, ora = [], []
    for step in range(3):
        batch = TC._batch("sdxl", seed=20 + step, index=((12, 0), (30, 5), (0, 20))[step], w=((2.0, 1.0), (1.5, 3.0), (1.0, 2.5))[step])
        hip.append(float(tr.train_step(_on(batch))))
        B = 2
        idx = batch["lcm_index"]
        start, t = tb.ddim_t[idx], (tb.ddim_t[idx] - 20).clamp_min(0)
        a = tb.sched[start].to(F64)
        x_s = (a[:, 0].reshape(B, 1, 1, 1) * batch["latent_batch"].to(F64) + a[:, 1].reshape(B, 1, 1, 1) * batch["lcm_noise"].to(F64)).to(BF16)
        ehs, te, ti = batch["prompt_embeds"], batch["add_text_embeds"], batch["batch_time_ids"]
        ack = {"text_embeds": te, "time_ids": ti}
        with torch.no_grad():
            pc = base(x_s, start, ehs, ack)
            pu = base(x_s, start, torch.zeros_like(ehs), {"text_embeds": torch.zeros_like(te), "time_ids": ti})
            xp = LR.solver64(x_s, torch.cat([pc, pu]), batch["lcm_guidance_scale"], idx, start, tb.sched, tb.prev64, "epsilon")["x_prev"].reshape(x_s.shape)
            target = LR.target64(xp, base(xp, t, ehs, ack), t, tb.sched, "epsilon")["target"]
        opt.zero_grad()
        l = LR.loss64(adapted(x_s, start, ehs, ack).reshape(B, -1), x_s.to(F64).reshape(B, -1), target, start, tb.sched, "epsilon")
        l.backward(); opt.step()
        ora.append(float(l.detach()))
    worst = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(hip, ora))
    print(f"[lcm gpu] 3 steps: loss hip {[round(x, 6) for x in hip]} oracle {[round(x, 6) for x in ora]}; worst {worst:.3e}")
    assert worst <= 2e-3
    for n, p in pl.model.named_parameters():
        if ".lora_" in n:
            assert UN._rel(p.detach().cpu(), lora[n].detach()) < 6e-2, n


def test_lcm_sample_on_the_device_matches_the_restatement_step_by_step():
    """a 4-step lcm_sample with injected noise: every step's output inside the sampler bound around the fp64 step from the SAME bf16 state, and sample_images under the
    method takes this sampler"""
    from simpletuner_amd import sampling
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(2, 4, 8, 8, generator=g)
    noises = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(3)]
    sched = sampling.LCMScheduler(prediction_type="epsilon")
    states, preds = [lat.to(BF16)], []

    def predict(x, t):
        out = (0.7 * x.float() + 0.1 * torch.sin(t.float()).reshape(-1, 1, 1, 1)).to(BF16)
        preds.append(out.cpu())
        return out
    got = sampling.lcm_sample(predict, lat.to(DEV), sched, 4, noises=noises, on_step=lambda i, x: states.append(x.cpu()))
    torch.cuda.synchronize()
    ts = [999, 759, 499, 259]
    assert len(states) == 5 and torch.equal(got.cpu(), states[-1])
    for i, t in enumerate(ts):
        last = i == 3
        ref = LB.sample_ref(states[i], preds[i], None if last else noises[i].to(BF16), sched.table, t, -1 if last else ts[i + 1], "epsilon")["out"]
        _report(f"lcm_sample step {i}", states[i + 1], *ref)
    pl, arch, cfg, acc = _sdxl()
    x = sampling.sample_images(pl, torch.randn(1, 9, 128), torch.randn(1, 64), 8, 8, num_inference_steps=4, decode=False, latents=torch.randn(1, 4, 8, 8),
                               generator=torch.Generator(device=DEV).manual_seed(1),
                               extra_batch={"added_cond_kwargs": {"time_ids": torch.tensor([[64.0, 48.0, 0.0, 0.0, 64.0, 48.0]], device=DEV)}})
    assert x.shape == (1, 4, 8, 8) and bool(torch.isfinite(x.float()).all())

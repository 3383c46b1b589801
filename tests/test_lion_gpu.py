"""Lion on the MI355X (simpletuner_amd/csrc/lion.hip) through the C ABI via ops.lion_step, element-wise against the fp64 restatement of tests/lion_bounds.py: both
arenas with guarded buffers and the run-twice determinism check of tests/test_step_bounds_gpu.py, exact zeros, what the Kahan buffer is for, St355Lion's one-launch
path and resume, three trainer steps of Flux LoRA (fp32 arena) and of an SD3 full fine-tune with fused EMA (bf16 arena), and a captured step.

The trajectories are checked CHAINED: each step's stored p, g and m before the step go through lion_bounds, and the stored results are held to its bounds.  Parameters are
deliberately not compared with an independent oracle trajectory: sign() turns bf16 gradient noise into a 2 lr difference per flipped element.  The share of elements
whose sign differs from the fp32 oracle's own Lion trajectory is printed (profiles/lion_step_kernel_stats.md records it), not asserted."""
import pytest
import torch

from tests import gemm_bounds as GB
from tests import lion_bounds as LB

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = torch.device("cuda:0")
SENT = 73728.0           # sentinel (2^16 + 2^13: exact in bf16 and fp32), far from every value the kernels produce
PAD = 32                 # guard elements on both sides of a flat arena (keeps 16-byte alignment for fp32 and bf16)
GOLD = LB.golden()
H = GOLD["hyper"]


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o
    return o


def _guarded(t, pad=PAD):
    n = t.numel()
    buf = torch.full((n + 2 * pad,), SENT, dtype=t.dtype, device=t.device)
    buf[pad:pad + n] = t.reshape(-1)
    return buf, buf[pad:pad + n]


def _guards_ok(buf, what, pad=PAD):
    s = torch.tensor(SENT, dtype=buf.dtype, device=buf.device)
    assert bool((buf[:pad] == s).all()) and bool((buf[-pad:] == s).all()), f"{what}: wrote outside its arena"


def _same(a, b, what):
    assert torch.equal(LB.bits(a), LB.bits(b)), f"{what}: two runs differ"


_INPUTS = {}


def _inputs(n, dtype):
    """the shared seeded inputs, drawn once per (n, dtype) and never written"""
    key = (n, dtype)
    if key not in _INPUTS:
        _INPUTS[key] = LB.make_inputs(n, dtype, GOLD["seeds"]["fp32" if dtype == F32 else "bf16"], grad_scale=H["grad_scale"], beta1=H["beta1"], device=DEV)
    return _INPUTS[key]


def _lion_case(ops, n, dtype, wd, with_ema, with_pb=False, kahan=False):
    name = f"lion {dtype} n={n} wd={wd} ema={with_ema} p_bf16={with_pb} kahan={kahan}"
    x = _inputs(n, dtype)
    p0, g0, m0, c0, e0 = x["p"], x["g"], x["m"], x["comp"], x["ema"]
    c = LB.lion_consts(H["lr"], H["beta1"], H["beta2"], wd, H["grad_scale"], H["ema_decay"])
    (pb_, p), (mb_, m), (cb_, comp), (eb_, ema), (gb_, g) = [_guarded(t) for t in (p0, m0, c0, e0, g0)]
    hb_, pbf = _guarded(torch.full((n,), SENT, dtype=BF16, device=DEV))
    kw = dict(ema=ema if with_ema else None, ema_decay=H["ema_decay"])
    if dtype == F32:
        kw["p_bf16"] = pbf if with_pb else None
    else:
        kw["comp"] = comp if kahan else None
    run = lambda: ops.lion_step(p, g, m, H["lr"], H["beta1"], H["beta2"], wd, grad_scale=H["grad_scale"], **kw)
    run()
    first = [t.clone() for t in (p, m, comp, ema, pbf)]
    for t, t0 in ((p, p0), (m, m0), (comp, c0), (ema, e0)):
        t.copy_(t0)
    pbf.fill_(SENT)
    run()
    for t, f in zip((p, m, comp, ema, pbf), first):
        _same(t, f, name)
    for b_ in (pb_, mb_, cb_, eb_, gb_, hb_):
        _guards_ok(b_, name)
    assert torch.equal(LB.bits(g), LB.bits(g0)), f"{name}: the gradient was written"
    reports, info = LB.check_step(name, c, p0, g0, m0, p, m, c0 if kahan else None, comp if kahan else None)
    LB.assert_reports(reports)
    if x["cancel"] and dtype == F32:
        assert info["undecided"] > 0, f"{name}: the cancelling elements did not reach the undecided branch"
    if not kahan:
        assert torch.equal(LB.bits(comp), LB.bits(c0)), f"{name}: a compensation buffer that was not passed changed"
    if with_ema:                                               # chained on the stored new parameter
        if dtype == F32:
            LB.assert_reports([LB.check_f32(f"{name} ema", ema, *LB.ema_f32(e0, p, c["omd"]))])
        else:
            LB.assert_reports([LB.check_bf16(f"{name} ema", ema, *LB.ema_bf16(e0, p, c["omd"]), flat=True)])
    else:
        assert torch.equal(LB.bits(ema), LB.bits(e0)), f"{name}: an EMA shadow that was not passed changed"
    if with_pb:
        assert torch.equal(LB.bits(pbf), LB.bits(GB.to_bf16_rne(p))), f"{name}: p_bf16 is not one RNE of the stored parameter"
    else:
        assert bool((pbf == SENT).all())
    # exact zeros: g == 0 and m == 0 (and comp == 0 there)
    z = x["zeros"]
    assert not m[:z].any(), f"{name}: a zero gradient on a zero momentum must leave the momentum zero"
    if wd == 0.0:
        assert torch.equal(LB.bits(p[:z]), LB.bits(p0[:z])), f"{name}: the bits of p changed where g == 0 and m == 0"
    else:
        lrwd = torch.tensor(H["lr"], dtype=F32, device=DEV) * torch.tensor(wd, dtype=F32, device=DEV)
        pf = p0[:z].float()
        want = (pf - lrwd * pf).to(dtype)                      # exactly the decayed value: fp32(p - fp32(fp32(lr wd) p)), then the arena's one RNE
        assert torch.equal(p[:z], want), f"{name}: p is not exactly the decayed value where g == 0 and m == 0"


@pytest.mark.parametrize("n", [1027, 2097152 + 3])
def test_lion_fp32_arena(ops, n):
    """the n % 4 tail and (n > 2 097 152) a second grid-stride pass; weight decay 0 and 1e-2; with and without ema; with and without p_bf16; grad_scale 0.5"""
    _lion_case(ops, n, F32, 1e-2, True, with_pb=True)
    _lion_case(ops, n, F32, 0.0, False, with_pb=False)
    _lion_case(ops, n, F32, 0.0, True, with_pb=False)
    _lion_case(ops, n, F32, 1e-2, False, with_pb=True)


@pytest.mark.parametrize("n", [1032, 2097152 + 8])
def test_lion_bf16_arena(ops, n):
    """Kahan on and off, with and without ema, weight decay 0 and 1e-2; with comp == NULL nothing but p, m (and ema) changes"""
    _lion_case(ops, n, BF16, 1e-2, True, kahan=True)
    _lion_case(ops, n, BF16, 0.0, False, kahan=True)
    _lion_case(ops, n, BF16, 0.0, True, kahan=False)
    _lion_case(ops, n, BF16, 1e-2, False, kahan=False)


def test_bad_arguments_are_refused(ops):
    from simpletuner_amd import lib
    p = torch.zeros(1028, dtype=BF16, device=DEV)
    with pytest.raises(lib.St355Error):
        ops.lion_step(p[:1027], p[:1027].clone(), p[:1027].clone(), 1e-3)            # bf16 arena: n % 8 != 0
    q = torch.zeros(1028, dtype=F32, device=DEV)
    with pytest.raises(lib.St355Error):
        ops.lion_step(q[1:], q[1:].clone(), torch.zeros(1027, dtype=F32, device=DEV), 1e-3)      # p not 16-byte aligned
    with pytest.raises(lib.St355Error):
        ops.lion_step(q, q.clone(), q.clone(), 1e-3, comp=p)                         # fp32 arena takes no compensation buffer


def test_what_the_compensation_buffer_is_for(ops):
    """p0 = 1.0 in bf16, g = +1 everywhere, lr 1e-4, no decay, 64 steps.  Half a bf16 ulp below 1.0 is 1.95e-3 > lr, so without the buffer every update rounds away and
    p stays bit-equal to p0; with it, p + comp (in fp64) tracks 1 - k lr within the per-step bound of lion_bounds summed over the steps, and p has moved by step 64."""
    n, lr, steps = 4096, 1e-4, 64
    one = lambda: torch.ones(n, dtype=BF16, device=DEV)
    g = one()
    p, m = one(), torch.zeros(n, dtype=BF16, device=DEV)
    for _ in range(steps):
        ops.lion_step(p, g, m, lr, 0.9, 0.99, 0.0)
    assert torch.equal(LB.bits(p), LB.bits(one())), "without a compensation buffer an update below half an ulp cannot move p"
    p, m, comp = one(), torch.zeros(n, dtype=BF16, device=DEV), torch.zeros(n, dtype=BF16, device=DEV)
    c = LB.lion_consts(lr, 0.9, 0.99, 0.0, 1.0)
    budget = torch.zeros(n, dtype=F64, device=DEV)
    for k in range(1, steps + 1):
        p_b, m_b, c_b = p.clone(), m.clone(), comp.clone()
        ops.lion_step(p, g, m, lr, 0.9, 0.99, 0.0, comp=comp)
        ref = LB.Ref(p_b, g, m_b, c, c_b)
        assert bool(ref.decided.all()) and bool((ref.s == 1).all())
        _, e_t, t = ref.update(ref.s)
        moved = p.to(F64) - p_b.to(F64)
        cw = t - moved
        e = e_t + LB.U * moved.abs() + LB.U * cw.abs()
        budget += 0.5 * GB.ulp_bf16(cw.abs() + e) + e            # the step's bound on (p' + comp') - (p + comp + d): comp' is the only rounded quantity that is not carried
        err = (p.to(F64) + comp.to(F64) - (1.0 - k * c["lr"])).abs()
        assert bool((err <= budget).all()), (k, float(err.max()), float(budget.max()))
    assert bool((p != one()).all()), "with the compensation buffer 64 updates of 1e-4 must have moved every element"
    print(f"[lion] kahan: after {steps} steps p = {float(p[0]):.6f}, p + comp = {float(p[0].double() + comp[0].double()):.8f}, wanted {1.0 - steps * c['lr']:.8f}, "
          f"|error| {float(err.max()):.2e} within the summed bound {float(budget.max()):.2e}")


def _arena(dtype, seed, shapes):
    gen = torch.Generator().manual_seed(seed)
    n = sum(a * b for a, b in shapes)
    flat = (0.05 * torch.randn(n, generator=gen)).to(dtype).to(DEV)
    grad = torch.zeros(n, dtype=dtype, device=DEV)
    ps, off = [], 0
    for a, b in shapes:
        p = torch.nn.Parameter(flat[off:off + a * b].view(a, b))
        p.grad = grad[off:off + a * b].view(a, b)
        ps.append(p)
        off += a * b
    return flat, grad, ps


def _set_grads(grad, step):
    gen = torch.Generator().manual_seed(GOLD["seeds"]["optimizer"] + step)
    grad.copy_((1e-2 * torch.randn(grad.numel(), generator=gen)).to(grad.dtype))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_one_abi_call_per_step_whatever_the_number_of_tensors(ops, monkeypatch, dtype):
    from simpletuner_amd.training.optimizer import St355Lion
    calls = []
    real = ops.lion_step
    monkeypatch.setattr(ops, "lion_step", lambda *a, **k: (calls.append(a[0].numel()), real(*a, **k))[1])

    def run(nmat):
        flat, grad, ps = _arena(dtype, 3, [(32, 256), (256, 32)] * nmat)
        opt = St355Lion(ps, lr=1e-3, weight_decay=0.01)
        calls.clear()
        for s in range(1, 4):
            _set_grads(grad, s)
            opt.step()
        torch.cuda.synchronize()
        return flat.clone(), opt._flat[0]["m"].clone(), list(calls)

    a, b, c = run(3), run(3), run(40)
    assert torch.equal(LB.bits(a[0]), LB.bits(b[0])) and torch.equal(LB.bits(a[1]), LB.bits(b[1]))
    assert a[2] == [6 * 8192] * 3 and c[2] == [80 * 8192] * 3            # one call per step over the whole arena


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_resume_is_bit_exact(dtype):
    from simpletuner_amd.training.optimizer import St355Lion
    shapes = [(64, 64), (1, 1024)]
    make = lambda ps, lr=1e-3: St355Lion(ps, lr=lr, weight_decay=0.01)
    a_flat, a_grad, a_ps = _arena(dtype, 1, shapes)
    a = make(a_ps)
    for s in range(1, 5):
        _set_grads(a_grad, s)
        a.step()
    b_flat, b_grad, b_ps = _arena(dtype, 1, shapes)
    b = make(b_ps)
    for s in range(1, 3):
        _set_grads(b_grad, s)
        b.step()
    sd = b.state_dict()
    sd = {"state": {k: {n: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()},
          "param_groups": sd["param_groups"]}                  # as read back from a checkpoint file
    c_flat, c_grad, c_ps = _arena(dtype, 99, shapes)           # fresh objects, different init ...
    c_flat.copy_(b_flat)                                       # ... the model weights come from the checkpoint
    c = make(c_ps, lr=0.5)
    c.load_state_dict(sd)
    for s in range(3, 5):
        _set_grads(c_grad, s)
        c.step()
    assert torch.equal(LB.bits(c_flat), LB.bits(a_flat))
    fa, fc = a._flat[0], c._flat[0]
    assert fc["m"].dtype == dtype and torch.equal(LB.bits(fc["m"]), LB.bits(fa["m"]))
    if dtype == BF16:
        assert torch.equal(LB.bits(fc["comp"]), LB.bits(fa["comp"])) and bool(fa["comp"].any())
    else:
        assert fc["comp"] is None and all("kahan_comp" not in c.state[p] for p in c_ps)


# ---- trajectories through the trainer ---------------------------------------------------------------------------------------------------------------------
def _record(ops, monkeypatch):
    calls = []
    real = ops.lion_step

    def rec(p, g, m, lr, beta1=0.9, beta2=0.99, weight_decay=0.0, grad_scale=1.0, comp=None, ema=None, ema_decay=0.0, p_bf16=None):
        cl = lambda t: None if t is None else t.clone()
        before = dict(p=cl(p), g=cl(g), m=cl(m), comp=cl(comp), ema=cl(ema))
        real(p, g, m, lr, beta1, beta2, weight_decay, grad_scale=grad_scale, comp=comp, ema=ema, ema_decay=ema_decay, p_bf16=p_bf16)
        calls.append(dict(before=before, hp=(lr, beta1, beta2, weight_decay, grad_scale, ema_decay), after=dict(p=cl(p), m=cl(m), comp=cl(comp), ema=cl(ema))))

    monkeypatch.setattr(ops, "lion_step", rec)
    return calls


def _check_chained(calls, what):
    for k, c in enumerate(calls):
        b, a = c["before"], c["after"]
        consts = LB.lion_consts(*c["hp"])
        reports, _ = LB.check_step(f"{what} step {k + 1}", consts, b["p"], b["g"], b["m"], a["p"], a["m"], b["comp"], a["comp"])
        LB.assert_reports(reports)
        if a["ema"] is not None:
            if a["ema"].dtype == BF16:
                LB.assert_reports([LB.check_bf16(f"{what} step {k + 1} ema", a["ema"], *LB.ema_bf16(b["ema"], a["p"], consts["omd"]), flat=True)])
            else:
                LB.assert_reports([LB.check_f32(f"{what} step {k + 1} ema", a["ema"], *LB.ema_f32(b["ema"], a["p"], consts["omd"]))])


def _sign_of(call):
    lr, b1, _, _, gs, _ = call["hp"]
    b = call["before"]
    return torch.sign(b["m"].to(F64) + (b["g"].to(F64) * LB.f32(gs) - b["m"].to(F64)) * (1.0 - LB.f32(b1)))


def _batch(devt):
    return {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}


def test_flux_lora_three_steps_chained(ops, monkeypatch):
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.training.optimizer import St355Lion
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU

    lr = 1e-3
    cfg = default_config(lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, optimizer="optimi-lion")
    acc = St355Accelerator(DEV)
    plugin = Flux(cfg, acc)
    plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    plugin.add_lora_adapter()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Lion)
    cpu, devt = PU.make_inputs(1, 16, 16, 64, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    model = plugin.get_trained_component()
    P, lora, scale = PU.oracle_state(model)
    ocfg = PU.oracle_cfg(model)
    names = list(lora)
    calls = _record(ops, monkeypatch)
    # the fp32 oracle's own Lion trajectory (fp64 moments): only the share of differing signs is taken from it
    mom = {k: (torch.zeros_like(a, dtype=F64), torch.zeros_like(b, dtype=F64)) for k, (a, b) in lora.items()}
    osign = []
    for _ in range(3):
        trainer.train_step(_batch(devt))
        _, _, grads = PU.oracle_step(P, ocfg, lora, scale, cpu)
        step_sign, new_lora, new_mom = {}, {}, {}
        for k in names:
            outs = []
            for t, gr, m0 in zip(lora[k], grads[k], mom[k]):
                cc = m0 + (gr.to(F64) - m0) * (1.0 - LB.f32(0.9))
                outs.append(((t.detach().to(F64) - LB.f32(lr) * torch.sign(cc)).float(), m0 + (gr.to(F64) - m0) * (1.0 - LB.f32(0.99)), torch.sign(cc)))
            new_lora[k] = (outs[0][0], outs[1][0])
            new_mom[k] = (outs[0][1], outs[1][1])
            step_sign[k] = (outs[0][2], outs[1][2])
        lora, mom = new_lora, new_mom
        osign.append(step_sign)
    torch.cuda.synchronize()
    assert len(calls) == 3 and all(c["before"]["p"].dtype == F32 and c["before"]["p"].numel() == model.lora_flat.numel() and c["before"]["comp"] is None for c in calls)
    _check_chained(calls, "flux lora")
    # the kernel's signs, laid out as the oracle's adapters (PU.oracle_state reads them from the same arena)
    keep = model.lora_flat.clone()
    shares = []
    with torch.no_grad():
        for call, want in zip(calls, osign):
            model.lora_flat.copy_(_sign_of(call).float())
            _, got, _ = PU.oracle_state(model)
            diff = sum(int((got[k][i].to(F64) != want[k][i]).sum()) for k in names for i in (0, 1))
            shares.append(diff / sum(want[k][i].numel() for k in names for i in (0, 1)))
        model.lora_flat.copy_(keep)
    print(f"[lion] flux lora: share of elements whose sign differs from the fp32 oracle's own Lion trajectory, steps 1-3: {[f'{s:.4f}' for s in shares]} (not asserted)")


def test_sd3_full_finetune_with_fused_ema_three_steps_chained(ops, monkeypatch):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.optimizer import St355Lion
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU

    cfg = default_config(model_family="sd3", model_type="full", train_batch_size=1, seed=5, learning_rate=1e-5, flow_schedule_shift=3.0, use_ema=True, ema_decay=0.99,
                         optimizer="optimi-lion", optimizer_config="weight_decay=0.01")
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(sample_size=32, num_layers=2, num_attention_heads=2, attention_head_dim=64, joint_attention_dim=128, caption_projection_dim=128,
                      pooled_projection_dim=64, pos_embed_max_size=24, qk_norm=None, dual_attention_layers=())
    plugin.enable_full_finetune()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Lion)
    cpu, devt = PU.make_inputs(1, 16, 16, 40, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    calls = _record(ops, monkeypatch)
    for _ in range(3):
        trainer.train_step(_batch(devt))
    torch.cuda.synchronize()
    n = sum(p.numel() for p in trainer.params)
    assert len(calls) == 3 and trainer.optimizer.ema_applied, "the EMA update did not ride in the optimizer launch"
    assert all(c["before"]["p"].dtype == BF16 and c["before"]["p"].numel() == n and c["before"]["comp"] is not None and c["before"]["ema"] is not None and c["hp"][3] == 0.01
               for c in calls), "one launch over the bf16 arena with the compensation buffer and the EMA shadow"
    assert trainer.ema_model.optimization_step == 3
    _check_chained(calls, "sd3 full")
    assert bool(calls[-1]["after"]["comp"].any())


def test_captured_step_equals_eager_step_bit_for_bit():
    """one hip_graph=True step (predict + loss + backward replayed from a hipGraph, the optimizer outside the capture) against the eager step"""
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU

    def run(graph):
        torch.manual_seed(0)
        cfg = default_config(lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=1e-3, optimizer="optimi-lion", hip_graph=graph)
        acc = St355Accelerator(DEV)
        plugin = Flux(cfg, acc)
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
        plugin.add_lora_adapter()
        trainer = Trainer(cfg, plugin, acc)
        _, devt = PU.make_inputs(1, 16, 16, 64, 128, 64, DEV, seed=5)
        sig = devt["sigmas"]
        plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
        loss = trainer.train_step(_batch(devt))
        torch.cuda.synchronize()
        return loss.clone(), plugin.get_trained_component().lora_flat.clone(), trainer.optimizer._flat[0]["m"].clone()

    eager, graph = run(False), run(True)
    for a, b, what in zip(eager, graph, ("loss", "adapters", "momentum")):
        assert torch.equal(LB.bits(a.float()), LB.bits(b.float())), f"captured step: {what} differs from the eager step"

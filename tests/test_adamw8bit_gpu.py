"""8-bit block-wise AdamW on the MI355X (simpletuner_amd/csrc/adamw8bit.hip): three chained steps over a five-tensor arena with every kind of segment, each step
held element-wise to the fp64 restatement stepping from the kernel's OWN stored state (tests/adamw8bit_ref.py: parameters, block scales, dequantised codes, plain
moments), guards intact, bit-identical run to run, one refusal; and the optimizer through SD3 LoRA and SD3 full fine-tune train steps.

Measured worst |err| / bound over all cases (MI355X): see the figures the test prints per step."""
import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.lib import St355Error
from tests import adamw8bit_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
SIZES = (4096, 3072, 4104, 8192, 64)          # eligible (16 blocks) | plain, below 4096 | plain, not a multiple of 256 | eligible | plain
GUARD = 64                                    # sentinel elements on both sides of every buffer
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-6)
STATE = ("m_codes", "v_codes", "m_scale", "v_scale", "m_plain", "v_plain")
_INPUTS = {}


def _inputs(dtype):
    """p0 and three gradients, made once per dtype and never modified: seeded normal; block 3 of tensor 0 has an all-zero gradient in every step (its scales fall to
    the 1e-12 floor); block 5 of tensor 3 holds one element 1e4 times the rest"""
    if dtype not in _INPUTS:
        gen = torch.Generator().manual_seed(8)
        n = sum(SIZES)
        p0 = (0.05 * torch.randn(n, generator=gen)).to(dtype)
        gs = []
        for _ in range(3):
            g = 0.01 * torch.randn(n, generator=gen)
            g[3 * 256:4 * 256] = 0
            g[sum(SIZES[:3]) + 5 * 256 + 17] = 100.0
            gs.append(g.to(dtype))
        _INPUTS[dtype] = (p0, gs)
    return _INPUTS[dtype]


def _guarded(n, dtype, fill):
    full = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device=DEV)
    full[GUARD:GUARD + n] = fill
    return full, full[GUARD:GUARD + n]


def _fresh(dtype):
    plan = ops.Adamw8bitPlan([sum(SIZES[:i]) for i in range(len(SIZES))], list(SIZES), DEV)
    p0, _ = _inputs(dtype)
    bufs = {"p": _guarded(plan.end, dtype, 0), "g": _guarded(plan.end, dtype, 0), "m_codes": _guarded(plan.n_codes, torch.uint8, 127),
            "v_codes": _guarded(plan.n_codes, torch.uint8, 0), "m_scale": _guarded(plan.n_scales, F32, 0), "v_scale": _guarded(plan.n_scales, F32, 0),
            "m_plain": _guarded(plan.n_plain, F32, 0), "v_plain": _guarded(plan.n_plain, F32, 0)}
    bufs["p"][1].copy_(p0)
    return plan, bufs


def _launch(plan, bufs, books, step, wd, gs):
    ops.adamw8bit_step(plan, bufs["p"][1], bufs["g"][1], *[bufs[k][1] for k in STATE], books, step, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, gs)


def _host(bufs):
    return {k: v[1].cpu().clone() for k, v in bufs.items()}


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
def test_three_steps_bounded_against_the_restatement_from_stored_state(dtype, wd, gs):
    plan, bufs = _fresh(dtype)
    books = ops.adamw8bit_books().to(DEV)
    cbs = R.codebooks()
    bf = dtype == torch.bfloat16
    worst = {}

    def hold(name, err, tol):
        r = float((err / tol.clamp_min(1e-300)).max())
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, f"{name}: worst |err| / bound = {r:.3f}"

    for step in (1, 2, 3):
        bufs["g"][1].copy_(_inputs(dtype)[1][step - 1])
        before = _host(bufs)
        if step == 1:                                                    # an equal second launch from equal inputs: bit-identical
            plan2, twin = _fresh(dtype)
            twin["g"][1].copy_(bufs["g"][1])
            _launch(plan2, twin, books, step, wd, gs)
        _launch(plan, bufs, books, step, wd, gs)
        torch.cuda.synchronize()
        after = _host(bufs)
        if step == 1:
            assert all(torch.equal(bufs[k][0].view(torch.uint8), twin[k][0].view(torch.uint8)) for k in bufs), "two launches from equal inputs differ"
        for k, (full, view) in bufs.items():                             # guards on both sides of every buffer
            assert bool((full[:GUARD] == 77).all()) and bool((full[GUARD + view.numel():] == 77).all()), f"step {step}: guard of {k} overwritten"
        c = R.consts(HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, step, gs)
        for off, n, kind, co, so, po in zip(plan.host.view(-1, 8)[:, 0].tolist(), SIZES, plan.kinds, plan.code_offsets, plan.scale_offsets, plan.state_offsets):
            sl, nb = slice(off, off + n), n // 256
            if kind == plan.QUANT:
                m0 = R.dequantise(cbs[0], before["m_codes"][co:co + n], before["m_scale"][so:so + nb])
                v0 = R.dequantise(cbs[1], before["v_codes"][co:co + n], before["v_scale"][so:so + nb])
            else:
                m0, v0 = before["m_plain"][po:po + n], before["v_plain"][po:po + n]
            ref = R.step(before["p"][sl], before["g"][sl], m0, v0, c, kind == plan.QUANT)
            want, e = ref["p"]
            hold("p", (after["p"][sl].to(F64) - want).abs(), R.p_tol(want, e, bf))
            for key, cb in (("m", cbs[0]), ("v", cbs[1])):
                want, e = ref[key]
                if kind == plan.QUANT:
                    s_ref, e_s, tol = R.code_bound(cb, want, e)
                    s_out = after[f"{key}_scale"][so:so + nb].to(F64)
                    hold(f"{key} scale", (s_out - s_ref).abs(), e_s)
                    hold(f"{key} code", (R.dequantise(cb, after[f"{key}_codes"][co:co + n], s_out) - want).abs(), tol)
                else:
                    hold(f"{key} plain", (after[f"{key}_plain"][po:po + n].to(F64) - want).abs(), e)
        assert not torch.equal(after["p"], before["p"]) and not torch.equal(after["m_codes"], before["m_codes"]), "the step moved nothing"
        if step == 1:
            assert float(after["m_scale"][3]) == float(after["v_scale"][3]) == R.FLOOR                      # the all-zero block sits on the floor
            assert bool((after["v_codes"][4096 + 5 * 256:4096 + 6 * 256] == 0).sum() >= 250)              # the dynamic-range block: v far below the block maximum quantises to 0
    print(f"[adamw8bit] {dtype} wd={wd} gs={gs}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_a_short_code_buffer_is_refused_before_any_launch():
    plan, bufs = _fresh(F32)
    bufs["g"][1].copy_(_inputs(F32)[1][0])
    before = bufs["p"][0].clone()
    args = [bufs[k][1] for k in STATE]
    args[0] = args[0][:-1]
    with pytest.raises(St355Error, match="m_codes must be a contiguous"):
        ops.adamw8bit_step(plan, bufs["p"][1], bufs["g"][1], *args, ops.adamw8bit_books().to(DEV), 1, 1e-2)
    torch.cuda.synchronize()
    assert torch.equal(bufs["p"][0], before)


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_sd3_trains_through_the_trainer(mode):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.optimizer import St355AdamW8bit
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    from tests.test_sd3_model_gpu import _arch
    extra = dict(lora_rank=16, lora_init_b_std=0.0, learning_rate=1e-3) if mode == "lora" else dict(model_type="full", train_batch_size=1, learning_rate=1e-4)
    cfg = default_config(model_family="sd3", seed=5, flow_schedule_shift=3.0, optimizer="ao-adamw8bit", **extra)
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(2))
    plugin.add_lora_adapter() if mode == "lora" else plugin.enable_full_finetune()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355AdamW8bit) and trainer.optimizer.defaults["eps"] == 1e-6
    _, devt = PU.make_inputs(1, 16, 16, 24, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    losses = [float(trainer.train_step(dict(batch))) for _ in range(5)]
    st = trainer.optimizer._flat[0]
    print(f"[adamw8bit] sd3 {mode}: losses {losses}; {st['plan'].n_codes} quantised and {st['plan'].n_plain} plain elements in {st['plan'].n} tensors")
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0], losses
    assert trainer.optimizer.abi_calls == 5 and st["step"] == 5
    if mode == "full":
        assert st["plan"].n_codes > 0 and st["plan"].n_plain > 0 and st["m_codes"].dtype == torch.uint8

"""Diff2Flow on the device: st355_diff2flow_loss inside its derived bounds (tests/diff2flow_bounds.py) and bit-identical across launches, against the CPU stand-in
op by op, the tiny SDXL LoRA step against the oracle, and the captured step (hip_graph) against the eager one."""
import pytest
import torch

from tests import diff2flow_bounds as DB
from tests import diff2flow_ref as DR

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda:0"
CASES = [(name, None, None) for name in DR.SHAPES] + [("b1", (1, 4, 8, 8), [500]), ("ends", (2, 4, 8, 8), [0, 999]), ("clamp", (2, 4, 8, 8), [1000, 7])]


def _run(o, mode, kind_mask, weight, want_grad, grad_scale=1.0):
    from simpletuner_amd import ops
    d = lambda t: None if t is None else t.to(DEV)
    wide = o.wide[mode].to(DEV)
    pred = wide[:, :wide.shape[1] // 2]
    pred = pred if o.strided else pred.contiguous()
    table = DR.pair_table(o.tables, mode, F32).to(DEV)
    args = (pred, d(o.noisy), d(o.tau), d(o.timesteps), table, mode)
    kw = dict(weight=d(weight), want_grad=want_grad, grad_scale=grad_scale, emask=d(kind_mask))
    a = ops.diff2flow_loss(*args, **kw)
    b = ops.diff2flow_loss(*args, **kw)
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_inside_the_bounds_and_bit_identical(case, mode):
    name, shape, ts = case
    for kind, with_weight, want_grad in ((None, False, True), ("mask", True, True), ("segmentation", False, True), ("mask", False, False)):
        o = DR.operands(name if shape is None else "small", seed=11, timesteps=ts, mask_kind=kind, with_weight=with_weight, shape=shape)
        a, b = _run(o, mode, o.emask, o.weight, want_grad, grad_scale=0.5)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)                                   # two launches, the same bits
        pred = DR.pred_of(o, mode)
        table = DR.pair_table(o.tables, mode, F32)
        ref = DB.loss_ref(pred, o.noisy, o.tau, o.timesteps, table, mode, emask=o.emask, weight=o.weight, grad_scale=0.5)
        outs = {"loss": a[0], "per_sample": a[1]}
        if want_grad:
            outs["dpred"] = a[2]
            assert a[2].dtype == BF16 and a[2].is_contiguous() and a[2].shape == pred.shape
        else:
            assert a[2] is None
        for nm, got in outs.items():
            ok, worst = DB.inside(got, *ref[nm])
            print(f"[diff2flow kernel] {name} {mode} mask={kind} weight={with_weight} {nm}: worst |err| / bound = {worst:.3f}")
            assert ok, (nm, worst)
        # op by op against the stand-in: both sit inside the bound around the same fp64 value, so they differ by at most two bounds
        s = DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, mode, weight=o.weight, want_grad=want_grad, grad_scale=0.5, emask=o.emask)
        for nm, got, want in zip(("loss", "per_sample", "dpred"), a, s):
            if got is not None:
                assert bool(((got.cpu().double() - want.double()).abs().reshape(ref[nm][1].shape) <= 2 * ref[nm][1]).all()), nm


def _layout(pred, which):
    """the same prediction values in a buffer that sends the kernel down one of its scalar fallbacks: a base 2 bytes off a 16-byte boundary (per-sample stride still
    a multiple of 8), or a per-sample stride that is no multiple of 8 (base aligned)"""
    B, N = pred.shape[0], pred[0].numel()
    if which == "misaligned_base":
        buf = torch.zeros(B * 2 * N + 8, dtype=BF16, device=pred.device)
        view = buf[1:1 + B * 2 * N].view(B, 2 * N)[:, :N].view(pred.shape)
        assert view.data_ptr() % 16 == 2 and view.stride(0) % 8 == 0
    else:
        buf = torch.zeros(B, 2 * N + 4, dtype=BF16, device=pred.device)
        view = buf[:, :N].view(pred.shape)
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 4
    view.copy_(pred)
    return view


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("fallback", ["mask_period", "misaligned_base", "odd_stride"])
def test_scalar_fallbacks_of_the_vector_path(fallback, mode):
    """per_sample % 8 == 0 but one of the other conditions of the 16-byte path fails: a mask period that is no multiple of 8 ([2, 4, 6, 6]: n = 144, period 36), a
    prediction base off a 16-byte boundary, a prediction stride that is no multiple of 8.  Same bounds, same bits across launches; the gradient comes
    back compact whatever the prediction's layout."""
    from simpletuner_amd import ops
    shape = (2, 4, 6, 6) if fallback == "mask_period" else (2, 4, 8, 8)
    o = DR.operands("small", seed=14, shape=shape, mask_kind="mask" if fallback == "mask_period" else None, with_weight=True)
    assert o.N % 8 == 0 and (fallback != "mask_period" or o.emask.shape[1] % 8 != 0)
    d = lambda t: None if t is None else t.to(DEV)
    table = DR.pair_table(o.tables, mode, F32)
    pred = DR.pred_of(o, mode)
    compact = pred.to(DEV).contiguous()
    dpred_in = compact if fallback == "mask_period" else _layout(compact, fallback)
    assert torch.equal(dpred_in, compact)
    run = lambda p: ops.diff2flow_loss(p, d(o.noisy), d(o.tau), d(o.timesteps), table.to(DEV), mode, weight=d(o.weight), emask=d(o.emask))
    a, b = run(dpred_in), run(dpred_in)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[2].is_contiguous() and a[2].shape == compact.shape
    ref = DB.loss_ref(pred, o.noisy, o.tau, o.timesteps, table, mode, emask=o.emask, weight=o.weight)
    for nm, got in zip(("loss", "per_sample", "dpred"), a):
        ok, worst = DB.inside(got, *ref[nm])
        assert ok, (nm, worst)


def test_out_of_range_timestep_clamps_to_the_last_entry():
    o = DR.operands("small", seed=12, timesteps=[1000, 7])
    o2 = DR.operands("small", seed=12, timesteps=[1000, 7])
    o2.timesteps = torch.tensor([999, 7])
    for mode in DR.MODES:
        a, _ = _run(o, mode, None, None, True)
        b, _ = _run(o2, mode, None, None, True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from simpletuner_amd import lib, ops
    o = DR.operands("small", seed=13)
    table = DR.pair_table(o.tables, "epsilon", F32).to(DEV)
    pred, noisy, tau, t = DR.pred_of(o, "epsilon").to(DEV), o.noisy.to(DEV), o.tau.to(DEV), o.timesteps.to(DEV)
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred.float(), noisy, tau, t, table)
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred, noisy, tau, t.int(), table)
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred, noisy[:1], tau, t, table)
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred, noisy, tau, t, table[:, :1].contiguous())
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred, noisy, tau, t, table, mode="sample")
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred, noisy, tau, t, table, emask=torch.ones(2, 7, device=DEV))
    with pytest.raises(lib.St355Error):
        ops.diff2flow_loss(pred.cpu(), noisy, tau, t, table)


def _trainer(graph, **over):
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_trainer_graph_gpu import SMALL
    dev = torch.device("cuda", 0)
    cfg = default_config(model_family="sdxl", model_type="lora", train_batch_size=2, learning_rate=1e-4, hip_graph=graph, lora_rank=16, lora_alpha=16.0,
                         lora_init_b_std=0.05, diff2flow_enabled=True, diff2flow_loss=True, **over)
    acc = St355Accelerator(dev)
    pl = SDXL(cfg, acc)
    pl.load_model(**SMALL)
    pl.add_lora_adapter()
    return pl, Trainer(cfg, pl, acc), SMALL


def _batch(i, dev):
    g = torch.Generator().manual_seed(20 + i)
    r = lambda *s: torch.randn(*s, generator=g).to(BF16).to(dev)
    return {"latent_batch": r(2, 4, 16, 16), "prompt_embeds": r(2, 9, 128), "add_text_embeds": r(2, 64),
            "batch_time_ids": torch.tensor([[128., 128, 0, 0, 128, 128]] * 2, device=dev, dtype=BF16), "timesteps": torch.tensor([100 + 400 * i, 999 - 300 * i]),
            "noise": r(2, 4, 16, 16)}


def test_tiny_sdxl_lora_step_matches_the_oracle():
    from oracle.unet import UNetConfig, unet_forward
    from tests.test_unet_host_sequencing_cpu import _rel
    torch.manual_seed(0)
    pl, _, arch = _trainer(False)
    dev = pl.accelerator.device
    prepared = pl.prepare_batch(_batch(0, dev), {"global_step": 0})
    out = pl.model_predict(prepared)
    loss = pl.loss(prepared, out)
    loss.backward()
    torch.cuda.synchronize()
    m = pl.model
    P = {k: v.float().cpu() for k, v in m.diffusers_state_dict().items()}
    lora = {n: p.detach().float().cpu().requires_grad_(True) for n, p in m.named_parameters() if ".lora_" in n}
    Pe = dict(P)
    for n in lora:
        if ".lora_A." in n:
            base = n.replace(".lora_A.default.weight", "")
            Pe[base + ".weight"] = P[base + ".weight"] + lora[base + ".lora_B.default.weight"] @ lora[n]              # alpha / rank = 1
    c = lambda t: t.float().cpu()
    ack = prepared["added_cond_kwargs"]
    ref = unet_forward(Pe, UNetConfig(**arch), c(prepared["noisy_latents"]), c(prepared["timesteps"]), c(prepared["encoder_hidden_states"]),
                       {"text_embeds": c(ack["text_embeds"]), "time_ids": c(ack["time_ids"])})
    assert _rel(out["model_prediction"].detach().cpu(), ref.detach()) < 2e-2
    table = pl.diff2flow_value().table("epsilon").cpu()
    flat = lambda t: t.double().cpu().reshape(2, -1)
    lref = DR.loss64(flat(ref), flat(prepared["noisy_latents"]), flat(prepared["flow_target"]), prepared["timesteps"].cpu(), table, "epsilon")[0]
    lref.backward()
    print(f"[diff2flow sdxl step] loss hip {loss.detach().item():.6f} oracle {float(lref):.6f}")
    assert abs(loss.detach().item() - float(lref)) < 2e-3 * max(1.0, abs(float(lref)))
    worst = (0.0, "")
    for n, p in m.named_parameters():
        if ".lora_" in n:
            r = _rel(p.grad.cpu(), lora[n].grad)
            worst = max(worst, (r, n))
            assert r < 6e-2, (n, r)
    print(f"[diff2flow sdxl step] worst adapter gradient rel_l2 {worst[0]:.3e} at {worst[1]}")


def test_captured_step_replays_equal_the_eager_calls():
    """two replays of the captured tiny SDXL step on two different batches (timesteps included: the coefficient pair is gathered on the device) equal the two
    eager steps on the same batches"""
    def run(graph):
        torch.manual_seed(0)
        pl, tr, _ = _trainer(graph)
        dev = pl.accelerator.device
        return [float(tr.train_step(_batch(i, dev))) for i in range(3)]
    eager, graph = run(False), run(True)
    print(f"[diff2flow graph] eager {eager}\n                  graph {graph}")
    assert all(abs(a - b) <= 2e-3 * max(1.0, abs(a)) for a, b in zip(eager, graph)), (eager, graph)
    assert len(set(eager)) == 3

"""T-LoRA on the MI355X: the mask kernel of simpletuner_amd/csrc/tlora.hip through the C ABI against the dense restatement (bit for bit, guards and padding columns
intact, two launches identical, every refused precondition), the stand-in against the kernel op by op, the tiny SD3 step against fp64 autograd through the oracle
with the explicit per-sample mask, and the captured step (hip_graph) replayed with other timesteps in its static input against the eager steps."""
import pytest
import torch

from simpletuner_amd import lib as L
from simpletuner_amd import ops
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests import tlora_ref as TR
from tests.test_tlora_cpu import BOTH, LYCORIS, R, T_TRAIN, _inputs3, _oracle, _perturb, _ranks, _worst

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
TS_KIND = {F32: 0, BF16: 1, torch.int64: 2}


def _abi(view, r_pad, rank, G, rows_per_sample, table, ts, over=None):
    """st355_tlora_mask itself: the arguments ops.tlora_mask would pass, `over` replacing some; returns the C return code"""
    M, _, ld, seg, seg_s = ops._seg(view, "t")
    a = dict(t=view.data_ptr(), ld=ld, seg=seg, seg_s=seg_s, M=M, rps=rows_per_sample, G=G, r_pad=r_pad, rank=rank, ts=ts.data_ptr(), kind=TS_KIND[ts.dtype],
             B=ts.numel(), table=table.data_ptr(), T=table.numel() - 1)
    a.update(over or {})
    return L.load().st355_tlora_mask(torch.cuda.current_stream().cuda_stream, a["t"], a["ld"], a["seg"], a["seg_s"], a["M"], a["rps"], a["G"], a["r_pad"], a["rank"],
                                     a["ts"], a["kind"], a["B"], a["table"], a["T"])


def _abi_mask(view, r_pad, rank, G, rows_per_sample, table, ts):
    assert _abi(view, r_pad, rank, G, rows_per_sample, table, ts) == 0
    return view


# ------------------------------------------------------------------------------------------------
# (8) the kernel through the C ABI
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", TR.MASK_LAYOUTS)
@pytest.mark.parametrize("G,rank", TR.MASK_SHAPES)
def test_the_kernel_equals_the_dense_restatement_bit_for_bit_and_repeats(G, rank, layout):
    """check_mask_case holds the WHOLE buffer to the restatement: the dead columns are +0; survivors, the padding columns [rank, r_pad) and [G r_pad, K2), the guards in
    front and behind, and (view) the joint buffer's other rows are bit for bit what they were"""
    dead = 0
    for rows in TR.MASK_ROWS:
        for ts in TR.MASK_TIMESTEPS:
            for dt in TR.MASK_DTYPES:
                first, n = TR.check_mask_case(_abi_mask, DEV, layout, rows, G, rank, ts, dt, seed=rows + G)
                second, _ = TR.check_mask_case(_abi_mask, DEV, layout, rows, G, rank, ts, dt, seed=rows + G)
                assert torch.equal(TR.bits(first), TR.bits(second))
                dead += n
    assert dead > 0


def test_a_second_launch_on_the_masked_operand_changes_nothing_and_int64_timesteps_read_the_same_table():
    G, rank, rows = 3, 33, 77
    r_pad = TR.r_pad_of(rank)
    table = TR.rank_table(1000, rank, 1, 1.0).to(DEV)
    whole, view = TR.mask_operand("view", rows, G, rank, DEV, seed=9)
    ts = torch.tensor([250, -4, 70000], dtype=torch.int64, device=DEV)          # (outside [0, T]: the table's ends)
    before = whole.cpu().clone()
    _abi_mask(view, r_pad, rank, G, rows, table, ts)
    once = whole.cpu().clone()
    _abi_mask(view, r_pad, rank, G, rows, table, ts)
    assert torch.equal(TR.bits(whole.cpu()), TR.bits(once)) and not torch.equal(TR.bits(once), TR.bits(before))
    want = before.clone()
    K2 = view.shape[-1]
    TR._operand_view(want, "view", rows, K2).copy_(TR.restate(TR._operand_view(before, "view", rows, K2), r_pad, rank, G, rows, table.cpu(), ts.cpu()))
    assert torch.equal(TR.bits(once), TR.bits(want))
    # NaN and infinities read the table's ends as well
    whole2, view2 = TR.mask_operand("compact", rows, G, rank, DEV, seed=9)
    odd = torch.tensor([float("nan"), float("inf"), float("-inf")], device=DEV)
    b2 = whole2.cpu().clone()
    _abi_mask(view2, r_pad, rank, G, rows, table, odd)
    want2 = b2.clone()
    TR._operand_view(want2, "compact", rows, K2).copy_(TR.restate(TR._operand_view(b2, "compact", rows, K2), r_pad, rank, G, rows, table.cpu(),
                                                                  torch.tensor([0.0, 1000.0, 0.0])))
    assert torch.equal(TR.bits(whole2.cpu()), TR.bits(want2))


REFUSED = [
    (dict(r_pad=48), "r_pad must be 32 or a multiple of 64"),
    (dict(r_pad=96), "r_pad must be 32 or a multiple of 64"),
    (dict(G=5), "1 .. 4 targets"),
    (dict(G=0), "1 .. 4 targets"),
    (dict(rank=0), "rank 0 outside 1 .. r_pad"),
    (dict(rank=33), "rank 33 outside 1 .. r_pad"),
    (dict(ld=36), "16-byte aligned rows"),
    (dict(ld=24), "16-byte aligned rows"),
    (dict(t="odd"), "16-byte aligned rows"),
    (dict(M=11), "must equal timesteps"),
    (dict(rps=4), "must equal timesteps"),
    (dict(seg=4), "seg_rows must divide M"),
    (dict(kind=7), "timesteps must be fp32, bf16 or int64"),
    (dict(T=0), "the table holds T \\+ 1 entries"),
    (dict(table=0), "null pointer"),
    (dict(ts=0), "null pointer"),
]


@pytest.mark.parametrize("over,pat", REFUSED, ids=[f"{next(iter(o))}{i}" for i, (o, _) in enumerate(REFUSED)])
def test_every_refused_precondition_returns_its_error_and_launches_nothing(over, pat):
    import re
    G, rank, rows = 1, 4, 5
    table = TR.rank_table(1000, rank, 1, 1.0).to(DEV)
    whole, view = TR.mask_operand("compact", rows, G, rank, DEV, seed=1)
    ts = torch.tensor([900.0, 900.0, 900.0], device=DEV)
    before = whole.cpu().clone()
    if over.get("t") == "odd":
        over = dict(over, t=view.data_ptr() + 2)
    if "seg" in over:
        over = dict(over, seg_s=over["seg"])
    rc = _abi(view, 32, rank, G, rows, table, ts, over)
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.load().st355_last_error().decode()
    assert msg.startswith("tlora_mask:") and re.search(pat, msg), msg
    assert torch.equal(TR.bits(whole.cpu()), TR.bits(before))
    assert _abi(view, 32, rank, G, rows, table, ts) == 0          # (the same call without the bad argument runs)


def test_the_wrapper_refuses_what_the_abi_cannot_be_given():
    table = TR.rank_table(1000, 4, 1, 1.0).to(DEV)
    _, view = TR.mask_operand("compact", 5, 1, 4, DEV)
    ts = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    with pytest.raises(L.St355Error, match="timesteps must be a contiguous"):
        ops.tlora_mask(view, 32, 4, 1, 5, table, ts.to(torch.float64))
    with pytest.raises(L.St355Error, match="do not fit the operand"):
        ops.tlora_mask(view, 64, 4, 2, 5, table, ts)
    with pytest.raises(L.St355Error, match="tlora_mask: M"):
        ops.tlora_mask(view, 32, 4, 1, 4, table, ts)


# ------------------------------------------------------------------------------------------------
# (9) the stand-in against the kernel, op by op
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", TR.MASK_LAYOUTS)
@pytest.mark.parametrize("G,rank", TR.MASK_SHAPES)
def test_the_stand_in_against_the_kernel_op_by_op(G, rank, layout):
    for rows in TR.MASK_ROWS:
        for ts in TR.MASK_TIMESTEPS:
            for dt in TR.MASK_DTYPES:
                dev, _ = TR.check_mask_case(ops.tlora_mask, DEV, layout, rows, G, rank, ts, dt, seed=3)
                emu, _ = TR.check_mask_case(TR.tlora_mask, "cpu", layout, rows, G, rank, ts, dt, seed=3)
                assert torch.equal(TR.bits(dev), TR.bits(emu))


# ------------------------------------------------------------------------------------------------
# (10) the tiny SD3 step
# ------------------------------------------------------------------------------------------------
def _gpu_model(layers, sd35, classes, seed=11):
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device=DEV, **SH._arch(layers, **(dict(qk_norm="rms_norm", dual=(0, 1)) if sd35 else {})))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".norm_q." in name or ".norm_k." in name or ".norm_added_" in name:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = model.config
        model.pos_embed.pos_embed.copy_(T.sincos_2d(model.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])
    model.add_tlora_adapter(classes=classes, linear_dim=R, linear_alpha=R, multiplier=1, min_rank=1, alpha=1.0, num_train_timesteps=T_TRAIN, seed=7)
    model.prepare_for_training()
    model.train()
    _perturb(model)
    return model


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "per-block"])
@pytest.mark.parametrize("classes", [["Attention"], ["FeedForward"], BOTH], ids=["attention", "feed-forward", "both"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_the_tiny_sd3_step_matches_the_masked_oracle(monkeypatch, sd35, classes, ckpt):
    """the tolerances of tests/test_lora_dropout_gpu.py::test_the_tiny_sd3_step_matches_the_masked_oracle (prediction rel-L2 2e-2, loss 2e-3, gradients rel-L2 5e-2, a
    reference without the mask above 0.25)"""
    model = _gpu_model(3, sd35, classes)
    model.gradient_checkpointing = ckpt
    d = _inputs3()
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, loss = SH._hip_side(model, dd)
    ranks = _ranks(model, d["t"])
    assert ranks == [14, 8, 2]
    o_out, o_loss, facs = _oracle(monkeypatch, model, d, ranks)
    assert PU.rel_l2(out.cpu(), o_out.float()) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, facs)
    assert worst < 5e-2, worst
    _, _, nfacs = _oracle(monkeypatch, model, d, None)
    plain = _worst(model, nfacs)
    assert plain > 0.25, plain
    print(f"[gpu] sd3{'.5' if sd35 else ''} T-LoRA {classes}: worst adapter gradient rel-L2 {worst:.3e} with the mask, {plain:.3e} against a reference without it")


def test_inactive_ranks_get_exactly_zero_gradient_on_the_device():
    model = _gpu_model(3, True, BOTH)
    d = SH._inputs(1, 16, 24, 33)
    d["t"] = torch.tensor([999.0])
    SH._hip_side(model, {k: v.to(DEV) for k, v in d.items()})
    dead = "transformer_blocks.2.attn.add_q_proj."
    for n, p in model.named_parameters():
        if n.endswith(TR.DOWN):
            assert bool((p.grad[1:] == 0).all()) and (n.startswith(dead) or float(p.grad[0].abs().max()) > 0), n
        if n.endswith(TR.UP):
            assert bool((p.grad[:, 1:] == 0).all()) and (n.startswith(dead) or float(p.grad[:, 0].abs().max()) > 0), n


# ------------------------------------------------------------------------------------------------
# (11) the captured step
# ------------------------------------------------------------------------------------------------
def _trainer(graph: bool, lr: float):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family="sd3", lora_rank=8, seed=5, learning_rate=lr, train_batch_size=2, hip_graph=graph)
    cfg.lora_type, cfg.lycoris_config = "lycoris", dict(LYCORIS, tlora_min_rank=1)
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    _perturb(plugin.get_trained_component())
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    cur = {}
    plugin.sample_flow_sigmas = lambda batch, state: (cur["t"] / 1000.0, cur["t"])
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}

    def step(ts):
        cur["t"] = torch.tensor(ts, dtype=F32, device=DEV)
        return trainer.train_step(dict(batch)).item()
    return plugin, step


@pytest.mark.parametrize("lr", [0.0, 1e-3])
def test_two_replays_of_the_captured_step_follow_the_timesteps_in_the_static_input_and_equal_the_eager_steps(lr):
    """captured once (two eager warm-up passes, then the capture, all at the first batch's timesteps), replayed with timesteps [10, 900], then [900, 10] copied into the
    static input: the mask kernel gathers its ranks from the device, so each replay is the eager step at those timesteps bit for bit.  lr = 0: the weights stand
    still, so the two replays differ by their masks (and the swapped noise levels) alone."""
    pg, gstep = _trainer(True, lr)
    g1, g2 = gstep([10.0, 900.0]), gstep([900.0, 10.0])
    torch.cuda.synchronize()
    pe, estep = _trainer(False, lr)
    e1, e2 = estep([10.0, 900.0]), estep([900.0, 10.0])
    assert g1 != g2 and (g1, g2) == (e1, e2)
    assert torch.equal(pg.get_trained_component().lora_flat, pe.get_trained_component().lora_flat)

"""LoRA dropout on the MI355X: the kernels of simpletuner_amd/csrc/lora_dropout.hip against the CPU restatement of the mask (bit for bit) and the fp64 references
(element-wise, inside the derived bounds of tests/lora_dropout_bounds.py), their determinism, one mask for one logical problem whatever the operand's lay-out, the
stand-ins op by op, the SD3 step against autograd through the oracle with the masked linear, and the captured step (hip_graph) against the eager one."""
from types import SimpleNamespace

import pytest
import torch

from simpletuner_amd import ops
from tests import lora_dropout_ref as LD
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_lora_dropout_cpu import KERNEL_SHAPES, RANK, SEED, _compare, check_dx_two_roundings, check_kernels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
OPS = SimpleNamespace(**{k: getattr(ops, k) for k in LD.STAND_INS})
STAND = SimpleNamespace(**LD.STAND_INS)


@pytest.mark.parametrize("p,stream,call,M,K", [(0.1, 0, 1, 154, 192), (0.5, 9, 0xFFFFFFFF, 154, 192), (0.25, 3, 7, 5, 8)])
def test_the_exported_mask_is_the_restatement_bit_for_bit(p, stream, call, M, K):
    drop = LD.Drop(p, seed=(7 << 32) | 11, rank=3, calls=call, device=DEV)
    got = ops.lora_dropout_mask(M, K, drop, stream).cpu()
    want = LD.keep_mask(M, K, (drop.key0, drop.key1), call, stream, drop.thr).to(torch.uint8)
    assert torch.equal(got, want)
    ops.lora_dropout_advance(drop.call)
    assert drop.calls() == (call + 1) & 0xFFFFFFFF                      # the counter wraps as 32 unsigned bits
    assert torch.equal(ops.lora_dropout_mask(M, K, drop, stream).cpu(), LD.keep_mask(M, K, (drop.key0, drop.key1), call + 1, stream, drop.thr).to(torch.uint8))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rank", [4, 64, 128])
@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("kind,B,rows", KERNEL_SHAPES)
@pytest.mark.parametrize("K", [64, 192])
def test_kernels_are_inside_the_derived_bounds_and_repeat_bit_for_bit(K, kind, B, rows, G, rank, accumulate):
    first = check_kernels(OPS, DEV, kind, B, rows, K, G, rank, accumulate)
    second = check_kernels(OPS, DEV, kind, B, rows, K, G, rank, accumulate)
    assert torch.equal(first[0], second[0]) and all(torch.equal(a, b) for a, b in zip(first[1], second[1])) and torch.equal(first[2], second[2])


@pytest.mark.parametrize("G,rank", [(3, 4), (1, 64), (4, 128)])
def test_a_strided_view_and_its_compact_copy_draw_one_mask(G, rank):
    """the same logical [154, K] problem as the [2, 77, K] view of a joint buffer and as a compact tensor: the same bits from all three kernels"""
    a = check_kernels(OPS, DEV, "seg77", 2, 77, 192, G, rank, False, seed=3)
    b = check_kernels(OPS, DEV, "compact", 1, 154, 192, G, rank, False, seed=3)
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("G,rank", [(1, 4), (3, 4), (3, 64), (4, 128)])
def test_the_two_roundings_of_dx(G, rank):
    """the plain dx GEMM, then lora_dx_drop in place, against the fp64 product: both bf16 roundings bounded element-wise"""
    check_dx_two_roundings(SimpleNamespace(gemm=ops.gemm, lora_dx_drop=ops.lora_dx_drop), DEV, G, rank)


@pytest.mark.parametrize("G,rank", [(3, 4), (3, 64), (1, 128)])
@pytest.mark.parametrize("kind,B,rows", KERNEL_SHAPES)
def test_stand_ins_against_the_kernels_op_by_op(kind, B, rows, G, rank):
    """both sit inside the bounds around one fp64 reference (check_kernels asserts that), so they differ by at most two bounds; here: a bf16 output by at most two bf16
    steps of its magnitude, an fp32 one by 1e-4 of the largest entry"""
    dev = check_kernels(OPS, DEV, kind, B, rows, 192, G, rank, True, seed=5)
    emu = check_kernels(STAND, "cpu", kind, B, rows, 192, G, rank, True, seed=5)
    for a, b in ((dev[0], emu[0]), (dev[2], emu[2])):
        assert bool(((a.float() - b.float()).abs() <= 2 ** -6 * b.float().abs() + 1e-6).all())
    for a, b in zip(dev[1], emu[1]):
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()


def _gpu_model(layers, sd35, dropout, rank=16, calls=0, seed=11):
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
    model.add_lora_adapter(rank=rank, alpha=float(rank), init_b_std=0.02, dropout=dropout, dropout_seed=SEED, dropout_rank=RANK, dropout_calls=calls)
    model.prepare_for_training()
    model.train()
    return model


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "per-block"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_the_tiny_sd3_step_matches_the_masked_oracle(monkeypatch, sd35, ckpt):
    model = _gpu_model(3, sd35, 0.25, calls=4)
    model.gradient_checkpointing = ckpt
    d = SH._inputs(2, 16, 24, 33)
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, loss = SH._hip_side(model, dd)
    assert model.lora_dropout.calls() == 5
    worst, plain = _compare(monkeypatch, model, d, out.cpu(), loss.cpu(), 5)
    print(f"[gpu] sd3{'.5' if sd35 else ''} lora_dropout: worst adapter gradient rel-L2 {worst:.3e} with the mask, {plain:.3e} against a reference without it")


def _trainer(graph: bool, calls: int, lr: float):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family="sd3", lora_rank=8, seed=5, lora_init_b_std=0.02, learning_rate=lr, train_batch_size=2, hip_graph=graph)
    cfg.lora_dropout = 0.25
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    plugin.get_trained_component().lora_dropout.set_calls(calls)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


@pytest.mark.parametrize("lr", [0.0, 1e-3])
def test_two_replays_of_the_captured_step_draw_two_masks_and_equal_the_eager_calls(lr):
    """the capture's two eager warm-up passes advance the counter to 2, the replays use calls 3 and 4 (the advance is a launch inside the graph); the eager trainer
    started at 2 makes the same two calls.  lr = 0: the weights stand still, so the two replays of one batch differ by their masks alone."""
    pg, tg, batch = _trainer(True, 0, lr)
    g1 = tg.train_step(dict(batch)).item()
    g2 = tg.train_step(dict(batch)).item()
    torch.cuda.synchronize()
    assert pg.get_trained_component().lora_dropout.calls() == 4
    pe, te, batch_e = _trainer(False, 2, lr)
    e1 = te.train_step(dict(batch_e)).item()
    e2 = te.train_step(dict(batch_e)).item()
    assert g1 != g2 and (g1, g2) == (e1, e2)
    assert torch.equal(pg.get_trained_component().lora_flat, pe.get_trained_component().lora_flat)

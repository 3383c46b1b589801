"""LyCORIS LoKr on the MI355X: the kernels of simpletuner_amd/csrc/lokr.hip element-wise inside the derived bounds of tests/lokr_bounds.py (fp64 on the same bf16 /
fp32 operands), their determinism, guard elements and refused preconditions, the P GEMM route, the stand-ins of tests/lokr_ref.py op by op, the tiny SD3 step against
autograd through the oracle with the merged-weight linear, and the captured step (hip_graph) against the eager one."""
from types import SimpleNamespace

import pytest
import torch

from simpletuner_amd import lib, ops
from tests import lokr_bounds as LB
from tests import lokr_ref as LR
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.lokr_checks import ROWS, W1_SIDES, _guarded, check_dw1, check_dw2, check_fold, check_mix, run_fold

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
OPS = SimpleNamespace(**{k: getattr(ops, k) for k in LR.STAND_INS})
STAND = SimpleNamespace(**LR.STAND_INS)


# ------------------------------------------------------------------------------------------------
# fold
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ok,in_", [(8, 8), (24, 40), (64, 64), (24, 192)])          # 40 / 24: no multiple of the 64-column / 32-row tile
@pytest.mark.parametrize("ol,im", W1_SIDES)
def test_fold_is_inside_the_derived_bounds_and_repeats_bit_for_bit(ol, im, ok, in_, G):
    a = check_fold(OPS, DEV, ol, im, ok, in_, G)
    b = check_fold(OPS, DEV, ol, im, ok, in_, G)
    assert torch.equal(a.Wf[0], b.Wf[0]) and torch.equal(a.WfT[0], b.WfT[0])


@pytest.mark.parametrize("ol,im,ok,in_,G", [(8, 4, 24, 40, 3), (2, 2, 64, 64, 1)])
def test_fold_with_a_zero_scale_is_the_identity_and_rows_without_an_adapter_are_copied(ol, im, ok, in_, G):
    r = run_fold(OPS, DEV, ol, im, ok, in_, G, 0.0)
    assert torch.equal(r.Wf[0], r.W) and torch.equal(r.WfT[0], r.W.t())
    r = check_fold(OPS, DEV, ol, im, ok, in_, G, gap=40)
    assert torch.equal(r.Wf[0][G * r.N:], r.W[G * r.N:])


# ------------------------------------------------------------------------------------------------
# mix, dw2, dw1, P
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ok", [8, 24, 64])
@pytest.mark.parametrize("ol,im", W1_SIDES)
@pytest.mark.parametrize("kind,B,rows", ROWS)
def test_mix_is_inside_the_derived_bounds_and_repeats_bit_for_bit(kind, B, rows, ol, im, ok, G):
    assert torch.equal(check_mix(OPS, DEV, kind, B, rows, ol, im, ok, G), check_mix(OPS, DEV, kind, B, rows, ol, im, ok, G))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("in_", [8, 40, 64, 192])
@pytest.mark.parametrize("ok", [8, 24, 64])
@pytest.mark.parametrize("im", [2, 4, 16])
@pytest.mark.parametrize("kind,B,rows", ROWS)
def test_dw2_is_inside_the_derived_bounds_and_repeats_bit_for_bit(kind, B, rows, im, ok, in_, accumulate):
    assert torch.equal(check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, accumulate), check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, accumulate))


@pytest.mark.parametrize("im,ok,in_", [(2, 128, 128), (4, 256, 128), (4, 136, 192)])          # multiples of 128 on both sides: the 128 x 128 tile schedule; 136 / 192: 64 x 64 tiles, ragged
@pytest.mark.parametrize("kind,B,rows", ROWS)
def test_dw2_on_the_large_tile_schedule(kind, B, rows, im, ok, in_):
    assert torch.equal(check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, True), check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, True))
    check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, False)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ok", [8, 24, 64])
@pytest.mark.parametrize("ol,im", W1_SIDES)
@pytest.mark.parametrize("kind,B,rows", ROWS)
def test_dw1_is_inside_the_derived_bounds_and_repeats_bit_for_bit(kind, B, rows, ol, im, ok, G, accumulate):
    assert torch.equal(check_dw1(OPS, DEV, kind, B, rows, ol, im, ok, G, accumulate), check_dw1(OPS, DEV, kind, B, rows, ol, im, ok, G, accumulate))


@pytest.mark.parametrize("ol,im,ok,in_", [(2, 2, 8, 8), (8, 4, 24, 40), (16, 16, 64, 64)])
def test_a_view_and_its_compact_copy_give_equal_bits(ol, im, ok, in_):
    for fn in (lambda k: check_mix(OPS, DEV, k, 2, 64, ol, im, ok, 3, seed=4), lambda k: check_dw2(OPS, DEV, k, 2, 64, im, ok, in_, True, seed=4),
               lambda k: check_dw1(OPS, DEV, k, 2, 64, ol, im, ok, 3, True, seed=4)):
        assert torch.equal(fn("view"), fn("compact"))


@pytest.mark.parametrize("in_", [64, 192])
@pytest.mark.parametrize("ok", [8, 24, 64])
@pytest.mark.parametrize("im", [2, 4, 16])
@pytest.mark.parametrize("M", [37, 154])
def test_p_on_the_gemm_route_is_inside_the_derived_bound(M, im, ok, in_):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, im * in_, generator=g).to(BF16).to(DEV)
    w2b = (0.05 * torch.randn(ok, in_, generator=g)).to(BF16).to(DEV)
    P, tail = _guarded((M, im * ok), BF16, DEV)
    ops.gemm(x.view(M * im, in_), w2b, out=P.view(M * im, ok))
    ok_, worst = LB.inside(P, *LB.p_ref(x, w2b, im))
    assert ok_, worst
    assert bool((tail.float() == -7.0).all())


def test_every_kernel_refuses_a_shape_outside_its_preconditions_by_name():
    e = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(lib.St355Error, match="lokr_fold: the w1 sides must lie in 1 .. 16"):
        ops.lokr_fold(e(17 * 8, 64), [(0, 17 * 8, e(17, 1, dt=F32), e(8, 64, dt=F32), e(8, 64))], 1.0, e(17 * 8, 64), e(64, 17 * 8))
    with pytest.raises(lib.St355Error, match="lokr_fold: ok and in must be multiples of 8"):
        ops.lokr_fold(e(24, 64), [(0, 24, e(2, 1, dt=F32), e(12, 64, dt=F32), e(12, 64))], 1.0, e(24, 64), e(64, 24))
    with pytest.raises(lib.St355Error, match="lokr_mix: ok, n_off and the row stride must be multiples of 8"):
        ops.lokr_mix(e(16, 48), 0, e(2, 2, dt=F32), 12, e(16, 24))
    with pytest.raises(lib.St355Error, match="lokr_dw2: ok, in and the row stride of x must be multiples of 8"):
        ops.lokr_dw2(e(16, 24), e(16, 24), 2, e(12, 12, dt=F32))
    with pytest.raises(lib.St355Error, match="lokr_dw1: the w1 sides must lie in 1 .. 16"):
        ops.lokr_dw1(e(16, 17 * 8), 0, e(16, 16), e(17, 2, dt=F32), 8)


@pytest.mark.parametrize("ol,im,ok,in_,G", [(8, 4, 24, 40, 3), (16, 16, 64, 64, 1)])
def test_stand_ins_against_the_kernels_op_by_op(ol, im, ok, in_, G):
    """both sit inside the bounds around one fp64 reference (the checks assert that): a bf16 output differs by at most one bf16 step, an fp32 one by the two bounds"""
    dev, emu = check_fold(OPS, DEV, ol, im, ok, in_, G, seed=5), check_fold(STAND, "cpu", ol, im, ok, in_, G, seed=5)
    a, b = dev.Wf[0].cpu().float(), emu.Wf[0].float()
    assert bool(((a - b).abs() <= 2 ** -7 * b.abs() + 1e-30).all())
    for kind, B, rows in ROWS[1:]:
        a, b = check_mix(OPS, DEV, kind, B, rows, ol, im, ok, G, seed=6).cpu().float(), check_mix(STAND, "cpu", kind, B, rows, ol, im, ok, G, seed=6).float()
        assert bool(((a - b).abs() <= 2 ** -7 * b.abs() + 1e-30).all())
        a, b = check_dw2(OPS, DEV, kind, B, rows, im, ok, in_, True, seed=7), check_dw2(STAND, "cpu", kind, B, rows, im, ok, in_, True, seed=7)
        assert (a.cpu() - b).abs().max().item() <= 1e-5 * b.abs().max().item()
        a, b = check_dw1(OPS, DEV, kind, B, rows, ol, im, ok, G, True, seed=8), check_dw1(STAND, "cpu", kind, B, rows, ol, im, ok, G, True, seed=8)
        assert (a.cpu() - b).abs().max().item() <= 1e-5 * b.abs().max().item()


# ------------------------------------------------------------------------------------------------
# the tiny SD3 step
# ------------------------------------------------------------------------------------------------
def _gpu_model(sd35: bool, seed=11):
    """the small SD3 config of the host-sequencing tests with 2 layers (sd35: qk RMSNorm, the first a dual-attention block), LoKr on Attention + FeedForward"""
    from simpletuner_amd.sd3 import transformer as T
    from tests.test_lokr_cpu import FACTORS, _perturb
    model = T.SD3Transformer2DModel(device=DEV, **SH._arch(2, **(dict(qk_norm="rms_norm", dual=(0,)) if sd35 else {})))
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
    model.add_lokr_adapter(factors=dict(FACTORS))
    _perturb(model)
    model.prepare_for_training()
    model.train()
    return model


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "per-block"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_the_tiny_sd3_step_matches_the_merged_weight_oracle(monkeypatch, sd35, ckpt):
    """loss and every gradient against autograd through the oracle with the merged, rounded weight, at the tolerances of the SD3 LoRA step test
    (tests/test_sd3_model_gpu.py: prediction rel-L2 <= 2e-2, loss |delta| <= 1e-3, adapter gradients rel-L2 <= 5e-2 per matrix)"""
    from tests.test_lokr_cpu import _oracle, _ref_grad
    model = _gpu_model(sd35)
    model.gradient_checkpointing = ckpt
    d = SH._inputs(2, 16, 24, 33)
    out, loss = SH._hip_side(model, {k: v.to(DEV) for k, v in d.items()})
    cpu = SimpleNamespace(named_parameters=lambda: [(n, p.detach().cpu()) for n, p in model.named_parameters()], pos_embed=SimpleNamespace(pos_embed=model.pos_embed.pos_embed.cpu()),
                          config=model.config)
    o_out, o_loss, facs = _oracle(monkeypatch, cpu, d)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))
    n = 0
    for name, p in model.named_parameters():
        if ".lokr_" in name:
            n += 1
            assert PU.rel_l2(p.grad, _ref_grad(name, facs)) < 5e-2, name
    assert n == 2 * sum(len(g.targets) for g in model.lora_groups)


def test_at_fresh_init_the_output_is_bit_equal_to_the_base_model_host_sequenced(monkeypatch):
    from simpletuner_amd.sd3 import transformer as T
    d = {k: v.to(DEV) for k, v in SH._inputs(2, 16, 24, 33).items()}
    run = lambda m: m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()
    model = _gpu_model(True)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(LR.K2):
                p.zero_()
        a = run(model)
        monkeypatch.setattr(T, "_BLOCK_ABI", False)
        for blk in model.blocks:          # the same weights without the adapters
            for l in (blk.qkv, blk.add_qkv, blk.to_out, blk.to_add_out, blk.qkv2, blk.to_out2, blk.ff1, blk.ff2, blk.ffc1, blk.ffc2):
                if l is not None:
                    l.lora = None
        model.lora_groups, model.lora_lokr = [], False
        assert torch.equal(a, run(model))


def _trainer(graph: bool):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_lokr_cpu import LYCORIS, _perturb
    cfg = default_config(model_family="sd3", lora_rank=8, seed=5, learning_rate=1e-3, train_batch_size=2, hip_graph=graph)
    cfg.lora_type, cfg.lycoris_config = "lycoris", dict(LYCORIS)
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    _perturb(plugin.get_trained_component())
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, DEV, seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


def test_two_replays_of_the_captured_step_equal_two_eager_steps():
    pg, tg, batch = _trainer(True)
    g1 = tg.train_step(dict(batch)).item()
    g2 = tg.train_step(dict(batch)).item()
    torch.cuda.synchronize()
    pe, te, batch_e = _trainer(False)
    e1 = te.train_step(dict(batch_e)).item()
    e2 = te.train_step(dict(batch_e)).item()
    assert g1 != g2 and (g1, g2) == (e1, e2)
    assert torch.equal(pg.get_trained_component().lora_flat, pe.get_trained_component().lora_flat)

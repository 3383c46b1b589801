"""DoRA on the MI355X: the kernels of simpletuner_amd/csrc/dora.hip element-wise inside the derived bounds of tests/dora_bounds.py (fp64 on the same bf16 operands),
their determinism and guard elements, the stand-ins of tests/dora_ref.py op by op, the tiny SD3 step against autograd through the oracle with the DoRA linear, and
the captured step (hip_graph) against the eager one."""
from types import SimpleNamespace

import pytest
import torch

from simpletuner_amd import ops
from tests import dora_bounds as DB
from tests import dora_ref as DR
from tests import ops_emulator as EMU
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_dora_cpu import _oracle, _perturb, _ref_grad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
OPS = SimpleNamespace(lora_pack=ops.lora_pack, **{k: getattr(ops, k) for k in DR.STAND_INS})
STAND = SimpleNamespace(lora_pack=EMU.lora_pack, **DR.STAND_INS)
GUARD = 64


def _guarded(shape, dtype, dev, sentinel):
    """a contiguous tensor of `shape` at the head of a larger buffer whose tail holds a sentinel: (tensor, tail)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device=dev)
    return buf[:n].view(*shape), buf[n:]


def run_fold(fns, dev, N, K, G, rank, seed=0, zero_b=False, init=False):
    """G targets of N rows each over one input of K columns, packed by lora_pack as the engine does: returns the operands and every output (with its guard tail)"""
    g = torch.Generator().manual_seed(seed)
    r_pad = 32 if rank <= 32 else (rank + 63) // 64 * 64
    K2, Nt, s = (G * r_pad + 63) // 64 * 64, G * N, 2.0
    W = (torch.randn(Nt, K, generator=g) / K ** 0.5).to(BF16).to(dev)
    z = lambda *sh: torch.zeros(*sh, dtype=BF16, device=dev)
    A_cat, A_cat_T, B_blk, B_blk_T = z(K2, K), z(K, K2), z(Nt, K2), z(K2, Nt)
    for i in range(G):
        A = (torch.randn(rank, K, generator=g) / K ** 0.5).to(dev)
        Bm = (torch.zeros(N, rank) if zero_b else 0.2 * torch.randn(N, rank, generator=g)).to(dev)
        fns.lora_pack(A, Bm, s, A_cat, A_cat_T, B_blk, B_blk_T, k2_off=i * r_pad, n_off=i * N)
    m = (0.5 + torch.rand(Nt, generator=g)).to(dev)
    targets = [(i * N, N) for i in range(G)]
    outs = {"inv_norm": _guarded((Nt,), F32, dev, -7.0), "g": _guarded((Nt,), F32, dev, -7.0), "Wf": _guarded((Nt, K), BF16, dev, -7.0),
            "WfT": _guarded((K, Nt), BF16, dev, -7.0), "Bf": _guarded((Nt, K2), BF16, dev, -7.0), "BfT": _guarded((K2, Nt), BF16, dev, -7.0)}
    fns.dora_fold(W, A_cat_T, B_blk, m, targets, r_pad, *(outs[k][0] for k in ("inv_norm", "g", "Wf", "WfT", "Bf", "BfT")), init=init)
    return SimpleNamespace(W=W, A_cat_T=A_cat_T, B_blk=B_blk, m=m, targets=targets, r_pad=r_pad, outs=outs)


def check_fold(fns, dev, N, K, G, rank, seed=0):
    r = run_fold(fns, dev, N, K, G, rank, seed)
    ref = DB.fold_ref(r.W, r.A_cat_T, r.B_blk, r.m, r.targets, r.r_pad)
    for name in ("inv_norm", "g", "Wf", "Bf"):
        ok, worst = DB.inside(r.outs[name][0], *ref[name])
        print(f"[dora_fold N={N} K={K} G={G} rank={rank}] {name}: worst error / bound = {worst:.3f}")
        assert ok, (name, worst)
    assert torch.equal(r.outs["WfT"][0], r.outs["Wf"][0].t()) and torch.equal(r.outs["BfT"][0], r.outs["Bf"][0].t())          # bitwise the transposes
    for name, (t, tail) in r.outs.items():
        assert bool((tail.float() == -7.0).all()), f"{name}: guard elements written"
    return r


@pytest.mark.parametrize("rank", [4, 32, 128])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("K", [64, 200])          # 200: % 8 but no multiple of a 32- or 64-column chunk
@pytest.mark.parametrize("N", [64, 80])           # 80: the last 32-row tile of a target is half empty, and targets start off the tile grid
def test_fold_is_inside_the_derived_bounds_and_repeats_bit_for_bit(N, K, G, rank):
    a = check_fold(OPS, DEV, N, K, G, rank)
    b = check_fold(OPS, DEV, N, K, G, rank)
    for name in a.outs:
        assert torch.equal(a.outs[name][0], b.outs[name][0]), name


@pytest.mark.parametrize("N,K,G,rank", [(80, 200, 3, 4), (64, 64, 1, 128)])
def test_fold_at_init_gives_g_of_exactly_one_and_w_bitwise(N, K, G, rank):
    r = run_fold(OPS, DEV, N, K, G, rank, zero_b=True, init=True)
    assert torch.equal(r.outs["g"][0], torch.ones_like(r.outs["g"][0])) and torch.equal(r.outs["Wf"][0], r.W) and torch.equal(r.outs["Bf"][0], r.B_blk)
    ok, _ = DB.inside(r.m, *DB.fold_ref(r.W, r.A_cat_T, r.B_blk, r.m, r.targets, r.r_pad)["norm"])          # m = the norm
    assert ok
    # a second fold that READS the m the first one wrote: the norm repeats bit for bit, so g is still exactly 1
    g2 = torch.empty_like(r.m)
    e = lambda t: torch.empty_like(t)
    ops.dora_fold(r.W, r.A_cat_T, r.B_blk, r.m, r.targets, r.r_pad, e(r.m), g2, e(r.W), e(r.W.t().contiguous()), e(r.B_blk), e(r.B_blk.t().contiguous()))
    assert torch.equal(g2, torch.ones_like(g2))


def _dy_layout(kind, B, rows, N, dev, g):
    """dy over B * rows logical rows: as a compact [B * rows, N] tensor, or as the [B, rows, N] view of a taller joint buffer [B, rows + 9, N + 16]; returns
    (operand, logical rows)"""
    vals = torch.randn(B * rows, N, generator=g).to(BF16)
    if kind == "compact":
        t = vals.to(dev)
        return t, t
    joint = torch.full((B, rows + 9, N + 16), 3.0, dtype=BF16, device=dev)
    view = joint[:, 4:4 + rows, 8:8 + N]
    view.copy_(vals.view(B, rows, N).to(dev))
    return view, vals.to(dev)


def check_dmag(fns, dev, kind, B, rows, N, accumulate, seed=0):
    g = torch.Generator().manual_seed(seed)
    M = B * rows
    dy, logical = _dy_layout(kind, B, rows, N, dev, g)
    y0 = torch.randn(M, N, generator=g).to(BF16).to(dev)
    inv = (0.5 + torch.rand(N, generator=g)).to(dev)
    prev = torch.randn(N, generator=g).to(dev)
    dm, tail = _guarded((N,), F32, dev, -7.0)
    dm.copy_(prev)
    fns.dora_dmag(dy, y0, inv, dm, accumulate=accumulate)
    ok, worst = DB.inside(dm, *DB.dmag_ref(logical, y0, inv, prev if accumulate else None))
    print(f"[dora_dmag {kind} {B} x {rows} rows N={N} acc={accumulate}] worst error / bound = {worst:.3f}")
    assert ok, worst
    assert bool((tail == -7.0).all())
    return dm.clone()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N", [64, 72])
@pytest.mark.parametrize("kind,B", [("compact", 1), ("view", 2)])          # M rows compact, and a [2, M, N] view of a taller joint buffer
@pytest.mark.parametrize("M", [1, 37, 300])                                # 300: more than one 256-row chunk; 2 x 300: a chunk that straddles the two segments
def test_dmag_is_inside_the_derived_bounds_and_repeats_bit_for_bit(M, kind, B, N, accumulate):
    a = check_dmag(OPS, DEV, kind, B, M, N, accumulate)
    b = check_dmag(OPS, DEV, kind, B, M, N, accumulate)
    assert torch.equal(a, b)


@pytest.mark.parametrize("N", [64, 72])
@pytest.mark.parametrize("M", [1, 37, 300])
def test_dmag_of_a_view_and_of_its_compact_copy_give_equal_bits(M, N):
    assert torch.equal(check_dmag(OPS, DEV, "view", 2, M, N, True, seed=4), check_dmag(OPS, DEV, "compact", 2, M, N, True, seed=4))


def check_db_finish(fns, dev, N, rank, accumulate, seed=0):
    g = torch.Generator().manual_seed(seed)
    P, gv, prev = torch.randn(N, rank, generator=g).to(dev), (0.5 + torch.rand(N, generator=g)).to(dev), torch.randn(N, rank, generator=g).to(dev)
    gB, tail = _guarded((N, rank), F32, dev, -7.0)
    gB.copy_(prev)
    fns.dora_db_finish(P, gv, gB, accumulate=accumulate)
    ok, worst = DB.inside(gB, *DB.db_finish_ref(P, gv, prev if accumulate else None))
    assert ok, worst
    assert bool((tail == -7.0).all())
    return gB.clone()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N,rank", [(64, 4), (72, 16), (72, 128), (1, 1)])
def test_db_finish_is_inside_the_derived_bounds_and_repeats_bit_for_bit(N, rank, accumulate):
    assert torch.equal(check_db_finish(OPS, DEV, N, rank, accumulate), check_db_finish(OPS, DEV, N, rank, accumulate))


@pytest.mark.parametrize("N,K,G,rank", [(80, 200, 3, 4), (64, 64, 1, 32), (80, 64, 3, 128)])
def test_stand_ins_against_the_kernels_op_by_op(N, K, G, rank):
    """both sit inside the bounds around one fp64 reference (the checks assert that), so they differ by at most two bounds: a bf16 output by at most one bf16 step,
    an fp32 one by the sum of the two bounds"""
    dev, emu = check_fold(OPS, DEV, N, K, G, rank, seed=5), check_fold(STAND, "cpu", N, K, G, rank, seed=5)
    ref = DB.fold_ref(dev.W, dev.A_cat_T, dev.B_blk, dev.m, dev.targets, dev.r_pad)
    for name in ("inv_norm", "g"):
        assert bool(((dev.outs[name][0].cpu().double() - emu.outs[name][0].double()).abs() <= 2 * ref[name][1]).all()), name
    for name in ("Wf", "Bf", "WfT", "BfT"):
        a, b = dev.outs[name][0].cpu().float(), emu.outs[name][0].float()
        assert bool(((a - b).abs() <= 2 ** -7 * b.abs() + 1e-30).all()), name
    for kind, B, M in (("compact", 1, 37), ("view", 2, 300)):
        a, b = check_dmag(OPS, DEV, kind, B, M, 72, True, seed=6), check_dmag(STAND, "cpu", kind, B, M, 72, True, seed=6)
        assert (a.cpu() - b).abs().max().item() <= 1e-5 * b.abs().max().item()
    a, b = check_db_finish(OPS, DEV, 72, 16, True, seed=7), check_db_finish(STAND, "cpu", 72, 16, True, seed=7)
    assert (a.cpu() - b).abs().max().item() <= 1e-6 * b.abs().max().item()


# ------------------------------------------------------------------------------------------------
# the tiny SD3 step
# ------------------------------------------------------------------------------------------------
def _gpu_model(dora, rank=16, seed=11):
    """the small SD3 config of the host-sequencing tests with 2 layers, the first a dual-attention block (the last block never is)"""
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device=DEV, **SH._arch(2, qk_norm="rms_norm", dual=(0,)))
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
    model.add_lora_adapter(rank=rank, alpha=float(rank), init_b_std=0.02, dora=dora)
    model.prepare_for_training()
    model.train()
    return model


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "per-block"])
def test_the_tiny_sd3_step_matches_the_dora_oracle(monkeypatch, ckpt):
    """loss and every gradient against autograd through the oracle with the DoRA linear, at the tolerances of the SD3 LoRA step test (tests/test_sd3_model_gpu.py:
    prediction rel-L2 <= 2e-2, loss |delta| <= 1e-3, adapter gradients rel-L2 <= 5e-2 per matrix); m's gradient to 5e-2 of its own maximum"""
    model = _gpu_model(True)
    _perturb(model)
    model.gradient_checkpointing = ckpt
    d = SH._inputs(2, 16, 24, 33)
    out, loss = SH._hip_side(model, {k: v.to(DEV) for k, v in d.items()})
    o_out, o_loss, lp, mags = _oracle(monkeypatch, model, d)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))
    n_m = 0
    for name, p in model.named_parameters():
        if ".lora_" not in name:
            continue
        ref = _ref_grad(name, lp, mags)
        if name.endswith(DR.KEY):
            n_m += 1
            assert ref.abs().max().item() > 0 and (p.grad.cpu() - ref).abs().max().item() <= 5e-2 * ref.abs().max().item(), name
        else:
            assert PU.rel_l2(p.grad, ref) < 5e-2, name
    assert n_m == sum(len(g.targets) for g in model.lora_groups)


def test_at_fresh_init_the_output_is_bit_equal_to_the_plain_lora_run_host_sequenced(monkeypatch):
    from simpletuner_amd.sd3 import transformer as T
    d = {k: v.to(DEV) for k, v in SH._inputs(2, 16, 24, 33).items()}
    run = lambda m: m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()
    a = run(_gpu_model(True))
    monkeypatch.setattr(T, "_BLOCK_ABI", False)
    assert torch.equal(a, run(_gpu_model(False)))


def _trainer(graph: bool):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    cfg = default_config(model_family="sd3", lora_rank=8, seed=5, lora_init_b_std=0.02, learning_rate=1e-3, train_batch_size=2, hip_graph=graph)
    cfg.use_dora = True
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
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
    assert any(not torch.equal(g.dora.g, torch.ones_like(g.dora.g)) for g in pe.get_trained_component().lora_groups)          # the magnitudes moved: g left 1

"""LoRA dropout (`lora_dropout`) on the CPU: the generator and the mask's counter lay-out, the scaling convention against torch, the stand-ins against the derived
bounds, the SD3 engine on the kernel-contract emulator against autograd through the oracle with the masked linear, and the plugin / trainer surface."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import sd3 as OS
from tests import lora_dropout_bounds as LB
from tests import lora_dropout_ref as LD
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------
# (a) the generator, the mask
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answer_vectors(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10"""
    got = tuple(int(w.item()) for w in LD.philox4x32_10(*ctr, *key))
    assert got == want, [hex(g) for g in got]


def test_counter_layout_of_the_mask():
    """element (row, col) of an [M, K] input: group (row K + col) / 8 in (c0, c1), the stream in c2, the call in c3; lane j = col % 8 from bits 16 (j % 2) of word j / 2"""
    M, K, key, call, stream, T = 5, 24, (0x1234, 0xabcd), 7, 3, 20000
    keep = LD.keep_mask(M, K, key, call, stream, T)
    for (row, col) in ((0, 0), (0, 7), (2, 9), (4, 23)):
        grp = (row * K + col) // 8
        w = LD.philox4x32_10(grp & 0xFFFFFFFF, grp >> 32, stream, call, *key)
        j = col % 8
        lane = (int(w[j // 2].item()) >> (16 * (j % 2))) & 0xFFFF
        assert bool(keep[row, col]) == (lane >= T)
    # the 64-bit group index carries into c1
    hi = LD.philox4x32_10(5, 1, stream, call, *key)
    lo = LD.philox4x32_10(5, 0, stream, call, *key)
    assert any(int(a.item()) != int(b.item()) for a, b in zip(hi, lo))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    """[154, 192]: the kept count within 6 sigma of n (1 - p'); two streams / calls / ranks disagree on 2 n p' (1 - p') elements within 6 sigma (the disagreement of two
    independent Bernoulli(p') draws has probability q = 2 p' (1 - p'), so the count has variance n q (1 - q)); no two of the eight lanes of a group agree on every group"""
    M, K, seed = 154, 192, 42
    n = M * K
    T = LD.threshold(p)
    pr = T / 65536.0
    base = LD.keep_mask(M, K, LD.key_of(seed, 0), 1, 0, T)
    sd = math.sqrt(n * pr * (1 - pr))
    assert abs(int(base.sum()) - n * (1 - pr)) <= 6 * sd
    q = 2 * pr * (1 - pr)
    for other in (LD.keep_mask(M, K, LD.key_of(seed, 0), 1, 1, T), LD.keep_mask(M, K, LD.key_of(seed, 0), 2, 0, T), LD.keep_mask(M, K, LD.key_of(seed, 1), 1, 0, T)):
        assert abs(int((base ^ other).sum()) - n * q) <= 6 * math.sqrt(n * q * (1 - q))
    lanes = LD.lanes16(M, K, LD.key_of(seed, 0), 1, 0).view(-1, 8)
    for a in range(8):
        for b in range(a + 1, 8):
            assert not torch.equal(lanes[:, a], lanes[:, b])


# ------------------------------------------------------------------------------------------------
# (b) the scaling convention is torch's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_nn_dropout_is_keep_over_one_minus_p(p):
    torch.manual_seed(0)
    x = torch.randn(64, 48, dtype=F64) + 3.0          # (no zeros in x: keep = out != 0)
    out = torch.nn.Dropout(p)(x)
    keep = out != 0
    assert 0 < int(keep.sum()) < x.numel()
    assert torch.allclose(out, x * keep / (1 - p), rtol=1e-12, atol=0)


def test_closed_forms_equal_autograd_under_an_explicit_mask():
    g = torch.Generator().manual_seed(1)
    M, K, N, r, s, scale = 20, 16, 12, 4, 0.5, 1.0 / (1.0 - 0.25)
    x, W, A, Bm, dy = (torch.randn(*sh, dtype=F64, generator=g) for sh in ((M, K), (N, K), (r, K), (N, r), (M, N)))
    keep = torch.rand(M, K, generator=g) >= 0.25
    xa, Aa, Ba = (t.clone().requires_grad_(True) for t in (x, A, Bm))
    y = F.linear(xa, W) + F.linear(F.linear(xa * keep * scale, Aa), Ba) * s
    y.backward(dy)
    y64, dx64, dA64, dB64 = LD.lora64(x, W, A, Bm, s, keep, scale, dy)
    for got, ref in ((y64, y.detach()), (dx64, xa.grad), (dA64, Aa.grad), (dB64, Ba.grad)):
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# (c) the stand-ins (and, on the GPU, the kernels: tests/test_lora_dropout_gpu.py calls check_kernels with the real wrappers) inside the derived bounds
# ------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [("seg77", 2, 77), ("seg256", 2, 256), ("compact", 1, 154)]


def _layout(kind, B, rows, C, dev, g, scale=1.0):
    """a bf16 [B * rows, C] operand: compact, or the rows [lo, lo + rows) of every sample of a joint [B, S, C] buffer as a [B, rows, C] view.  Returns (operand,
    its compact copy)"""
    v = (torch.randn(B * rows, C, generator=g) * scale).to(BF16)
    if kind == "compact":
        return v.clone().to(dev), v
    lo, S = 24, rows + 40
    joint = torch.full((B, S, C), float("nan"), dtype=BF16)
    joint[:, lo:lo + rows] = v.view(B, rows, C)
    return joint.to(dev)[:, lo:lo + rows], v


def check_kernels(fns, dev, kind, B, rows, K, G, rank, accumulate, seed=0, p=0.25):
    """one logical problem through the three wrappers `fns` (the ops module or the stand-ins) at the lay-out `kind`: every output inside its bound; returns the outputs"""
    g = torch.Generator().manual_seed(seed)
    M = B * rows
    r_pad = 32 if rank <= 32 else (rank + 63) // 64 * 64
    K2 = (G * r_pad + 63) // 64 * 64
    drop = LD.Drop(p, seed=99, rank=1, calls=5, device=dev)
    streams = [7 + 3 * i for i in range(G)]
    scale = float(LD.scale_f32(drop.thr))
    key, call, T = (drop.key0, drop.key1), 5, drop.thr
    keeps = [LD.keep_mask(M, K, key, call, st, T) for st in streams]
    x_op, x = _layout(kind, B, rows, K, dev, g)
    A_cat = torch.zeros(K2, K, dtype=BF16)
    for i in range(G):
        A_cat[i * r_pad:i * r_pad + rank] = (torch.randn(rank, K, generator=g) / K ** 0.5).to(BF16)
    U = (torch.randn(M, K2, generator=g) * 0.5).to(BF16)
    # ---- forward ----
    T_out = fns.lora_down_drop(x_op, A_cat.to(dev), r_pad, streams, drop, out=torch.full((M, K2), float("nan"), dtype=BF16, device=dev)).cpu()
    for i in range(G):
        ref, bound = LB.down(x, A_cat[i * r_pad:(i + 1) * r_pad], keeps[i], scale)
        err = (T_out[:, i * r_pad:(i + 1) * r_pad].to(F64) - ref).abs()
        assert bool((err <= bound).all()), f"T target {i}: worst excess {(err - bound).max().item():.3e}"
    assert bool((T_out[:, G * r_pad:] == 0).all())                                     # the K-extension's padding columns
    # ---- dA ----
    prev = [torch.randn(rank, K, generator=g) for _ in range(G)]
    gA = [(q.clone() if accumulate else torch.full((rank, K), float("nan"))).to(dev) for q in prev]
    multi = 1 < G <= 4 and r_pad == 32 and K2 >= 128
    cw = min(r_pad, 64)
    U_dev = U.to(dev)
    if multi:
        fns.skinny_tn_drop_multi(x_op, U_dev, gA, 1, K, rank, streams, drop, accumulate=accumulate)
    else:
        for i in range(G):
            for s0 in range(0, rank, cw):
                c0 = i * r_pad + s0
                fns.skinny_tn_drop(x_op, U_dev[:, c0:c0 + cw], gA[i][s0:], 1, K, min(cw, rank - s0), streams[i], drop, accumulate=accumulate)
    for i in range(G):
        ref, bound = LB.dA(x, U[:, i * r_pad:i * r_pad + rank], keeps[i], scale, prev=prev[i] if accumulate else None, chunks=(M + 255) // 256)
        err = (gA[i].cpu().to(F64) - ref).abs()
        assert bool((err <= bound).all()), f"dA target {i}: worst excess {(err - bound).max().item():.3e}"
    # ---- dx ----
    dx_op, dx_old = _layout(kind, B, rows, K, dev, g)
    fns.lora_dx_drop(dx_op, U_dev, A_cat.t().contiguous().to(dev), r_pad, streams, drop)
    ref, bound = LB.dx(dx_old, U, A_cat, keeps, r_pad, scale)
    dx_new = dx_op.cpu().reshape(M, K)
    err = (dx_new.to(F64) - ref).abs()
    assert bool((err <= bound).all()), f"dx: worst excess {(err - bound).max().item():.3e}"
    return T_out, [q.cpu() for q in gA], dx_new


def check_dx_two_roundings(fns, dev, G, rank, seed=0, p=0.25):
    """the input gradient as the engine forms it under dropout — the plain dx GEMM (bf16 store: the first rounding), then lora_dx_drop in place (the second) — against
    the fp64 product dy W + scale sum_g keep_g . (U_g A_g), element-wise inside lora_dropout_bounds.dx_after_gemm.  fns: gemm and lora_dx_drop."""
    g = torch.Generator().manual_seed(seed)
    M, K, N = 154, 192, 128
    r_pad = 32 if rank <= 32 else (rank + 63) // 64 * 64
    K2 = (G * r_pad + 63) // 64 * 64
    drop = LD.Drop(p, seed=99, rank=1, calls=5, device=dev)
    streams = [2 + 5 * i for i in range(G)]
    keeps = [LD.keep_mask(M, K, (drop.key0, drop.key1), 5, st, drop.thr) for st in streams]
    dy, wT = torch.randn(M, N, generator=g).to(BF16), (torch.randn(K, N, generator=g) / N ** 0.5).to(BF16)
    A_cat = torch.zeros(K2, K, dtype=BF16)
    for i in range(G):
        A_cat[i * r_pad:i * r_pad + rank] = (torch.randn(rank, K, generator=g) / K ** 0.5).to(BF16)
    U = (torch.randn(M, K2, generator=g) * 0.5).to(BF16)
    dx = fns.gemm(dy.to(dev), wT.to(dev))
    fns.lora_dx_drop(dx, U.to(dev), A_cat.t().contiguous().to(dev), r_pad, streams, drop)
    ref, bound = LB.dx_after_gemm(dy.to(F64) @ wT.to(F64).t(), dy.to(F64).abs() @ wT.to(F64).abs().t(), N, U, A_cat, keeps, r_pad, float(LD.scale_f32(drop.thr)))
    err = (dx.cpu().to(F64) - ref).abs()
    assert bool((err <= bound).all()), f"dx after the GEMM: worst excess {(err - bound).max().item():.3e}"


@pytest.mark.parametrize("G,rank", [(1, 4), (3, 4), (3, 64), (4, 128)])
def test_the_two_roundings_of_dx_on_the_stand_ins(monkeypatch, G, rank):
    ops = LD.install(monkeypatch)
    check_dx_two_roundings(SimpleNamespace(gemm=ops.gemm, lora_dx_drop=ops.lora_dx_drop), "cpu", G, rank)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rank", [4, 64, 128])
@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("kind,B,rows", KERNEL_SHAPES)
@pytest.mark.parametrize("K", [64, 192])
def test_stand_ins_stay_inside_the_derived_bounds(K, kind, B, rows, G, rank, accumulate):
    check_kernels(SimpleNamespace(**LD.STAND_INS), "cpu", kind, B, rows, K, G, rank, accumulate)


def test_a_strided_view_and_its_compact_copy_draw_one_mask():
    fns = SimpleNamespace(**LD.STAND_INS)
    a = check_kernels(fns, "cpu", "seg77", 2, 77, 64, 3, 4, False, seed=3)
    b = check_kernels(fns, "cpu", "compact", 1, 154, 64, 3, 4, False, seed=3)
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and torch.equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------
# (d) the SD3 engine on the emulator
# ------------------------------------------------------------------------------------------------
P_DROP, SEED, RANK = 0.25, 1234, 2


def _model(monkeypatch, layers, sd35=False, dropout=P_DROP, rank=16, calls=0):
    LD.install(monkeypatch)
    model = SH._model(monkeypatch, layers, sd35)
    LD.install(monkeypatch)                       # (SH._model installs the plain emulator again)
    model.add_lora_adapter(rank=rank, alpha=float(rank), init_b_std=0.02, dropout=dropout, dropout_seed=SEED, dropout_rank=RANK, dropout_calls=calls)
    model.train()
    return model


def test_stream_ids_are_the_index_in_the_ordered_target_list(monkeypatch):
    """every adapted Linear its own mask stream: 0 .. n - 1 in the order the adapters were laid out (= the order of the lora_A parameters), so to_q / to_k / to_v of one
    group, attn and attn2 of a dual block and the blocks themselves never share one — a shared mask would be a different distribution"""
    model = _model(monkeypatch, 3, True)
    order = [n.split(".lora_A.")[0] for n, _ in model.named_parameters() if ".lora_A." in n]
    ids = LD.stream_ids(model)
    assert len(order) == len(set(order)) == len(ids) == sum(len(g.targets) for g in model.lora_groups)
    assert [ids[n] for n in order] == list(range(len(order)))
    for g in model.lora_groups:
        assert len(set(g.streams)) == len(g.targets)


def _oracle(monkeypatch, model, d, call, T, tread=None):
    """autograd through the oracle with the masked linear (T = 0: without the mask)"""
    monkeypatch.setattr(OS, "linear", LD.masked_linear(LD.stream_ids(model), LD.key_of(SEED, RANK), call, T))
    P, lora, scale = PU.oracle_state(model)
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    kw = dict(tread=tread) if tread is not None else {}
    out = OS.sd3_forward(P, SH._ocfg(model), d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale, **kw)
    loss = ((out - d["target"].float()) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), lp


def _worst(model, lp):
    worst = 0.0
    for name, p in model.named_parameters():
        if ".lora_" in name:
            key, which = name.split(".lora_")
            worst = max(worst, PU.rel_l2(p.grad, lp[key][0 if which.startswith("A") else 1].grad))
    return worst


def _compare(monkeypatch, model, d, out, loss, call, tread=None):
    T = model.lora_dropout.thr
    o_out, o_loss, lp = _oracle(monkeypatch, model, d, call, T, tread)
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, o_loss.item())
    worst = _worst(model, lp)
    assert worst < 5e-2, worst
    # ... and a computation that forgets the mask is far outside the same tolerances
    n_out, _, nlp = _oracle(monkeypatch, model, d, call, 0, tread)
    plain = _worst(model, nlp)
    assert plain > 0.25, plain
    return worst, plain


def _set_ckpt(model, mode):
    if mode != "plain":
        model.gradient_checkpointing = True
    if mode == "segmented":
        model.gradient_checkpointing_interval = 2
    if mode == "stride":          # a plan that recomputes some segments and keeps others
        model.gradient_checkpointing_interval, model.gradient_checkpointing_segment_stride = 2, 3


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented", "stride"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_engine_with_lora_dropout_matches_autograd_through_the_masked_oracle(monkeypatch, sd35, ckpt):
    model = _model(monkeypatch, 4 if ckpt == "stride" else 3, sd35, calls=4)
    _set_ckpt(model, ckpt)
    if ckpt == "stride":
        from simpletuner_amd.training.checkpoint_plan import segments
        plan = segments(len(model.blocks), True, 2, 3)
        assert any(ck for (_, _, ck) in plan) and not all(ck for (_, _, ck) in plan), plan          # recomputed and kept segments in one backward
    d = SH._inputs(2, 16, 24, 33)
    out, loss = SH._hip_side(model, d)
    assert model.lora_dropout.calls() == 5          # one advance per training forward, none per recompute
    worst, plain = _compare(monkeypatch, model, d, out, loss, 5)
    print(f"[emu] sd3{'.5' if sd35 else ''} lora_dropout {ckpt}: worst adapter gradient rel-L2 {worst:.3e} with the mask, {plain:.3e} against a reference without it")


@pytest.mark.parametrize("ckpt", ["plain", "per-block"])          # (under routing every plan is the per-block one, as in the reference)
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_engine_with_lora_dropout_under_tread(monkeypatch, sd35, ckpt):
    from simpletuner_amd.training.tread import ReplayRouter
    d = SH._inputs(2, 16, 16, 24)
    B, Si = 2, 64
    g = torch.Generator().manual_seed(11)
    perm = torch.stack([torch.randperm(Si, generator=g) for _ in range(B)])
    Kk = Si - int(round(Si * 0.5))
    rec = {"mask": torch.ones(B, Si, dtype=torch.bool).scatter_(1, perm[:, :Kk], False), "ids_keep": perm[:, :Kk], "ids_mask": perm[:, Kk:], "ids_shuffle": perm,
           "ids_restore": torch.argsort(perm, dim=1)}
    routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]
    model = _model(monkeypatch, 4, sd35, rank=8)
    model.set_router(ReplayRouter([rec]), routes)
    _set_ckpt(model, ckpt)
    out, loss = SH._hip_side(model, d)
    assert model.lora_dropout.calls() == 1
    _compare(monkeypatch, model, d, out, loss, 1, tread={"routes": routes, "mask_infos": [rec]})


def test_a_second_training_forward_draws_other_masks_and_eval_is_the_p0_forward(monkeypatch):
    d = SH._inputs(2, 16, 24, 33)
    model = _model(monkeypatch, 2)
    run = lambda m: m(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0].detach()
    a, b = run(model), run(model)
    assert model.lora_dropout.calls() == 2 and not torch.equal(a, b)
    plain = _model(monkeypatch, 2, dropout=0.0)
    assert plain.lora_dropout is None
    ref = run(plain)
    assert not torch.equal(a, ref)
    model.eval()
    assert torch.equal(run(model), ref) and model.lora_dropout.calls() == 2          # an eval() forward: no mask, no advance
    with torch.no_grad():
        model.train()
        assert torch.equal(run(model), ref)                                           # a forward without gradients (validation sampling) likewise


def test_the_launch_stream_with_the_flag_off_does_not_change(monkeypatch):
    """What this test shows, and what it does not: on ONE commit, `dropout=0.0` handed over explicitly issues the same sequence of wrapper NAMES (and the same output
    bits) as a model built without the argument, none of them a dropout wrapper, and `dropout=0.25` leaves the block-level entry points for the masked wrappers.  It
    does not use tools/launch_trace.py and compares nothing against the parent commit.  The flag-off stream itself — every emulated launch with its operands' dtypes,
    shapes and strides — is pinned by tests/test_layersync_cpu.py's digest of tools/launch_trace.py over the Flux and SD3 LoRA host-sequencing tests, recorded
    before LayerSync: a change of this feature to the flag-off launches of those tests fails there."""
    from simpletuner_amd import ops
    d = SH._inputs(2, 16, 24, 33)

    def trace(**kw):
        LD.install(monkeypatch)
        model = SH._model(monkeypatch, 3, True)
        LD.install(monkeypatch)
        names = []
        for nm in ("gemm", "gemm_grouped", "skinny_tn", "skinny_tn_multi", "block_sd3_joint_fwd", "block_sd3_joint_bwd") + tuple(LD.STAND_INS):
            fn = getattr(ops, nm)
            monkeypatch.setattr(ops, nm, (lambda f, n: (lambda *a, **k: (names.append(n), f(*a, **k))[1]))(fn, nm))
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02, **kw)
        model.train()
        out, _ = SH._hip_side(model, d)
        return names, out

    (n0, o0), (n1, o1) = trace(), trace(dropout=0.0)
    assert n0 == n1 and torch.equal(o0, o1) and not any(n in LD.STAND_INS for n in n0)
    n2, _ = trace(dropout=0.25)
    assert "lora_down_drop" in n2 and "lora_dx_drop" in n2 and "block_sd3_joint_fwd" not in n2


# ------------------------------------------------------------------------------------------------
# (e) surface
# ------------------------------------------------------------------------------------------------
def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family="sd3", **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    LD.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=0.02, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(2))
    return plugin


@pytest.mark.parametrize("cls_path", ["simpletuner_amd.flux.model.Flux", "simpletuner_amd.pixart.model.PixartSigma", "simpletuner_amd.sdxl.model.SDXL",
                                      "simpletuner_amd.sd1x.model.StableDiffusion1"])
def test_families_without_the_masked_kernels_refuse_the_flag_by_name(cls_path):
    import importlib
    mod, cls = cls_path.rsplit(".", 1)
    Plug = getattr(importlib.import_module(mod), cls)
    plug = Plug.__new__(Plug)
    plug.config = SimpleNamespace(model_type="lora", lora_type="standard", lora_dropout=0.1)
    with pytest.raises(NotImplementedError) as ei:
        plug.lora_dropout_value()
    assert str(ei.value) == f"lora_dropout=0.1: LoRA dropout is not built for {Plug.NAME} on the st355 path (built: SD3); set --lora_dropout=0"
    for cfg in (SimpleNamespace(model_type="lora", lora_type="standard"), SimpleNamespace(model_type="lora", lora_type="standard", lora_dropout=0.0),
                SimpleNamespace(model_type="full", lora_dropout=0.1), SimpleNamespace(model_type="lora", lora_type="lycoris", lora_dropout=0.1)):
        plug.config = cfg
        assert plug.lora_dropout_value() == 0.0          # absent = 0; a full fine-tune and lycoris ignore the flag


def test_flux_add_lora_adapter_refuses_and_sd3_takes_the_flag(monkeypatch):
    plugin = _plugin(monkeypatch, "flux")
    plugin.config.lora_dropout = 0.1
    with pytest.raises(NotImplementedError, match=r"lora_dropout=0.1: LoRA dropout is not built for .* \(built: SD3\); set --lora_dropout=0"):
        plugin.add_lora_adapter()
    plugin = _plugin(monkeypatch, "sd3")
    plugin.config.lora_dropout = 0.1
    plugin.add_lora_adapter()
    drop = plugin.get_trained_component().lora_dropout
    assert drop is not None and drop.thr == 6554 and (drop.key0, drop.key1) == LD.key_of(3, 0)
    for bad in (1.0, 1.5, -0.1):
        plugin = _plugin(monkeypatch, "sd3")
        plugin.config.lora_dropout = bad
        with pytest.raises(ValueError, match="lora_dropout must lie in"):
            plugin.add_lora_adapter()


def _trainer(monkeypatch, p):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, "sd3", learning_rate=1e-3)
    plugin.config.lora_dropout = p
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


def test_lora_dropout_changes_the_training_loss_against_zero(monkeypatch):
    plugin0, trainer0, batch0 = _trainer(monkeypatch, 0.0)
    assert plugin0.get_trained_component().lora_dropout is None
    l0 = trainer0.train_step(dict(batch0))
    plugin, trainer, batch = _trainer(monkeypatch, 0.25)
    l1 = trainer.train_step(dict(batch))
    assert plugin.get_trained_component().lora_dropout.calls() == 1
    assert l0.item() != l1.item()


def test_the_call_counter_survives_save_and_resume(monkeypatch, tmp_path):
    """the counter is saved and loaded as itself: it is moved away from the micro-step count (as the warm-up passes of a captured step move it) before the save, so the
    micro-step fallback of a state file without the entry would not pass"""
    import json
    plugin, trainer, batch = _trainer(monkeypatch, 0.25)
    trainer.train_step(dict(batch))
    plugin.get_trained_component().lora_dropout.set_calls(7)
    trainer.save_state(str(tmp_path / "ck"))
    assert json.load(open(tmp_path / "ck" / "training_state.json"))["lora_dropout_calls"] == 7 and trainer.state["micro_step"] == 1
    want = trainer.train_step(dict(batch))
    want_w = plugin.get_trained_component().lora_flat.clone()
    assert plugin.get_trained_component().lora_dropout.calls() == 8
    plugin2, trainer2, _ = _trainer(monkeypatch, 0.25)
    trainer2.load_state(str(tmp_path / "ck"))
    assert plugin2.get_trained_component().lora_dropout.calls() == 7
    got = trainer2.train_step(dict(batch))
    assert got.item() == want.item() and torch.equal(plugin2.get_trained_component().lora_flat, want_w)

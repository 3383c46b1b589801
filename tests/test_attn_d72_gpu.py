"""The fused head_dim-72 attention (csrc/attention_d72.hip) on token-major column blocks with a head pitch and a key bias, element-wise against the fp64 models
of tests/attn_bounds.py: O and lse2, then dQ / dK / dV chained on the kernel's own O and lse2 (delta = sum_c dO O from the bf16 O).  Shapes, adversarial data
and sentinel-filled blocks are those of tests/test_attn_wide_gpu.py plus one 520 x 520 case: from 512 keys the launcher runs dK / dV with 32 keys per wave
instead of 16, so 520 runs that kernel, with ragged tails on both sides and nine staged tiles.  Operands sit at head pitch 72 or 96
with the pad lanes 72 .. pitch-1 left at the sentinel (a contraction step reading past lane 71 would pick it up); the pad lanes of every output must be bit-zero,
nothing outside the blocks may change, and the backward runs twice and must be bit-identical.

The global rel-L2 bar on O (8e-3) is the narrow test's: on the CPU, with the same generator recipe, the fp64 O rounded to bf16 sits at 1.0e-3 .. 1.6e-3 at d 72
over all six shapes, without and with the bias (d 40 / 80: 1.0e-3 .. 1.6e-3; the biased 7 x 2 case keeps one key per row, O = v exactly, 0).  The unchained gradient figures are printed, not asserted, for the reason given in
tests/test_attn_narrow_gpu.py: these kernels take delta from the bf16 O.
"""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests.test_attn_bounds_gpu import _bits, _guard, _sent, dev
from tests.test_attn_wide_gpu import CASES, _blocks, _data

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
D = 72
SHAPES = [c + (False,) for c in CASES + [(1, 2, 520, 520, True)]] + [c + (True,) for c in CASES if not c[4]]


@pytest.mark.parametrize("B,H,Sq,Sk,self_attn,biased", SHAPES)
@pytest.mark.parametrize("pitch", [72, 96])
def test_d72_attention_against_the_fp64_bounds(pitch, B, H, Sq, Sk, self_attn, biased):
    from simpletuner_amd import ops
    Dp, scale = H * pitch, 1.0 / math.sqrt(D)
    name = f"d72 pitch{pitch} B{B} H{H} Sq{Sq} Sk{Sk}{' bias' if biased else ''}"
    g = torch.Generator(device=dev()).manual_seed(Sq + Sk)
    q, k, v, dO = _data(g, B, H, Sq, Sk, D, 3.0 if self_attn else 0.0, scale)
    bias = None
    if biased:      # PixArt's caption mask: -10000 on about a third of the keys of every batch row, at least one key kept
        drop = (torch.arange(Sk, device=dev())[None] + torch.arange(B, device=dev())[:, None]) % 3 == 1
        bias = torch.where(drop, -10000.0, 0.0).float().contiguous()
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(-1, H, D)
    lanes = lambda t2d: t2d.unflatten(1, (H, pitch))                     # [rows, H, pitch] view of a column block
    heads = lambda t2d, S_: lanes(t2d)[:, :, :D].reshape(B, S_, H, D).permute(0, 2, 1, 3)
    _, (q2, k2, v2), _ = _blocks(B, Sq, Sk, Dp, self_attn)
    dO2 = _sent((B * Sq + 5, Dp + 64))[:B * Sq, :Dp]
    for blk, t in ((q2, q), (k2, k), (v2, v), (dO2, dO)):               # lanes 72 .. pitch-1 keep the sentinel
        lanes(blk)[:, :, :D].copy_(rows(t))
    O_buf, lse_buf = _sent((B * Sq + 7, Dp + 32)), _sent((B * H * Sq + 64,), torch.float32)
    O, lse2 = O_buf[:B * Sq, :Dp], lse_buf[:B * H * Sq].view(B, H, Sq)
    before = [_bits(x).clone() for x in (O_buf, lse_buf)]
    ops.attn_d72_fwd(q2, k2, v2, O, lse2, B, H, Sq, Sk, D, scale, pitch=pitch, key_bias=bias)
    torch.cuda.synchronize()
    inside = torch.zeros_like(O_buf, dtype=torch.bool)
    inside[:B * Sq, :Dp] = True
    _guard(f"{name} O", O_buf, inside, before[0])
    _guard(f"{name} lse2", lse_buf, torch.arange(lse_buf.numel(), device=dev()) < B * H * Sq, before[1])
    assert not bool(_bits(lanes(O)[:, :, D:]).any()), f"{name}: pad lanes of O are not zero"
    f = AB.attn_fwd_model(q, k, v, scale, bias=bias)
    Oh = heads(O, Sq)
    reps = [AB.check(f"{name} O", Oh, f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2", lse2, f.lse2, f.e_lse2)]
    r = AB.rel_l2(Oh, f.O)
    print(f"{name} O rel-L2 {r:.2e}")
    assert r < 8e-3

    outs = []
    for _ in range(2):
        bufs, (dq, dk, dv), ins = _blocks(B, Sq, Sk, Dp, self_attn)
        b0 = [_bits(x).clone() for x in bufs]
        ops.attn_d72_bwd(q2, k2, v2, O, dO2, lse2, dq, dk, dv, B, H, Sq, Sk, D, scale, pitch=pitch, key_bias=bias)
        torch.cuda.synchronize()
        for i, (bf, m, bb) in enumerate(zip(bufs, ins, b0)):
            _guard(f"{name} gradient buffer {i}", bf, m, bb)
        outs.append([_bits(x).clone() for x in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*outs)), f"{name}: the backward is not deterministic"
    bw = AB.attn_bwd_model(q, k, v, dO, Oh, lse2, scale, bias=bias)
    u = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale, bias=bias)          # unchained: the fully fp64 backward
    for n, t, S_ in (("dQ", dq, Sq), ("dK", dk, Sk), ("dV", dv, Sk)):
        assert not bool(_bits(lanes(t)[:, :, D:]).any()), f"{name}: pad lanes of {n} are not zero"
        reps.append(AB.check(f"{name} {n}", heads(t, S_), getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n)))
        print(f"[unchained] {name} {n} rel-L2 {AB.rel_l2(heads(t, S_), getattr(u, n)):.2e}")
    for rep in reps:
        AB.assert_bound(rep)


@pytest.mark.parametrize("d,pitch,offset", [(64, None, 0), (80, None, 0), (72, 64, 0), (72, 76, 0), (72, 96, 4)])
def test_other_widths_bad_pitches_and_misaligned_blocks_are_refused(d, pitch, offset):
    """a width that is not built -> ST355_ENOSYS by name; a pitch below 72 or off the 8-lane grid, and a q that starts 8 bytes into a 16-byte chunk -> the
    launcher's precondition messages, before any launch"""
    from simpletuner_amd import lib, ops
    w = 2 * (pitch or d)
    t = torch.zeros(64, w + 8, dtype=BF16, device=dev())
    a, qq = t[:, :w], t[:, offset:offset + w]
    lse = torch.zeros(1, 2, 64, device=dev())
    what = (rf"rc=-38\): attn_d72_(fwd|bwd): head_dim {d} not built" if d != 72 else "every column block needs a 16-byte aligned start" if offset
            else rf"pitch {pitch}: the head pitch must be >= 72 and a multiple of 8")
    with pytest.raises(lib.St355Error, match=what):
        ops.attn_d72_fwd(qq, a, a, torch.empty_like(a), lse, 1, 2, 64, 64, d, 0.1, pitch=pitch)
    with pytest.raises(lib.St355Error, match=what):
        ops.attn_d72_bwd(qq, a, a, a, a, lse, torch.empty_like(a), torch.empty_like(a), torch.empty_like(a), 1, 2, 64, 64, d, 0.1, pitch=pitch)


@pytest.mark.parametrize("case", ["controlnet", "lora"])
def test_pixart_model_with_the_switch_on(monkeypatch, case):
    """tests/test_pixart_model_gpu.py's bf16 trunk + ControlNet gradient case and its LoRA case (at that file's tolerances) on the fused route: self-attention is
    one attn_d72_fwd with Sq == Sk and no bias, cross-attention one with the caption mask's bias, and ops.head_split / head_merge are never called"""
    from simpletuner_amd import ops
    from tests import test_pixart_model_gpu as PM
    calls, copies = [], []
    fwd = ops.attn_d72_fwd
    monkeypatch.setattr(ops, "ATTN_D72", True)
    monkeypatch.setattr(ops, "attn_d72_fwd", lambda *a, **kw: (calls.append((a[7] == a[8], kw.get("key_bias") is not None, kw.get("pitch"))), fwd(*a, **kw))[1])
    monkeypatch.setattr(ops, "head_split", lambda *a, **kw: copies.append("split"))
    monkeypatch.setattr(ops, "head_merge", lambda *a, **kw: copies.append("merge"))
    if case == "controlnet":
        PM.test_pixart_controlnet_branch_gradients_match_autograd()
    else:
        PM.test_pixart_trunk_lora_gradients_match_autograd(False)
    assert not copies, copies
    assert set(calls) == {(True, False, 96), (False, True, 96)} and len(calls) % 2 == 0, calls

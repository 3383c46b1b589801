"""The fused head_dim-40 / 80 attention (csrc/attention_narrow.hip) on token-major column blocks, element-wise against the fp64 models of tests/attn_bounds.py:
O, lse2 and (self cases) O + o_res, then dQ / dK / dV chained on the kernel's own O, o_res and lse2 (delta = sum_c dO (O + o_res), the attn_bwd_res chaining of
tests/test_attn_bounds_gpu.py).  Shapes, adversarial data and sentinel-filled blocks are those of tests/test_attn_wide_gpu.py: for d = 40 the sentinels right of
the last head are what a tail contraction step that loads past its head would read.  The backward runs twice and must be bit-identical.

Of the wide test's two global rel-L2 bars, the one on O (8e-3) stays: the fp64 O rounded to bf16 sits at 1.0e-3 .. 1.6e-3 at these inputs (CPU, both widths,
all five shapes).  The unchained 2e-2 bar on the gradients does not: these kernels take delta from the bf16 O (+ o_res in the self cases), and the fp64 backward
alone, fed the fp64 O rounded to bf16 and with its results rounded to bf16, already gives 2.20e-2 (d 40, dQ) and 2.22e-2 (d 80, dK) against the fully fp64
backward at the cross case (1, 1, 7, 2) with the CPU generator's data — all its rows are near one-hot, dP - delta cancels — and 7.7e-3 / 8.0e-3 on dQ at
(1, 2, 200, 77); 1.6e-3 .. 1.8e-3 everywhere with o_res.  The kernels on the device generator's data: 1.9e-3 .. 4.2e-3 in the self cases, 8.1e-3 / 8.0e-3 on dQ
at Sk 77, and 2.2e-2 / 1.4e-1 (d 40, dQ / dK), 1.8e-1 / 6.8e-1 (d 80) at (1, 1, 7, 2).  The unchained figures are printed; the element-wise bounds, chained on
what the kernels read, are the check.
"""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests.test_attn_bounds_gpu import _bits, _guard, _sent, dev
from tests.test_attn_wide_gpu import CASES, _blocks, _data

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize("B,H,Sq,Sk,self_attn", CASES)
@pytest.mark.parametrize("d", [40, 80])
def test_narrow_attention_against_the_fp64_bounds(d, B, H, Sq, Sk, self_attn):
    from simpletuner_amd import ops
    D, scale = H * d, 1.0 / math.sqrt(d)
    name = f"narrow d{d} B{B} H{H} Sq{Sq} Sk{Sk}"
    g = torch.Generator(device=dev()).manual_seed(Sq + Sk)
    q, k, v, dO = _data(g, B, H, Sq, Sk, d, 3.0 if self_attn else 0.0, scale)
    _, (q2, k2, v2), _ = _blocks(B, Sq, Sk, D, self_attn, fill=(q, k, v))
    dO2 = _sent((B * Sq + 5, D + 64))[:B * Sq, :D]
    dO2.copy_(dO.permute(0, 2, 1, 3).reshape(B * Sq, D))
    O_buf, R_buf, lse_buf = _sent((B * Sq + 7, D + 32)), _sent((B * Sq + 7, D + 32)), _sent((B * H * Sq + 64,), torch.float32)
    O, lse2 = O_buf[:B * Sq, :D], lse_buf[:B * H * Sq].view(B, H, Sq)
    R = R_buf[:B * Sq, :D] if self_attn else None
    before = [_bits(x).clone() for x in (O_buf, R_buf, lse_buf)]
    ops.attn_narrow_fwd(q2, k2, v2, O, lse2, B, H, Sq, Sk, d, scale, o_res=R)
    torch.cuda.synchronize()
    inside = torch.zeros_like(O_buf, dtype=torch.bool)
    inside[:B * Sq, :D] = True
    _guard(f"{name} O", O_buf, inside, before[0])
    if self_attn:
        _guard(f"{name} o_res", R_buf, inside, before[1])
    _guard(f"{name} lse2", lse_buf, torch.arange(lse_buf.numel(), device=dev()) < B * H * Sq, before[2])
    heads = lambda t2d, S_: t2d.reshape(B, S_, H, d).permute(0, 2, 1, 3)
    f = AB.attn_fwd_model(q, k, v, scale)
    Oh, Rh = heads(O, Sq), heads(R, Sq) if self_attn else None
    reps = [AB.check(f"{name} O", Oh, f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2", lse2, f.lse2, f.e_lse2)]
    if self_attn:      # O + o_res carries the fp32 output acc / l (one fp32 rounding, u |O|): the same model as O, with the final RNE that of the residual
        reps.append(AB.check(f"{name} O + o_res", Oh.double() + Rh.double(), f.O, f.e_O + AB.U24 * f.O.abs(), f.var_O, final=f.O - Oh.double()))
    r = AB.rel_l2(Oh, f.O)
    print(f"{name} O rel-L2 {r:.2e}")
    assert r < 8e-3

    outs = []
    for _ in range(2):
        bufs, (dq, dk, dv), ins = _blocks(B, Sq, Sk, D, self_attn)
        b0 = [_bits(x).clone() for x in bufs]
        ops.attn_narrow_bwd(q2, k2, v2, O, dO2, lse2, dq, dk, dv, B, H, Sq, Sk, d, scale, o_res=R)
        torch.cuda.synchronize()
        for i, (bf, m, bb) in enumerate(zip(bufs, ins, b0)):
            _guard(f"{name} gradient buffer {i}", bf, m, bb)
        outs.append([_bits(x).clone() for x in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*outs)), f"{name}: the backward is not deterministic"
    bw = AB.attn_bwd_model(q, k, v, dO, Oh, lse2, scale, O_res=Rh)
    u = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale)          # unchained: the fully fp64 backward
    for n, t, S_ in (("dQ", dq, Sq), ("dK", dk, Sk), ("dV", dv, Sk)):
        reps.append(AB.check(f"{name} {n}", heads(t, S_), getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n)))
        print(f"[unchained] {name} {n} rel-L2 {AB.rel_l2(heads(t, S_), getattr(u, n)):.2e}")
    for rep in reps:
        AB.assert_bound(rep)


@pytest.mark.parametrize("d,offset", [(64, 0), (160, 0), (40, 4)])
def test_other_head_widths_and_misaligned_blocks_are_refused(d, offset):
    """offset 0: a width that is not built -> ST355_ENOSYS by name; offset 4: q starts 8 bytes into a 16-byte chunk -> the launcher's precondition message"""
    from simpletuner_amd import lib, ops
    t = torch.zeros(64, 2 * d + 8, dtype=BF16, device=dev())
    a, qq = t[:, :2 * d], t[:, offset:offset + 2 * d]
    lse = torch.zeros(1, 2, 64, device=dev())
    what = r"every column block needs a 16-byte aligned start" if offset else rf"rc=-38\): attn_narrow_%s: head_dim {d} not built"
    with pytest.raises(lib.St355Error, match=what % "fwd" if not offset else what):
        ops.attn_narrow_fwd(qq, a, a, torch.empty_like(a), lse, 1, 2, 64, 64, d, 0.1)
    with pytest.raises(lib.St355Error, match=what % "bwd" if not offset else what):
        ops.attn_narrow_bwd(qq, a, a, a, a, lse, torch.empty_like(a), torch.empty_like(a), torch.empty_like(a), 1, 2, 64, 64, d, 0.1)


def test_sd15_narrow_heads_model_with_the_switch_on(monkeypatch):
    """tests/test_unet_model_gpu.py's sd15_narrow_heads case (prediction, loss and every parameter gradient vs fp32 autograd, at that file's tolerances) on the
    fused route: every attention (heads 40 and 80, self and cross) goes through attn_narrow_fwd, and ops.head_split is never called"""
    from simpletuner_amd import ops
    from tests import test_unet_model_gpu as UM
    calls, splits = [], []
    fwd = ops.attn_narrow_fwd
    monkeypatch.setattr(ops, "ATTN_NARROW", True)
    monkeypatch.setattr(ops, "attn_narrow_fwd", lambda *a, **kw: (calls.append((a[9], a[7] == a[8], kw.get("o_res") is not None)), fwd(*a, **kw))[1])
    monkeypatch.setattr(ops, "head_split", lambda *a, **kw: splits.append(a))
    UM.test_unet_full_finetune_gradients_match_autograd("sd15_narrow_heads")
    assert not splits, len(splits)
    # (head width, Sq == Sk, o_res kept): self attention keeps the residual, cross attention does not
    assert {c for c in calls} == {(40, True, True), (40, False, False), (80, True, True), (80, False, False)}, calls

"""The fused head_dim-160 attention (csrc/attention_wide.hip) on token-major column blocks, element-wise against the fp64 models of tests/attn_bounds.py (+ the
delta-from-sum(P dP) term of tests/attn_wide_bounds.py): O, lse2, then dQ / dK / dV chained on the kernel's own lse2 with the fp64 forward O.  Operands and
outputs sit inside sentinel-filled buffers wider and longer than the contract; the backward runs twice and must be bit-identical."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests import attn_wide_bounds as AWB
from tests.test_attn_bounds_gpu import _bits, _guard, _sent, dev

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
D_HEAD = 160
# (B, H, Sq, Sk, self): one exact tile (the mid block) | ragged tails of 16, H not a power of two, batch stride | a 13-key second tile, Sq % 8 != 0 |
# everything inside one partial tile | five tiles: the staging ring wraps
CASES = [(1, 2, 64, 64, True), (2, 3, 144, 144, True), (1, 2, 200, 77, False), (1, 1, 7, 2, False), (1, 2, 320, 320, True)]


def _data(g, B, H, Sq, Sk, d, common, scale):
    """test_attn_bounds_gpu._data's adversarial rows: a late 70-nat spike, a max rising tile by tile, a max in the ragged tail, a zero query, a near one-hot row"""
    q, k, v, dO = (torch.randn(B, H, S_, d, device=dev(), generator=g) for S_ in (Sq, Sk, Sk, Sq))
    if common:
        k += common * torch.randn(B, H, 1, d, device=dev(), generator=g)
        v += common * torch.randn(B, H, 1, d, device=dev(), generator=g)
    q, k = q.to(BF16).float(), k.to(BF16).float()
    aim = lambda row, nats: row * (nats / (scale * float((row * row).sum().clamp_min(1e-6))))
    for b in range(B):
        for h in range(H):
            spike = max(0, Sk - 70)
            k[b, h, spike] = aim(q[b, h, 0], 70.0)
            for t in range((Sk + 63) // 64):
                j = min(Sk - 1, 64 * t + 17)
                if j != spike:
                    k[b, h, j] = aim(q[b, h, 1], 4.0 + 0.5 * t)
            k[b, h, Sk - 1] = aim(q[b, h, 2], 25.0)
            q[b, h, 3] = 0
            q[b, h, 4] = aim(k[b, h, Sk // 2], 30.0)
    return q.to(BF16), k.to(BF16), v.to(BF16), dO.to(BF16)


def _blocks(B, Sq, Sk, D, self_attn, fill=None):
    """sentinel-filled q | k | v column blocks: one [B S + 5, 3 D + 64] buffer (self) or [.., D + 64] and [.., 2 D + 64] (cross); fill: head-major tensors to place"""
    if self_attn:
        buf = _sent((B * Sq + 5, 3 * D + 64))
        bufs, views = [buf], [buf[:B * Sq, i * D:(i + 1) * D] for i in range(3)]
    else:
        bq, bkv = _sent((B * Sq + 5, D + 64)), _sent((B * Sk + 5, 2 * D + 64))
        bufs, views = [bq, bkv], [bq[:B * Sq, :D], bkv[:B * Sk, :D], bkv[:B * Sk, D:2 * D]]
    inside = []
    for bf in bufs:
        m = torch.zeros_like(bf, dtype=torch.bool)
        m[:bf.shape[0] - 5, :bf.shape[1] - 64] = True
        inside.append(m)
    for vw, t in zip(views, fill or ()):
        vw.copy_(t.permute(0, 2, 1, 3).reshape(vw.shape))
    return bufs, views, inside


@pytest.mark.parametrize("B,H,Sq,Sk,self_attn", CASES)
def test_wide_attention_against_the_fp64_bounds(B, H, Sq, Sk, self_attn):
    from simpletuner_amd import ops
    d, D, scale = D_HEAD, H * D_HEAD, 1.0 / math.sqrt(D_HEAD)
    name = f"wide B{B} H{H} Sq{Sq} Sk{Sk}"
    g = torch.Generator(device=dev()).manual_seed(Sq + Sk)
    q, k, v, dO = _data(g, B, H, Sq, Sk, d, 3.0 if self_attn else 0.0, scale)
    _, (q2, k2, v2), _ = _blocks(B, Sq, Sk, D, self_attn, fill=(q, k, v))
    dO2 = _sent((B * Sq + 5, D + 64))[:B * Sq, :D]
    dO2.copy_(dO.permute(0, 2, 1, 3).reshape(B * Sq, D))
    O_buf, lse_buf = _sent((B * Sq + 7, D + 32)), _sent((B * H * Sq + 64,), torch.float32)
    O, lse2 = O_buf[:B * Sq, :D], lse_buf[:B * H * Sq].view(B, H, Sq)
    before = _bits(O_buf).clone(), _bits(lse_buf).clone()
    ops.attn_wide_fwd(q2, k2, v2, O, lse2, B, H, Sq, Sk, d, scale)
    torch.cuda.synchronize()
    inside = torch.zeros_like(O_buf, dtype=torch.bool)
    inside[:B * Sq, :D] = True
    _guard(f"{name} O", O_buf, inside, before[0])
    _guard(f"{name} lse2", lse_buf, torch.arange(lse_buf.numel(), device=dev()) < B * H * Sq, before[1])
    heads = lambda t2d, S_: t2d.reshape(B, S_, H, d).permute(0, 2, 1, 3)
    f = AB.attn_fwd_model(q, k, v, scale)
    reps = [AB.check(f"{name} O", heads(O, Sq), f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2", lse2, f.lse2, f.e_lse2)]
    assert AB.rel_l2(heads(O, Sq), f.O) < 8e-3

    outs = []
    for _ in range(2):
        bufs, (dq, dk, dv), ins = _blocks(B, Sq, Sk, D, self_attn)
        b0 = [_bits(x).clone() for x in bufs]
        ops.attn_wide_bwd(q2, k2, v2, dO2, lse2, dq, dk, dv, B, H, Sq, Sk, d, scale)
        torch.cuda.synchronize()
        for i, (bf, m, bb) in enumerate(zip(bufs, ins, b0)):
            _guard(f"{name} gradient buffer {i}", bf, m, bb)
        outs.append([_bits(x).clone() for x in bufs])
    assert all(torch.equal(a, b) for a, b in zip(*outs)), f"{name}: the backward is not deterministic"
    bw = AWB.add_delta_sum_terms(AB.attn_bwd_model(q, k, v, dO, f.O, lse2, scale), q, k, v, dO, f.O, lse2, f.e_lse2, scale)
    u = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale)          # unchained: the fully fp64 backward
    for n, t, S_ in (("dQ", dq, Sq), ("dK", dk, Sk), ("dV", dv, Sk)):
        reps.append(AB.check(f"{name} {n}", heads(t, S_), getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n)))
        r = AB.rel_l2(heads(t, S_), getattr(u, n))
        print(f"[unchained] {name} {n} rel-L2 {r:.2e}")
        assert r < 2e-2, (name, n, r)
    for rep in reps:
        AB.assert_bound(rep)


@pytest.mark.parametrize("d", [128, 192])
def test_other_head_widths_are_refused_by_name(d):
    from simpletuner_amd import lib, ops
    t = torch.zeros(64, 2 * d, dtype=BF16, device=dev())
    lse = torch.zeros(1, 2, 64, device=dev())
    with pytest.raises(lib.St355Error, match=rf"rc=-38\): attn_wide_fwd: head_dim {d} not built"):          # ST355_ENOSYS
        ops.attn_wide_fwd(t, t, t, torch.empty_like(t), lse, 1, 2, 64, 64, d, 0.1)
    with pytest.raises(lib.St355Error, match=rf"rc=-38\): attn_wide_bwd: head_dim {d} not built"):
        ops.attn_wide_bwd(t, t, t, t, lse, torch.empty_like(t), torch.empty_like(t), torch.empty_like(t), 1, 2, 64, 64, d, 0.1)


def test_sd15_wide_heads_model_with_the_switch_on(monkeypatch):
    """tests/test_unet_model_gpu.py's sd15_wide_heads case (prediction, loss and every parameter gradient vs fp32 autograd, at that file's tolerances) on the fused route"""
    from simpletuner_amd import ops
    from tests import test_unet_model_gpu as UM
    assert UM.SD15_WIDE["block_out_channels"][1] // UM.SD15_WIDE["attention_head_dim"][1] == D_HEAD
    calls = []
    fwd = ops.attn_wide_fwd
    monkeypatch.setattr(ops, "ATTN_WIDE", True)
    monkeypatch.setattr(ops, "attn_wide_fwd", lambda *a, **kw: (calls.append(a[5:9]), fwd(*a, **kw))[1])
    UM.test_unet_full_finetune_gradients_match_autograd("sd15_wide_heads")
    assert len(calls) == 8 and {c[3] for c in calls} == {64, 9}, calls          # self (64 keys) and cross (9 text keys) of the four transformers (down, mid, two up)

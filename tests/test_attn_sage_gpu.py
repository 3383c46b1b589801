"""The quantised attention forward (csrc/attention_sage.hip) against tests/attn_sage_ref.py at the smallest shapes at which indexing, tails and K smoothing
can go wrong: a ragged 64-row block and a half-empty 128-key step (200, 77, 333), nine steps over several workgroups (1088), one key (1), both head dims.
Each shape runs with Gaussian operands and with K carrying +8 on a quarter of its channels (the case smoothing exists for).
  1. the quantisers are bit-equal to the restatement (int8 and e4m3 bytes, fp32 scales), rows / columns >= S zero;
  2. every element of O lies within the bound derived in tests/attn_sage_ref.py of the fp64 attention over the DEQUANTISED operands;
  3. a second launch is bit-identical, and the sentinel bytes around O and around the workspace are untouched."""
import math

import pytest
import torch

from tests import attn_sage_ref as R
from tests.test_attn_bounds_gpu import _bits, _guard, _sent, dev

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SHAPES = [(2, 3, 200, 64), (1, 2, 77, 128), (1, 1, 333, 128), (1, 2, 1088, 64), (1, 1, 1, 64)]


@pytest.mark.parametrize("offset", [False, True], ids=["gauss", "koffset"])
@pytest.mark.parametrize("B,H,S,d", SHAPES)
def test_sage_attention_quantisers_bound_and_determinism(monkeypatch, B, H, S, d, offset):
    from simpletuner_amd import lib, ops
    Sp, scale = (S + 63) // 64 * 64, 1.0 / math.sqrt(d)
    g = torch.Generator().manual_seed(S + d)
    Q, K, V = (torch.randn(B, H, S, d, generator=g) for _ in range(3))
    if offset:
        K[..., : d // 4] += 8.0
    Q, K = Q.to(BF16), K.to(BF16)
    Vt = torch.zeros(B, H, d, Sp, dtype=BF16)
    Vt[..., :S] = V.transpose(2, 3)
    Vt[..., S:] = 7.0          # the pad columns of a caller's V^T are not part of the contract: nothing may depend on them
    need = lib.load().st355_attn_sage_workspace(B, H, S, d)
    ws_buf = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=dev())
    monkeypatch.setattr(ops, "_scratch", lambda name, dv, nbytes, key=(): ws_buf[256:256 + nbytes])

    got = ops.attn_sage_quantize(Q.to(dev()), K.to(dev()), Vt.to(dev()), B, H, S, Sp, d)
    want = R.quantize(Q, K, Vt, S)
    for n, a, b in zip(("Qh", "Kh", "Vh", "sq", "sk", "sv"), got, want):
        bits = torch.int32 if a.dtype == torch.float32 else torch.int8
        assert torch.equal(a.cpu().view(bits), b.view(bits)), f"{n}: {int((a.cpu().view(bits) != b.view(bits)).sum())} of {b.numel()} differ from the restatement"
    assert not bool(got[0][:, :, S:].any()) and not bool(got[1][:, :, S:].any()) and not bool(got[2].view(torch.int8)[..., S:].any())

    O_buf = _sent((B * S + 7, H * d + 32))
    O, before = O_buf[:B * S, :H * d], _bits(O_buf).clone()
    ops.attn_sage_fwd(Q.to(dev()), K.to(dev()), Vt.to(dev()), O, B, H, S, Sp, d, scale)
    torch.cuda.synchronize()
    inside = torch.zeros_like(O_buf, dtype=torch.bool)
    inside[:B * S, :H * d] = True
    _guard("O", O_buf, inside, before)
    first, ws_first = _bits(O_buf).clone(), ws_buf.clone()
    ops.attn_sage_fwd(Q.to(dev()), K.to(dev()), Vt.to(dev()), O, B, H, S, Sp, d, scale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(O_buf), first) and torch.equal(ws_buf, ws_first), "two launches differ"
    assert bool((ws_buf[:256] == 0x5A).all()) and bool((ws_buf[256 + need:] == 0x5A).all()), "bytes around the workspace were written"

    q, k, v = R.dequantize(*want, S)
    ref, S2 = R.attention(q, k, v, scale)
    Oh = O.cpu().double().view(B, S, H, d).permute(0, 2, 1, 3)
    err, bnd = (Oh - ref).abs(), R.bound(ref, S2, v, S)
    exact, _ = R.attention(Q, K, V.to(BF16), scale)
    print(f"B{B} H{H} S{S} d{d} {'koffset' if offset else 'gauss'}: worst err/bound {float((err / bnd).max()):.3f}; against exact attention on the bf16 operands: "
          f"rel-L1 {float((Oh - exact).abs().sum() / exact.abs().sum()):.3e} cosine {float(torch.cosine_similarity(Oh.flatten(), exact.flatten(), 0)):.6f}")
    assert bool(torch.isfinite(Oh).all()) and bool((err <= bnd).all()), f"{int((err > bnd).sum())} elements outside the bound, worst err/bound {float((err / bnd).max()):.3f}"


@pytest.mark.parametrize("what", ["d", "Sp", "dtype", "layout", "device"])
def test_preconditions_are_refused_by_name(what):
    from simpletuner_amd import lib, ops
    B, H, S, Sp, d = 1, 1, 64, 64, 96 if what == "d" else 64
    Q = torch.zeros(B, H, S, d, dtype=BF16, device=dev())
    K, Vt, O = Q.clone(), torch.zeros(B, H, d, Sp, dtype=BF16, device=dev()), torch.zeros(B * S, H * d, dtype=BF16, device=dev())
    if what == "Sp":
        Sp, Vt = 128, torch.zeros(B, H, d, 128, dtype=BF16, device=dev())
    elif what == "dtype":
        K = K.float()
    elif what == "layout":
        Q = Q.transpose(2, 3).contiguous().transpose(2, 3)
    elif what == "device":
        Vt = Vt.cpu()
    msg = {"d": "head_dim 96 not built", "Sp": "Sp 128: expected ceil64", "dtype": "K: expected dtype", "layout": "Q: expected a contiguous", "device": "Vt: expected a device tensor"}
    with pytest.raises(lib.St355Error, match=msg[what]):
        ops.attn_sage_fwd(Q, K, Vt, O, B, H, S, Sp, d, 0.125)

"""k_attn_fwd64x (attn_set_impl fwd = 2: head_dim 64, 64 queries per wave, every bias / O_res / cross form) element-wise against the fp64 model of
tests/attn_bounds.py, at the smallest shapes that cross each boundary of the kernel: one row / one key, one key short of a 64-key tile, exactly a tile, one over
a tile with a second 256-query workgroup, three key tiles with a ragged last one, the 77-key cross-attention shape.  Bounds are the derived ones of
attn_bounds.check / check_lse2, the same as for k_attn_fwd4; data, sentinels and guards are those of tests/test_attn_bounds_gpu.py."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests.test_attn_bounds_gpu import _bits, _data, _guard, _sent, dev

pytestmark = pytest.mark.gpu

B, H, D = 2, 3, 64
SCALE = 1.0 / math.sqrt(D)
SHAPES = [(1, 1), (65, 63), (64, 64), (257, 65), (130, 129), (300, 77)]


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _forward(ops, Sq, Sk, bias, res, kb=None, seed=0):
    """one forward under fwd = 2 into sentinel-filled, over-allocated buffers -> dict of operands, outputs (head-major views) and the guard checks done"""
    g = torch.Generator(device="cuda").manual_seed(1000 * Sq + Sk + seed)
    q, k, v, dO = _data(g, B, H, Sq, Sk, D, D, common=3.0 if (Sq, Sk) == (130, 129) else 0.0, scale=SCALE)
    if bias and kb is None:
        kb = 2.0 * torch.randn(B, Sk, device=dev(), generator=g)
    Skp = (Sk + 63) // 64 * 64
    Vt = torch.zeros(B, H, D, Skp, device=dev(), dtype=torch.bfloat16)
    Vt[..., :Sk] = v.transpose(2, 3)
    rows, cols = B * Sq + 7, H * D + 32
    O_buf, R_buf = _sent((rows, cols)), _sent((rows, cols)) if res else None
    lse_buf = _sent((B * H * Sq + 64,), torch.float32)
    O, R = O_buf[:B * Sq, :H * D], R_buf[:B * Sq, :H * D] if res else None
    lse2 = lse_buf[:B * H * Sq].view(B, H, Sq)
    before = [_bits(x).clone() for x in (O_buf, lse_buf)] + ([_bits(R_buf).clone()] if res else [])
    prev = ops.attn_set_impl(fwd=2)
    try:
        assert ops.attn_plan(B, H, Sq, Sk, D, key_bias=bias, O_res=res)["fwd"] == "fwd64x<64>"
        ops.attn_cross_fwd(q, k, Vt, O, lse2, B, H, Sq, Sk, Skp, D, SCALE, key_bias=kb, O_res=R)
        torch.cuda.synchronize()
    finally:
        ops.attn_set_impl(fwd=prev[0])
    inside = torch.zeros(rows, cols, dtype=torch.bool, device=dev())
    inside[:B * Sq, :H * D] = True
    lin = torch.zeros(B * H * Sq + 64, dtype=torch.bool, device=dev())
    lin[:B * H * Sq] = True
    _guard("O", O_buf, inside, before[0])
    _guard("lse2", lse_buf, lin, before[1])
    if res:
        _guard("O_res", R_buf, inside, before[2])
    hm = lambda t: t.view(B, Sq, H, D).permute(0, 2, 1, 3)
    return dict(q=q, k=k, v=v, dO=dO, kb=kb, Skp=Skp, O=O, R=R, lse2=lse2, Oh=hm(O), Rh=hm(R) if res else None, raw=(O_buf, R_buf, lse_buf))


def _bound(name, r):
    f = AB.attn_fwd_model(r["q"], r["k"], r["v"], SCALE, r["kb"])
    reps = [AB.check(f"{name} O", r["Oh"], f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2", r["lse2"], f.lse2, f.e_lse2)]
    if r["Rh"] is not None:      # O + O_res carries the fp32 output: the fp32-output bound of the existing residual test
        reps.append(AB.check(f"{name} O + O_res", r["Oh"].double() + r["Rh"].double(), f.O, f.e_O + AB.U24 * f.O.abs(), f.var_O, final=f.O - r["Oh"].double()))
    for rep in reps:
        AB.assert_bound(rep)


def test_route(ops):
    prev = ops.attn_set_impl(fwd=2)
    try:
        for bias in (False, True):
            for res in (False, True):
                assert ops.attn_plan(2, 24, 4327, 4327, 64, key_bias=bias, O_res=res)["fwd"] == "fwd64x<64>"
        assert ops.attn_plan(2, 24, 4096, 77, 64, O_res=True)["fwd"] == "fwd64x<64>"
        assert ops.attn_plan(1, 24, 4608, 4608, 128)["fwd"] == "fwd64<128>"
    finally:
        ops.attn_set_impl(fwd=prev[0])
    prev = ops.attn_set_impl(fwd=64)
    try:
        assert ops.attn_plan(2, 24, 4327, 4327, 64)["fwd"] == "fwd4<64>"
    finally:
        ops.attn_set_impl(fwd=prev[0])


@pytest.mark.parametrize("res", [False, True], ids=["", "res"])
@pytest.mark.parametrize("bias", [False, True], ids=["", "bias"])
@pytest.mark.parametrize("Sq,Sk", SHAPES)
def test_fwd_against_fp64(ops, Sq, Sk, bias, res):
    _bound(f"fwd64x Sq{Sq} Sk{Sk} bias{int(bias)} res{int(res)}", _forward(ops, Sq, Sk, bias, res))


def test_bias_all_but_one_key(ops):
    kb = torch.full((B, 130), -10000.0, device=dev())
    kb[0, 7] = 0.0
    kb[1, 129] = 0.0
    r = _forward(ops, 65, 130, True, True, kb=kb)
    assert bool(torch.isfinite(r["Oh"].float()).all() and torch.isfinite(r["Rh"].float()).all() and torch.isfinite(r["lse2"]).all())
    _bound("fwd64x all but one key at -1e4", r)


def test_bit_identical(ops):
    a, b = _forward(ops, 130, 129, True, True), _forward(ops, 130, 129, True, True)
    for x, y in zip(a["raw"], b["raw"]):
        assert torch.equal(_bits(x), _bits(y))


def test_backward_takes_it(ops):
    """the existing backward (O_res form, key bias) on the new forward's O, O_res, lse2: dQ, dK, dV inside attn_bwd_model's bounds"""
    Sq, Sk = 257, 65
    r = _forward(ops, Sq, Sk, True, True)
    plan = ops.attn_plan(B, H, Sq, Sk, D, key_bias=True, O_res=True)
    v_rows = r["v"].permute(0, 2, 1, 3).reshape(B * Sk, H * D).contiguous()
    dO2 = r["dO"].permute(0, 2, 1, 3).reshape(B * Sq, H * D).contiguous()
    dQ, dK = _sent((B, H, Sq, D)), _sent((B, H, Sk, D))
    dv_rows = _sent((B * Sk, H * D))
    ops.attn_cross_bwd(r["q"], r["k"], None, None, v_rows, r["O"], dO2, r["lse2"], dQ, dK, dv_rows, B, H, Sq, (Sq + 63) // 64 * 64, Sk, r["Skp"], D, SCALE,
                       key_bias=r["kb"], O_res=r["R"])
    torch.cuda.synchronize()
    bw = AB.attn_bwd_model(r["q"], r["k"], r["v"], r["dO"], r["Oh"], r["lse2"], SCALE, bias=r["kb"], O_res=r["Rh"],
                           lse_in_chain=plan["dkv"].startswith("dkv4"), tail_from=Sk // 64 * 64 if plan["dq_tail"] else None)
    dVh = dv_rows.view(B, Sk, H, D).permute(0, 2, 1, 3)
    for rep in (AB.check("fwd64x -> dQ", dQ, bw.dQ, bw.e_dQ, bw.var_dQ, extra_round=bw.dQ_part), AB.check("fwd64x -> dK", dK, bw.dK, bw.e_dK, bw.var_dK),
                AB.check("fwd64x -> dV", dVh, bw.dV, bw.e_dV, bw.var_dV)):
        AB.assert_bound(rep)

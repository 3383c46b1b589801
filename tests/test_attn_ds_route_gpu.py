"""The dS-spill attention backward (head_dim 128): k_attn_bwd_dkv4<128, true> writes the packed dS it holds (bf16, fragment-major blocks), k_attn_bwd_dq_ds<128> forms
dQ = scale dS K from it (simpletuner_amd/csrc/attention_bwd.hip, tools/kgen/dkv.py DKV_DS=1).  Every case runs with the switch forced on (ops.attn_set_ds(1): the
default size gate admits only grids of three full rounds) and checks, on the adversarial inputs of tests/test_attn_bounds_gpu.py:
  1. st355_attn_plan reports the _ds routes with the buffer flag, today's routes without it or with the switch at 0;
  2. dK / dV bit-identical to the dkv4 route;
  3. the spill buffer (allocated larger than needed, filled with the bf16 NaN sentinel 0x7FA5): every element inside B H Sk Sqp written, every one outside bit-unchanged;
  4. plain form: dQ against scale dS_spill K in fp64 FROM THE SPILLED BUFFER: |err| <= 2^-8 |ref| + Sk 2^-24 scale sum_k |dS K| (one bf16 rounding + the fp32
     accumulation) — this isolates the new dQ kernel;
  5. dQ (plain) / the dq rows (RoPE form) inside the fp64 bounds of tests/attn_bounds.py exactly as the "flux S4608 rope" case applies them, rel-L2 < 2e-2 against
     the fully fp64 backward;
  6. two runs bit-identical;
  7. a buffer one byte short runs today's route: every output equals the switch-0 result bit for bit and the buffer is not touched.
Shapes: B1 H2 S512 (two 256-key workgroups, eight query tiles, four dQ workgroups per head), B2 H2 S768 (an odd count of 256 tiles), B1 H2 S1024 through the RoPE
form with split = 256 (both norm-weight sets)."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests import test_attn_bounds_gpu as TB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = TB.SENT
D_HEAD = 128


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _case(ops, name, B, H, S, rope, seed):
    d = D_HEAD
    dev = TB.dev()
    scale = 1.0 / math.sqrt(d)
    D = H * d
    tag = "_rope" if rope else ""
    kw = dict(vrows=rope, rope=rope)
    prev = ops.attn_set_ds(1)
    try:
        # 1. the plan
        plan = ops.attn_plan(B, H, S, S, d, ds=True, **kw)
        today = ops.attn_plan(B, H, S, S, d, **kw)
        assert (plan["dkv"], plan["dq"], plan["dq_tail"]) == (f"dkv4{tag}_ds<128>", f"dq_ds{tag}<128>", False), plan
        assert (today["dkv"], today["dq"]) == (f"dkv4{tag}<128>", f"dq64{tag}<128>"), today
        assert {k: plan[k] for k in ("fwd", "prep")} == {k: today[k] for k in ("fwd", "prep")}
        ops.attn_set_ds(0)
        assert ops.attn_plan(B, H, S, S, d, ds=True, **kw) == today
        ops.attn_set_ds(1)

        g = torch.Generator(device="cuda").manual_seed(seed)
        q, k, v, dO = TB._data(g, B, H, S, S, d, d, scale=scale)
        qkv = torch.randn(B * S, 3 * D, device=dev, generator=g).to(BF16)
        v_rows = qkv[:, 2 * D:]
        v_rows.copy_(v.permute(0, 2, 1, 3).reshape(B * S, D))
        dO2 = dO.permute(0, 2, 1, 3).reshape(B * S, D).contiguous()
        O = torch.empty(B * S, D, device=dev, dtype=BF16)
        lse2 = torch.empty(B, H, S, device=dev, dtype=torch.float32)
        if rope:
            ops.attn_fwd_vrows(q, k, v_rows, O, lse2, B, H, S, d, scale)
            gq = torch.Generator(device="cuda").manual_seed(seed + 1000)
            rrms = torch.rand(B * S, 2 * H, device=dev, generator=gq) * 1.5 + 0.5
            w = [(1.0 + 0.2 * torch.randn(128, device=dev, generator=gq)).to(BF16) for _ in range(4)]     # wq_lo, wk_lo, wq_hi, wk_hi
            ang = torch.rand(S, 64, device=dev, generator=gq) * (2 * math.pi)
            cos_p, sin_p = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
            split = 256
        else:
            Vt = v.transpose(2, 3).contiguous()
            ops.attn_fwd(q, k, Vt, O, lse2, B, H, S, S, d, scale)
        Oh = O.view(B, S, H, d).permute(0, 2, 1, 3)

        need = int(ops._l.load().st355_attn_bwd_ds_bytes(B, H, S, S, S, d))
        assert need == B * H * S * S * 2
        extra = 4096

        def backward(mode, ds_bytes):
            """one backward with the switch at `mode` and a fresh sentinel-filled spill buffer announced as ds_bytes bytes -> (dQ, dK, dqkv, buffer) bit tensors"""
            ops.attn_set_ds(mode)
            buf = torch.full((need // 2 + extra,), SENT, dtype=torch.int16, device=dev)
            dQ, dK, dqkv = TB._sent((B, H, S, d)), TB._sent((B, H, S, d)), TB._sent((B * S, 3 * D))
            if rope:
                ops.attn_bwd_rope(q, k, v_rows, O, dO2, lse2, rrms, w[0], w[1], w[2], w[3], split, cos_p, sin_p, dqkv, B, H, S, S, d, scale, ds=buf, ds_bytes=ds_bytes)
            else:
                ops.attn_bwd(q, k, None, None, v_rows, O, dO2, lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, S, d, scale, ds=buf, ds_bytes=ds_bytes)
            torch.cuda.synchronize()
            ops.attn_set_ds(1)
            return TB._bits(dQ), TB._bits(dK), TB._bits(dqkv), buf

        whole = (need // 2 + extra) * 2
        old = backward(0, whole)                       # today's route (the A/B switch), the buffer given but unused
        new = backward(1, whole)
        again = backward(1, whole)
        short = backward(1, need - 1)
        assert bool((old[3] == SENT).all()), f"{name}: switch 0 wrote the spill buffer"
        # 6. deterministic
        for a, b in zip(new, again):
            assert torch.equal(a, b), f"{name}: the spill route is not deterministic"
        # 7. one byte short: today's route, bit for bit, buffer untouched
        for a, b in zip(short[:3], old[:3]):
            assert torch.equal(a, b), f"{name}: a too-small spill buffer did not run today's route"
        assert bool((short[3] == SENT).all()), f"{name}: a too-small spill buffer was written"
        # 2. dK / dV bit-identical to the dkv4 route
        if rope:
            assert torch.equal(new[2][:, D:], old[2][:, D:]), f"{name}: dk rows / dV differ from the dkv4 route"
        else:
            assert torch.equal(new[1], old[1]), f"{name}: dK differs from the dkv4 route"
            assert torch.equal(new[2][:, 2 * D:], old[2][:, 2 * D:]), f"{name}: dV differs from the dkv4 route"
            assert bool((new[2][:, :2 * D] == SENT).all())
        # 3. the spill buffer
        buf = new[3]
        left = int((buf[:need // 2] == SENT).sum())
        assert left == 0, f"{name}: {left} elements of dS^T never written"
        assert bool((buf[need // 2:] == SENT).all()), f"{name}: written behind B H Sk Sqp"
        # fragment-major (attention_bwd.hip): [b, h, key / 32, query / 64, (query % 64) / 16, (query % 16) / 8, key % 32, query % 8] -> [b, h, key, query], unscaled
        dsT = buf[:need // 2].view(BF16).view(B, H, S // 32, S // 64, 4, 2, 32, 8).permute(0, 1, 2, 6, 3, 4, 5, 7).reshape(B, H, S, S).to(AB.F64)

        dQ_new = new[0].view(BF16) if not rope else None
        if not rope:
            # 4. the dQ kernel alone: fp64 product of the spilled dS^T with K
            kk = k.to(AB.F64)
            ref = scale * (dsT.transpose(2, 3) @ kk)
            mag = scale * (dsT.abs().transpose(2, 3) @ kk.abs())
            tol = 2.0 ** -8 * ref.abs() + S * 2.0 ** -24 * mag
            err = (dQ_new.to(AB.F64) - ref).abs()
            ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
            print(f"[ds] {name} dQ vs fp64 scale dS_spill K: worst err/tol {float(ratio.max()):.3f}, max |err| {float(err.max()):.3e}, rel-L2 {AB.rel_l2(dQ_new, ref):.2e}")
            assert float(ratio.max()) <= 1.0, (name, float(ratio.max()))

        # 5. the project's fp64 bounds, as the "flux S4608 rope" case uses them
        bw = AB.attn_bwd_model(q, k, v, dO, Oh, lse2, scale, lse_in_chain=True)
        f = AB.attn_fwd_model(q, k, v, scale)
        u = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale)
        dqkv = new[2].view(BF16)
        dVh = dqkv[:, 2 * D:].reshape(B, S, H, d).permute(0, 2, 1, 3)
        if rope:
            dQ = dqkv[:, :D].reshape(B, S, H, d).permute(0, 2, 1, 3)
            dK = dqkv[:, D:2 * D].reshape(B, S, H, d).permute(0, 2, 1, 3)
            pos = torch.arange(S, device=dev)[:, None] < split
            rr = rrms.view(B, S, 2, H).permute(0, 2, 3, 1)
            wtok = [torch.where(pos, w[i].float()[None], w[i + 2].float()[None])[None, None] for i in (0, 1)]
            want, ee, vv = {}, {}, {}
            for n, z, i in (("dQ", q, 0), ("dK", k, 1)):
                tg, vg = AB.stored_tol_var(getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n))
                want[n], ee[n], vv[n] = AB.rope_norm_bwd_model(getattr(bw, n), tg, vg, z, rr[:, i], wtok[i].expand(B, H, S, 128), cos_p, sin_p)
                setattr(u, n, AB.rope_norm_bwd_model(getattr(u, n), tg, vg, z, rr[:, i], wtok[i].expand(B, H, S, 128), cos_p, sin_p)[0])
            reps = [AB.check(f"{name} dq rows [{plan['dq']}]", dQ, want["dQ"], ee["dQ"], vv["dQ"]),
                    AB.check(f"{name} dk rows [{plan['dkv']}]", dK, want["dK"], ee["dK"], vv["dK"])]
        else:
            dQ, dK = dQ_new, new[1].view(BF16)
            reps = [AB.check(f"{name} dQ [{plan['dq']}]", dQ, bw.dQ, bw.e_dQ, bw.var_dQ), AB.check(f"{name} dK [{plan['dkv']}]", dK, bw.dK, bw.e_dK, bw.var_dK)]
        reps.append(AB.check(f"{name} dV [{plan['dkv']}]", dVh, bw.dV, bw.e_dV, bw.var_dV))
        for n, t in (("dQ", dQ), ("dK", dK), ("dV", dVh)):
            r = AB.rel_l2(t, getattr(u, n))
            print(f"[unchained] {name} {n} rel-L2 {r:.2e}")
            assert r < 2e-2, (name, n, r)
        for rep in reps:
            AB.assert_bound(rep)
    finally:
        ops.attn_set_ds(prev)


def test_ds_route_s512(ops):
    _case(ops, "ds B1 H2 S512", 1, 2, 512, False, 300)


def test_ds_route_s768_odd_tile_count(ops):
    _case(ops, "ds B2 H2 S768", 2, 2, 768, False, 301)


def test_ds_route_rope_s1024(ops):
    _case(ops, "ds B1 H2 S1024 rope", 1, 2, 1024, True, 302)

"""Every attention route, element-wise against an fp64 reference (tests/attn_bounds.py), at the sequence lengths we train.

Each case first asserts the kernels it runs on (ops.attn_plan -> st355_attn_plan: the decision functions the launchers call), then bounds O, lse2, dQ, dK, dV
(and O + O_res where written) element by element and over every (b, h, 64-row tile) block, with the backward chained on the kernel's own O / lse2; the
RoPE route's dq / dk rows are bounded through the RoPE + RMSNorm backward's Jacobian; every case is also held to rel-L2 < 2e-2 against the fully fp64
backward.  Outputs go
into sentinel-filled buffers wider and longer than the contract (ld_o > H d, V / dV inside a fused [B S, 3D] buffer, ld_do != D): everything outside the contract
must be bit-unchanged, nothing inside may still hold the sentinel, zero-padded head channels must come back exactly 0.  Each backward runs twice and must be
bit-identical.  The last test asserts that the cases reached every route of the enumeration below: run the module as a whole."""
import math

import pytest
import torch

from tests import attn_bounds as AB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = 0x7FA5             # int16 bit pattern of the bf16 sentinel (a NaN: no kernel computes it)
SENT_F32 = 0x7FC0DEAD     # int32 bit pattern of the fp32 sentinel (a NaN)
HIT = set()
# the route enumeration (st355_attn_plan names; dq64_tail<d>: dq64 + the tail launch)
ALL_ROUTES = ({"fwd64<96>", "fwd64<128>", "fwd4_vrows<128>", "fwd4_vrows_bias<128>"}
              | {f"{r}<{d}>" for d in (64, 96, 128) for r in ("fwd4", "fwd4_bias", "fwd4_res", "prep", "prep_res", "prep_dot", "dkv4", "dkv3", "dkv2",
                                                          "dq64", "dq_tr", "dq_tr_bias", "dq", "dq_bias")}
              | {"fwd4_res_bias<64>", "dq64_tail<64>", "dq64_tail<96>", "dq64_tail<128>"}
              | {"dkv4_rope<128>", "dkv3_rope<128>", "dq64_rope<128>", "dq_tr_rope<128>", "dq_tr_bias_rope<128>"})


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _sent(shape, dtype=BF16):
    t = torch.empty(shape, dtype=dtype, device=dev())
    if dtype == BF16:
        t.view(torch.int16).fill_(SENT)
    else:
        t.view(torch.int32).fill_(SENT_F32)
    return t


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _guard(name, buf, inside, before_bits):
    """buf: the whole sentinel-filled allocation; inside: bool mask of the contract (same shape)"""
    b = _bits(buf)
    sent = SENT if buf.dtype == BF16 else SENT_F32
    outside_changed = (b != before_bits) & ~inside
    assert not bool(outside_changed.any()), f"{name}: {int(outside_changed.sum())} elements written outside the contract"
    left = (b == sent) & inside
    assert not bool(left.any()), f"{name}: {int(left.sum())} elements of the contract never written"


def _data(g, B, H, Sq, Sk, d, live, common=0.0, adversarial=True, scale=1.0):
    """q [B,H,Sq,d], k [B,H,Sk,d], v [B,H,Sk,d], dO [B,H,Sq,d] fp32 values (rounded to bf16 later), channels >= live zero"""
    q = torch.randn(B, H, Sq, d, device=dev(), generator=g)
    k = torch.randn(B, H, Sk, d, device=dev(), generator=g)
    v = torch.randn(B, H, Sk, d, device=dev(), generator=g)
    dO = torch.randn(B, H, Sq, d, device=dev(), generator=g)
    if common:      # the k / v common component over tokens (test_kernels_gpu.py's UNet case)
        k += common * torch.randn(B, H, 1, d, device=dev(), generator=g)
        v += common * torch.randn(B, H, 1, d, device=dev(), generator=g)
    for t in (q, k, v, dO):
        t[..., live:] = 0
    q, k = q.to(BF16).float(), k.to(BF16).float()
    if adversarial and Sq >= 6 and Sk >= 2:
        nt = (Sk + 63) // 64

        def aim(qrow, nats):      # a key that gives query qrow a score of `nats` (natural units, before the 1/sqrt(d) scale is undone)
            return qrow * (nats / (scale * float((qrow * qrow).sum().clamp_min(1e-6))))

        for b in range(B):
            for h in range(H):
                k[b, h, max(0, Sk - 70)] = aim(q[b, h, 0], 70.0)                  # one late-tile spike of ~70 nats (fwd64's out-of-line re-reference)
                for t in range(min(nt, 64)):                                    # row 1: a max that rises in every tile
                    j = min(Sk - 1, 64 * t + 17)
                    if j != max(0, Sk - 70):
                        k[b, h, j] = aim(q[b, h, 1], 4.0 + 0.5 * t)
                k[b, h, Sk - 1] = aim(q[b, h, 2], 25.0)                           # row 2: the max inside the ragged tail tile
                q[b, h, 3] = 0                                                  # row 3: q = 0, uniform P
                q[b, h, 4] = k[b, h, Sk // 2] * (30.0 / (scale * float((k[b, h, Sk // 2] ** 2).sum().clamp_min(1e-6))))   # row 4: nearly one-hot
    return q.to(BF16), k.to(BF16), v.to(BF16), dO.to(BF16)


def P(fwd, prep, dkv, dq, tail=False):
    """the planned routes a case must run on (ops.attn_plan's dict)"""
    return {"fwd": fwd, "prep": prep, "dkv": dkv, "dq": dq, "dq_tail": tail}


def _run(ops, name, B, H, Sq, Sk, d, expect, live=None, self_attn=True, bias=None, vrows=False, res=False, copies=False, common=0.0, seed=0,
         impl=None, adversarial=True, rope=False, cancels=False):
    """expect: P(...) of every stage.  rope: the backward through st355_attn_bwd_rope (dq / dk / dv into the projection-gradient rows, RoPE + RMSNorm backward
    fused into the dQ / dK epilogues).  cancels: exact arithmetic gives dQ = dK = 0 (one key per query): the unchained check asserts the fp64 reference is 0."""
    live = live or d
    scale = 1.0 / math.sqrt(live)
    plan_kw = dict(key_bias=bias is not None, vrows=vrows, O_res=res, Qt=copies, Kt=copies, rope=rope)
    prev = ops.attn_set_impl(*impl) if impl else None
    try:
        plan = ops.attn_plan(B, H, Sq, Sk, d, **plan_kw)
        assert plan == expect, (name, plan)
        HIT.update({plan["fwd"], plan["prep"], plan["dkv"], plan["dq"]})
        if plan["dq_tail"]:
            HIT.add(plan["dq"].replace("dq64", "dq64_tail"))
        g = torch.Generator(device="cuda").manual_seed(seed)
        q, k, v, dO = _data(g, B, H, Sq, Sk, d, live, common=common, adversarial=adversarial, scale=scale)
        D = H * d
        Sqp, Skp = (Sq + 63) // 64 * 64, (Sk + 63) // 64 * 64
        # V inside a fused [B Sk, 3D] buffer (the QKV projection output), dV inside another; dO with ld_do = D + 64
        qkv = torch.randn(B * Sk, 3 * D, device=dev(), generator=g).to(BF16)
        qkv.view(B * Sk, 3, H, d)[..., live:] = 0
        v_rows = qkv[:, 2 * D:]
        v_rows.copy_(v.permute(0, 2, 1, 3).reshape(B * Sk, D))
        dO_buf = torch.randn(B * Sq, D + 64, device=dev(), generator=g).to(BF16)
        dO2 = dO_buf[:, :D]
        dO2.copy_(dO.permute(0, 2, 1, 3).reshape(B * Sq, D))
        Vt = torch.zeros(B, H, d, Skp, device=dev(), dtype=BF16)
        Vt[..., :Sk] = v.transpose(2, 3)
        Qt = Kt = None
        if copies:
            Qt = torch.zeros(B, H, d, Sqp, device=dev(), dtype=BF16)
            Qt[..., :Sq] = q.transpose(2, 3)
            Kt = torch.zeros(B, H, d, Skp, device=dev(), dtype=BF16)
            Kt[..., :Sk] = k.transpose(2, 3)
        # outputs: sentinel-filled, wider (ld_o = D + 32) and longer (+ 7 rows) than the contract
        O_buf = _sent((B * Sq + 7, D + 32))
        O = O_buf[:B * Sq, :D]
        Ores_buf = _sent((B * Sq + 7, D + 32)) if res else None
        O_res = Ores_buf[:B * Sq, :D] if res else None
        lse_buf = _sent((B * H * Sq + 64,), torch.float32)
        lse2 = lse_buf[:B * H * Sq].view(B, H, Sq)
        bufs0 = {"O": _bits(O_buf).clone(), "lse2": _bits(lse_buf).clone()}
        if res:
            bufs0["O_res"] = _bits(Ores_buf).clone()
        if self_attn and not res:
            if vrows:
                ops.attn_fwd_vrows(q, k, v_rows, O, lse2, B, H, Sk, d, scale, key_bias=bias)
            else:
                ops.attn_fwd(q, k, Vt, O, lse2, B, H, Sk, Skp, d, scale, key_bias=bias)
        else:
            ops.attn_cross_fwd(q, k, Vt, O, lse2, B, H, Sq, Sk, Skp, d, scale, key_bias=bias, O_res=O_res)
        torch.cuda.synchronize()
        inside = torch.zeros(B * Sq + 7, D + 32, dtype=torch.bool, device=dev())
        inside[:B * Sq, :D] = True
        _guard(f"{name} O", O_buf, inside, bufs0["O"])
        if res:
            _guard(f"{name} O_res", Ores_buf, inside, bufs0["O_res"])
        lin = torch.zeros(B * H * Sq + 64, dtype=torch.bool, device=dev())
        lin[:B * H * Sq] = True
        _guard(f"{name} lse2", lse_buf, lin, bufs0["lse2"])
        Oh = O.view(B, Sq, H, d).permute(0, 2, 1, 3)
        assert bool((Oh[..., live:] == 0).all()), f"{name}: padded channels of O are not 0"

        f = AB.attn_fwd_model(q, k, v, scale, bias)
        reps = [AB.check(f"{name} O [{plan['fwd']}]", Oh, f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2 [{plan['fwd']}]", lse2, f.lse2, f.e_lse2)]
        assert AB.rel_l2(Oh, f.O) < 8e-3
        Rh = None
        if res:
            Rh = O_res.view(B, Sq, H, d).permute(0, 2, 1, 3)
            assert bool((Rh[..., live:] == 0).all()), f"{name}: padded channels of O_res are not 0"
            # O + O_res carries the fp32 output acc / l (one fp32 rounding, u |O|): the same model as O, with the final RNE that of the residual
            reps.append(AB.check(f"{name} O + O_res [{plan['fwd']}]", Oh.double() + Rh.double(), f.O, f.e_O + AB.U24 * f.O.abs(), f.var_O,
                                 final=f.O - Oh.double()))

        # backward, twice: bit-identical.  dQ / dK head-major with a guard tail (rope: q / k blocks of the projection-gradient rows); dV inside a fused
        # [B Sk, 3D] buffer
        if rope:
            gq = torch.Generator(device="cuda").manual_seed(seed + 1000)
            rrms = torch.rand(B * Sk, 2 * H, device=dev(), generator=gq) * 1.5 + 0.5
            w = [(1.0 + 0.2 * torch.randn(128, device=dev(), generator=gq)).to(BF16) for _ in range(4)]     # wq_lo, wk_lo, wq_hi, wk_hi
            ang = torch.rand(Sk, 64, device=dev(), generator=gq) * (2 * math.pi)
            cos_p, sin_p = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
            split = min(512, Sk)
        outs = []
        for rep_i in range(2):
            dQ_buf = _sent((B * H * Sq * d + 256,))
            dK_buf = _sent((B * H * Sk * d + 256,))
            dqkv = _sent((B * Sk + 5, 3 * D + 64))
            dQ = dQ_buf[:B * H * Sq * d].view(B, H, Sq, d)
            dK = dK_buf[:B * H * Sk * d].view(B, H, Sk, d)
            dv_rows = dqkv[:B * Sk, 2 * D:3 * D]
            b0 = [_bits(x).clone() for x in (dQ_buf, dK_buf, dqkv)]
            vin = torch.zeros(B * Sk + 5, 3 * D + 64, dtype=torch.bool, device=dev())
            if rope:
                ops.attn_bwd_rope(q, k, v_rows, O, dO2, lse2, rrms, w[0], w[1], w[2], w[3], split, cos_p, sin_p, dqkv[:B * Sk, :3 * D], B, H, Sk, Skp, d,
                                  scale, key_bias=bias)
                vin[:B * Sk, :3 * D] = True
            elif self_attn and not res:
                ops.attn_bwd(q, k, Qt, Kt, v_rows, O, dO2, lse2, dQ, dK, dv_rows, B, H, Sk, Skp, d, scale, key_bias=bias)
                vin[:B * Sk, 2 * D:3 * D] = True
            else:
                ops.attn_cross_bwd(q, k, Qt, Kt, v_rows, O, dO2, lse2, dQ, dK, dv_rows, B, H, Sq, Sqp, Sk, Skp, d, scale, key_bias=bias, O_res=O_res)
                vin[:B * Sk, 2 * D:3 * D] = True
            torch.cuda.synchronize()
            qin = torch.zeros_like(dQ_buf, dtype=torch.bool)
            kin = torch.zeros_like(dK_buf, dtype=torch.bool)
            if not rope:
                qin[:B * H * Sq * d] = True
                kin[:B * H * Sk * d] = True
            _guard(f"{name} dQ", dQ_buf, qin, b0[0])
            _guard(f"{name} dK", dK_buf, kin, b0[1])
            _guard(f"{name} dqkv rows", dqkv, vin, b0[2])
            outs.append((dQ_buf.clone(), dK_buf.clone(), dqkv.clone()))
        for a, b in zip(*outs):
            assert torch.equal(_bits(a), _bits(b)), f"{name}: the backward is not deterministic"
        if rope:
            dQ = dqkv[:B * Sk, :D].reshape(B, Sk, H, d).permute(0, 2, 1, 3)
            dK = dqkv[:B * Sk, D:2 * D].reshape(B, Sk, H, d).permute(0, 2, 1, 3)
        dVh = dv_rows.reshape(B, Sk, H, d).permute(0, 2, 1, 3)
        for n, t in (("dQ", dQ), ("dK", dK), ("dV", dVh)):
            assert bool((t[..., live:] == 0).all()), f"{name}: padded channels of {n} are not 0"

        tail_from = Sk // 64 * 64 if plan["dq_tail"] else None
        lse_in_chain = plan["dkv"].startswith("dkv4")
        bw = AB.attn_bwd_model(q, k, v, dO, Oh, lse2, scale, bias=bias, O_res=Rh, lse_in_chain=lse_in_chain, tail_from=tail_from)
        u = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale, bias=bias)      # unchained: the fully fp64 backward (fp64 O, no O_res)
        dq_name = plan["dq"] + (" + tail" if plan["dq_tail"] else "")
        if rope:
            # dQ / dK leave through the RoPE + RMSNorm backward: the stored-dQ / dK bound carried through the epilogue's Jacobian in fp64
            pos = torch.arange(Sk, device=dev())[:, None] < split
            rr = rrms.view(B, Sk, 2, H).permute(0, 2, 3, 1)            # [B, 2, H, S]
            wtok = [torch.where(pos, w[i].float()[None], w[i + 2].float()[None])[None, None] for i in (0, 1)]   # q, k: [1, 1, S, 128]
            want, ee, vv = {}, {}, {}
            for n, z, i in (("dQ", q, 0), ("dK", k, 1)):
                tg, vg = AB.stored_tol_var(getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n))
                want[n], ee[n], vv[n] = AB.rope_norm_bwd_model(getattr(bw, n), tg, vg, z, rr[:, i], wtok[i].expand(B, H, Sk, 128), cos_p, sin_p)
                u_n = AB.rope_norm_bwd_model(getattr(u, n), tg, vg, z, rr[:, i], wtok[i].expand(B, H, Sk, 128), cos_p, sin_p)[0]
                setattr(u, n, u_n)
            reps += [AB.check(f"{name} dq rows [{dq_name}]", dQ, want["dQ"], ee["dQ"], vv["dQ"]),
                     AB.check(f"{name} dk rows [{plan['dkv']}]", dK, want["dK"], ee["dK"], vv["dK"])]
        else:
            reps += [AB.check(f"{name} dQ [{dq_name}]", dQ, bw.dQ, bw.e_dQ, bw.var_dQ, extra_round=bw.dQ_part),
                     AB.check(f"{name} dK [{plan['dkv']}]", dK, bw.dK, bw.e_dK, bw.var_dK)]
        reps.append(AB.check(f"{name} dV [{plan['dkv']}]", dVh, bw.dV, bw.e_dV, bw.var_dV))
        # unchained: against the fully fp64 backward, at the suite's constant, every case
        for n, t in (("dQ", dQ), ("dK", dK), ("dV", dVh)):
            ref = getattr(u, n)
            if cancels and n != "dV":
                big = float(ref.abs().max())
                print(f"[unchained] {name} {n}: fp64 reference max |.| {big:.1e} (cancels exactly)")
                assert big < 1e-12, (name, n, big)
                continue
            r = AB.rel_l2(t, ref)
            print(f"[unchained] {name} {n} rel-L2 {r:.2e}")
            assert r < 2e-2, (name, n, r)
        for rep in reps:
            AB.assert_bound(rep)
        return plan
    finally:
        if prev is not None:
            ops.attn_set_impl(*prev)


def _text_bias(B, Sk, ntext):
    """the masked-training key bias: +1 over the text keys, 0 over the image keys"""
    kb = torch.zeros(B, Sk, device=dev())
    kb[:, :ntext] = 1.0
    return kb


# ---- production shapes ------------------------------------------------------------------------------------------------------------------------------------
def test_flux_rope(ops):
    """the Flux training backward: st355_attn_bwd_rope (fused RoPE + RMSNorm backward), row-major V in the forward, S = 4096 + 512"""
    _run(ops, "flux S4608 rope", 1, 2, 4608, 4608, 128, P("fwd4_vrows<128>", "prep<128>", "dkv4_rope<128>", "dq64_rope<128>"), vrows=True, rope=True, seed=90)
    _run(ops, "flux S4608 rope text bias", 1, 2, 4608, 4608, 128, P("fwd4_vrows_bias<128>", "prep<128>", "dkv3_rope<128>", "dq_tr_bias_rope<128>"),
         vrows=True, rope=True, bias=_text_bias(1, 4608, 512), seed=91)
    _run(ops, "impl32 S1024 rope", 1, 2, 1024, 1024, 128, P("fwd4_vrows<128>", "prep<128>", "dkv3_rope<128>", "dq_tr_rope<128>"), vrows=True, rope=True,
         impl=(32, 32, 3), seed=92)


def test_flux_vrows(ops):
    _run(ops, "flux S4608 vrows", 1, 2, 4608, 4608, 128, P("fwd4_vrows<128>", "prep<128>", "dkv4<128>", "dq64<128>"), vrows=True)


def test_flux_fwd64(ops):
    _run(ops, "flux S4608", 2, 1, 4608, 4608, 128, P("fwd64<128>", "prep<128>", "dkv4<128>", "dq64<128>"), seed=1)


def test_flux_masked_bias(ops):
    kb = _text_bias(1, 4608, 512)
    _run(ops, "flux S4608 text bias vrows", 1, 2, 4608, 4608, 128, P("fwd4_vrows_bias<128>", "prep<128>", "dkv3<128>", "dq_tr_bias<128>"), bias=kb,
         vrows=True, seed=2)
    _run(ops, "flux S4608 text bias", 1, 2, 4608, 4608, 128, P("fwd4_bias<128>", "prep<128>", "dkv3<128>", "dq_tr_bias<128>"), bias=kb, seed=3)


def test_sd3(ops):
    _run(ops, "sd3 S4327", 1, 2, 4327, 4327, 64, P("fwd4<64>", "prep<64>", "dkv4<64>", "dq64<64>", True), seed=4)
    _run(ops, "sd3 bucket S3274", 2, 1, 3120 + 154, 3120 + 154, 64, P("fwd4<64>", "prep<64>", "dkv4<64>", "dq64<64>", True), seed=5)


def test_sdxl_res(ops):
    for S in (4096, 1024):
        _run(ops, f"sdxl S{S} O_res", 1, 2, S, S, 64, P("fwd4_res<64>", "prep_res<64>", "dkv4<64>", "dq64<64>"), res=True, common=3.0, seed=6)


def test_sdxl_cross77(ops):
    _run(ops, "sdxl cross Sk77", 2, 2, 1024, 77, 64, P("fwd4_res<64>", "prep_res<64>", "dkv4<64>", "dq_tr<64>"), self_attn=False, res=True, seed=7)


def test_sd15_padded_heads(ops):
    _run(ops, "sd1.5 head 40->64 S4096", 1, 2, 4096, 4096, 64, P("fwd4<64>", "prep<64>", "dkv4<64>", "dq64<64>"), live=40, seed=8)
    _run(ops, "sd1.5 head 80->96 S1024", 2, 2, 1024, 1024, 96, P("fwd64<96>", "prep<96>", "dkv4<96>", "dq64<96>"), live=80, seed=9)


def test_pixart_2k(ops):
    _run(ops, "pixart 2K S16384 head 72->96", 1, 2, 16384, 16384, 96, P("fwd64<96>", "prep<96>", "dkv4<96>", "dq64<96>"), live=72, seed=10)


def test_pixart_cross300(ops):
    kb = torch.zeros(2, 300, device=dev())
    kb[0, 120:] = -10000.0       # padded T5 tokens
    kb[1, 250:] = -10000.0
    _run(ops, "pixart cross Sk300 bias copies", 2, 2, 1024, 300, 96, P("fwd4_bias<96>", "prep_dot<96>", "dkv2<96>", "dq_bias<96>"), live=72,
         self_attn=False, bias=kb, copies=True, seed=11)
    _run(ops, "pixart cross Sk300 copies", 2, 2, 1024, 300, 96, P("fwd4<96>", "prep_dot<96>", "dkv2<96>", "dq<96>"), live=72, self_attn=False,
         copies=True, seed=12)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 17, 63, 64, 65])
def test_short_self(ops, S):
    """S < 64: general dQ; 64: dq64; 65: a short ragged key axis, general dQ in one pass"""
    dq = "dq64<64>" if S == 64 else "dq_tr<64>"
    _run(ops, f"edge S{S}", 2, 2, S, S, 64, P("fwd4<64>", "prep<64>", "dkv4<64>", dq), seed=20 + S, cancels=S == 1)


def test_ragged_keys(ops):
    """Sk in [64, 128) ragged: the short-ragged general dQ; Sk = 128 + 1: dq64 + a one-key tail"""
    _run(ops, "edge Sk100 d128", 1, 2, 300, 100, 128, P("fwd4_res<128>", "prep_res<128>", "dkv4<128>", "dq_tr<128>"), self_attn=False, res=True, seed=30)
    _run(ops, "edge Sk100 d96", 1, 2, 300, 100, 96, P("fwd4<96>", "prep<96>", "dkv4<96>", "dq_tr<96>"), live=80, self_attn=False, seed=31)
    _run(ops, "edge Sk129 d128", 1, 2, 300, 129, 128, P("fwd4_res<128>", "prep_res<128>", "dkv4<128>", "dq64<128>", True), self_attn=False, res=True,
         seed=32)
    _run(ops, "edge Sk129 d96", 1, 2, 300, 129, 96, P("fwd4<96>", "prep<96>", "dkv4<96>", "dq64<96>", True), live=80, self_attn=False, seed=33)


def test_ragged_query_workgroup(ops):
    _run(ops, "edge Sq257 Sk256 d128", 2, 1, 257, 256, 128, P("fwd4_res<128>", "prep_res<128>", "dkv4<128>", "dq64<128>"), self_attn=False, res=True,
         seed=40)
    _run(ops, "edge S257 d96", 1, 2, 257, 257, 96, P("fwd4<96>", "prep<96>", "dkv4<96>", "dq64<96>", True), live=80, seed=41)


def test_cross_extremes(ops):
    _run(ops, "edge Sq17 Sk1000", 2, 2, 17, 1000, 64, P("fwd4_res<64>", "prep_res<64>", "dkv4<64>", "dq64<64>", True), self_attn=False, res=True, seed=50)
    _run(ops, "edge Sq2000 Sk70", 2, 2, 2000, 70, 64, P("fwd4_res<64>", "prep_res<64>", "dkv4<64>", "dq_tr<64>"), self_attn=False, res=True, seed=51)


def test_bias_all_but_one_key(ops):
    kb = torch.full((2, 300), -10000.0, device=dev())
    kb[0, 7] = 0.0
    kb[1, 299] = 0.0
    _run(ops, "bias -10000 but one key d64", 2, 2, 200, 300, 64, P("fwd4_bias<64>", "prep<64>", "dkv3<64>", "dq_tr_bias<64>"), self_attn=False, bias=kb,
         seed=60, adversarial=False, cancels=True)
    _run(ops, "bias -10000 but one key res", 2, 2, 200, 300, 64, P("fwd4_res_bias<64>", "prep_res<64>", "dkv3<64>", "dq_tr_bias<64>"), self_attn=False,
         bias=kb, res=True, seed=61, adversarial=False, cancels=True)


def test_remaining_routes(ops):
    """the 32-row kernels (attn_set_impl 32 / 32 / 3), the bias / copy forms at every head_dim"""
    _run(ops, "impl32 S1024 d128", 1, 2, 1024, 1024, 128, P("fwd4<128>", "prep<128>", "dkv3<128>", "dq_tr<128>"), impl=(32, 32, 3), seed=70)
    _run(ops, "impl32 S1024 d96", 1, 2, 1024, 1024, 96, P("fwd4<96>", "prep<96>", "dkv3<96>", "dq_tr<96>"), live=80, impl=(32, 32, 3), seed=71)
    _run(ops, "impl32 S1024 d64", 1, 2, 1024, 1024, 64, P("fwd4<64>", "prep<64>", "dkv3<64>", "dq_tr<64>"), impl=(32, 32, 3), seed=72)
    for d, live in ((64, 64), (96, 80), (128, 128)):
        kb = _text_bias(1, 640, 77)
        t = f"<{d}>"
        _run(ops, f"bias S640 d{d}", 1, 2, 640, 640, d, P("fwd4_bias" + t, "prep" + t, "dkv3" + t, "dq_tr_bias" + t), live=live, bias=kb, seed=73 + d)
        fwd = "fwd4<64>" if d == 64 else "fwd64" + t
        _run(ops, f"copies S640 d{d}", 1, 2, 640, 640, d, P(fwd, "prep_dot" + t, "dkv2" + t, "dq" + t), live=live, copies=True, seed=74 + d)
        _run(ops, f"copies bias S640 d{d}", 1, 2, 640, 640, d, P("fwd4_bias" + t, "prep_dot" + t, "dkv2" + t, "dq_bias" + t), live=live, copies=True,
             bias=kb, seed=75 + d)
        _run(ops, f"res S1000 d{d}", 1, 2, 1000, 1000, d, P("fwd4_res" + t, "prep_res" + t, "dkv4" + t, "dq64" + t, True), live=live, res=True, seed=76 + d)
    _run(ops, "res bias S640 d64", 1, 2, 640, 640, 64, P("fwd4_res_bias<64>", "prep_res<64>", "dkv3<64>", "dq_tr_bias<64>"), res=True,
         bias=_text_bias(1, 640, 77), seed=80)
    _run(ops, "S4097 d128 dq64 + tail", 1, 2, 4097, 4097, 128, P("fwd4<128>", "prep<128>", "dkv4<128>", "dq64<128>", True), seed=81)
    _run(ops, "S1000 d96 dq64 + tail", 1, 2, 1000, 1000, 96, P("fwd4<96>", "prep<96>", "dkv4<96>", "dq64<96>", True), live=80, seed=82)


def test_every_route_reached():
    missing = ALL_ROUTES - HIT
    assert not missing, f"routes no case reached: {sorted(missing)} (run the module as a whole)"

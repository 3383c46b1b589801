"""The attention bound checker (tests/attn_bounds.py) bites: on CPU emulations of the kernels' rounding points (fp32 scores, online softmax over 64-key tiles,
P / dS packed to bf16 by RNE, one RNE per stored output), a correctly rounded result passes it, and each modelled kernel defect fails it while the suite's
existing global rel-L2 check for that output (O < 8e-3, dQ / dK / dV < 2e-2) still passes."""
import math

import pytest
import torch

from tests import attn_bounds as AB

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634


def _bf(x):
    return x.float().to(BF16).float()


def _trunc_bf(x):
    """bf16 rounding toward zero (the 'P rounded toward zero' defect)"""
    return (x.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def _data(B, H, Sq, Sk, d, seed, live=None, common=0.0, head_corr=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, d, generator=g)
    k = torch.randn(B, H, Sk, d, generator=g)
    v = torch.randn(B, H, Sk, d, generator=g)
    dO = torch.randn(B, H, Sq, d, generator=g)
    if common:      # the k / v common component over tokens (test_kernels_gpu.py's UNet case)
        k = k + common * torch.randn(B, H, 1, d, generator=g)
        v = v + common * torch.randn(B, H, 1, d, generator=g)
    if head_corr is not None:      # head 1 = head 0 + a small perturbation
        for t in (q, k, v, dO):
            t[:, 1] = t[:, 0] + head_corr * torch.randn(t[:, 0].shape, generator=g)
    if live is not None:
        for t in (q, k, v, dO):
            t[..., live:] = 0
    return _bf(q), _bf(k), _bf(v), _bf(dO)


def emu_fwd(q, k, v, scale, bias=None, skip_alpha=None, round_p=_bf, drop_tail_head=None, bias_shift=0):
    """k_attn_fwd4's arithmetic in fp32: 64-key tiles, running max, P packed to bf16 for PV, l from the fp32 P.  Returns (O bf16 values, lse2 fp32).
    skip_alpha = (tile, rows): the rescale of the accumulator skipped in that tile for those query rows; drop_tail_head: the ragged last key tile skipped for
    that head; bias_shift: the key bias read that many keys off (clamped)."""
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    scale2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)) * scale2
    if bias is not None:
        idx = (torch.arange(Sk) + bias_shift).clamp(0, Sk - 1)
        s = s + (bias[:, idx] * torch.tensor(LOG2E, dtype=torch.float32))[:, None, None, :]
    acc = torch.zeros(B, H, Sq, d)
    m = torch.full((B, H, Sq, 1), -math.inf)
    l = torch.zeros(B, H, Sq, 1)
    nt = (Sk + 63) // 64
    for t in range(nt):
        sl = slice(64 * t, min(Sk, 64 * t + 64))
        st = s[..., sl]
        if drop_tail_head is not None and t == nt - 1 and Sk % 64:
            st = st.clone()
            st[:, drop_tail_head] = -math.inf
        m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - m_new)
        if skip_alpha is not None and t == skip_alpha[0]:
            alpha = alpha.clone()
            alpha[:, :, skip_alpha[1]] = 1.0
        acc = acc * alpha
        p = torch.exp2(st - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc + round_p(p) @ v[..., sl, :]
        m = m_new
    O = _bf(acc / l)
    return O, (m + torch.log2(l))[..., 0]


def emu_bwd(q, k, v, dO, O, lse2, scale, bias=None, tail=None, delta_shift=None, prescale_k=False, dk_wrong_head=None):
    """the backward kernels' arithmetic in fp32: P from the stored lse2, dP = dO v, delta = sum O dO, dS = P (dP - delta); P and dS packed to bf16.
    tail = (first tail key, mode): dq64 + tail (mode 'ok' / 'twice' / 'none').  delta_shift = (head, rows): delta taken from the next query row there.
    prescale_k: the old dkv4 arithmetic (K pre-scaled by scale2 and re-rounded to bf16) for dK / dV.  dk_wrong_head = (key tile): that 64-key tile of dK in
    head 0 taken from head 1."""
    scale2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    Sk = k.shape[2]
    s = q @ k.transpose(-1, -2)
    s2 = s * scale2
    if bias is not None:
        s2 = s2 + (bias * torch.tensor(LOG2E, dtype=torch.float32))[:, None, None, :]
    p = torch.exp2(s2 - lse2[..., None])
    dp = dO @ v.transpose(-1, -2)
    delta = (O * dO).sum(-1, keepdim=True)
    delta_q = delta
    if delta_shift is not None:
        h, rows = delta_shift
        delta_q = delta.clone()
        delta_q[:, h, rows] = delta[:, h, [min(r + 1, q.shape[2] - 1) for r in rows]]
    ds_q = _bf(p * (dp - delta_q))
    if prescale_k:
        p_kv = torch.exp2(q @ _bf(k * scale2).transpose(-1, -2) - lse2[..., None])
    else:
        p_kv = p
    ds_kv = _bf(p_kv * (dp - delta))
    dV = _bf(_bf(p_kv).transpose(-1, -2) @ dO)
    dK = _bf((ds_kv.transpose(-1, -2) @ q) * scale)
    if dk_wrong_head is not None:
        sl = slice(64 * dk_wrong_head, 64 * dk_wrong_head + 64)
        dK[:, 0, sl] = dK[:, 1, sl]
    if tail is None:
        dQ = _bf((ds_q @ k) * scale)
    else:
        t0, mode = tail
        part = _bf((ds_q[..., :t0] @ k[:, :, :t0]) * scale)
        rest = (ds_q[..., t0:] @ k[:, :, t0:]) * scale
        dQ = {"ok": _bf(part + rest), "twice": _bf(_bf(part + rest) + rest), "none": part}[mode]
    return dQ, dK, dV


def _fwd_ref(q, k, v, scale, bias=None):
    return AB.attn_fwd_model(q, k, v, scale, bias)


def _verdict(name, out, want, e, var, old_bar, extra_round=None):
    rep = AB.check(name, out, want, e, var, extra_round=extra_round, verbose=False)
    rel = AB.rel_l2(out, want)
    print(f"[mutation] {name}: new checker {'PASS' if rep.ok else 'FAIL'} (worst err/tol {rep.worst:.2f}, block stat {rep.block_stat:.2f}), "
          f"old rel-L2 {rel:.2e} (bar {old_bar:.0e})")
    return rep, rel


def _case(d, Sq=333, Sk=333, H=2, seed=1, **kw):
    live = 80 if d == 96 else None
    q, k, v, dO = _data(1, H, Sq, Sk, d, seed, live=live, **kw)
    return q, k, v, dO, 1.0 / math.sqrt(d)


@pytest.mark.parametrize("d", [64, 96])
def test_exact_plus_one_rne_passes(d):
    """the checker itself: the fp64 result rounded once to bf16 passes with room to spare"""
    q, k, v, dO, scale = _case(d)
    f = _fwd_ref(q, k, v, scale)
    rep = AB.check(f"exact+RNE O d{d}", _bf(f.O), f.O, f.e_O, f.var_O)
    AB.assert_bound(rep)
    assert rep.block_stat < 1.2
    b = AB.attn_bwd_model(q, k, v, dO, f.O, f.lse2, scale)
    for n in ("dQ", "dK", "dV"):
        AB.assert_bound(AB.check(f"exact+RNE {n} d{d}", _bf(getattr(b, n)), getattr(b, n), getattr(b, "e_" + n), getattr(b, "var_" + n)))


@pytest.mark.parametrize("d", [64, 96])
def test_emulated_kernels_pass(d):
    """the emulated kernel arithmetic (forward, chained backward, dq64 + tail) passes the element and block bounds"""
    q, k, v, dO, scale = _case(d)
    g = torch.Generator().manual_seed(9)
    bias = torch.where(torch.rand(1, 333, generator=g) < 0.2, torch.tensor(-10000.0), torch.tensor(0.0))
    bias[:, :50] = 1.0
    for kb in (None, bias):
        O, lse2 = emu_fwd(q, k, v, scale, bias=kb)
        f = _fwd_ref(q, k, v, scale, kb)
        AB.assert_bound(AB.check(f"emulated O d{d} bias={kb is not None}", O, f.O, f.e_O, f.var_O))
        AB.assert_bound(AB.check_lse2(f"emulated lse2 d{d}", lse2, f.lse2, f.e_lse2))
        dQ, dK, dV = emu_bwd(q, k, v, dO, O, lse2, scale, bias=kb, tail=(320, "ok"))
        b = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale, bias=kb, tail_from=320)
        AB.assert_bound(AB.check("emulated dQ (dq64 + tail)", dQ, b.dQ, b.e_dQ, b.var_dQ, extra_round=b.dQ_part))
        AB.assert_bound(AB.check("emulated dK", dK, b.dK, b.e_dK, b.var_dK))
        AB.assert_bound(AB.check("emulated dV", dV, b.dV, b.e_dV, b.var_dV))


def _fwd_defect(name, d, old=8e-3, data_kw=None, bias=None, **defect):
    q, k, v, dO, scale = _case(d, **(data_kw or {}))
    f = _fwd_ref(q, k, v, scale, bias)
    O, _ = emu_fwd(q, k, v, scale, bias=bias, **defect)
    rep, rel = _verdict(f"{name} d{d}", O, f.O, f.e_O, f.var_O, old)
    assert rel < old and not rep.ok


def _bwd_defect(name, d, which, old=2e-2, data_kw=None, Sq=333, Sk=333, H=2, tail_from=None, lse_in_chain=False, **defect):
    q, k, v, dO, scale = _case(d, Sq=Sq, Sk=Sk, H=H, **(data_kw or {}))
    O, lse2 = emu_fwd(q, k, v, scale)
    out = dict(zip(("dQ", "dK", "dV"), emu_bwd(q, k, v, dO, O, lse2, scale, **defect)))
    b = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale, tail_from=tail_from, lse_in_chain=lse_in_chain)
    extra = b.dQ_part if which == "dQ" else None
    rep, rel = _verdict(f"{name} d{d}", out[which], getattr(b, which), getattr(b, "e_" + which), getattr(b, "var_" + which), old, extra_round=extra)
    assert rel < old and not rep.ok
    return rep


@pytest.mark.parametrize("d", [64, 96])
def test_skipped_alpha_rescale_fails(d):
    """the rescale factor alpha skipped in one tile for the rows whose running max rises there (a late key lifts 2 rows' max a little)"""
    q, k, v, dO, scale = _case(d)
    rows = [0, 1]
    k[:, :, 300] = _bf(q[:, :, :2].mean(2) * 0.5)
    f = _fwd_ref(q, k, v, scale)
    O, _ = emu_fwd(q, k, v, scale, skip_alpha=(4, rows))
    rep, rel = _verdict(f"alpha skipped in tile 4, 2 rows d{d}", O, f.O, f.e_O, f.var_O, 8e-3)
    assert rel < 8e-3 and not rep.ok


@pytest.mark.parametrize("d", [64, 96])
def test_p_rounded_toward_zero_fails(d):
    """with a k / v common component the output sits near that component, and the weights' systematic shortfall (sum_j bf16_rz(P_j) / l < 1) shows"""
    _fwd_defect("P rounded toward zero", d, round_p=_trunc_bf, data_kw={"common": 3.0})


@pytest.mark.parametrize("d", [64, 96])
def test_key_bias_one_key_off_fails(d):
    bias = torch.zeros(1, 333)
    bias[:, :77] = 1.0          # the masked-training bias: +1 over the text keys; one key (76) gets the wrong bias
    _fwd_defect("key bias read one key off", d, bias=bias, bias_shift=1, data_kw={"common": 3.0})


def test_ragged_tail_tile_dropped_for_one_head_fails():
    """dQ of the dq64 + tail route when the tail launch skips head 0 (Sk = 4096 + 1: a one-key ragged tile, four heads)"""
    q, k, v, dO, scale = _case(64, Sq=128, Sk=4097, H=4)
    O, lse2 = emu_fwd(q, k, v, scale)
    dQ, _, _ = emu_bwd(q, k, v, dO, O, lse2, scale, tail=(4096, "ok"))
    dQn, _, _ = emu_bwd(q, k, v, dO, O, lse2, scale, tail=(4096, "none"))
    dQ[:, 0] = dQn[:, 0]
    b = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale, tail_from=4096)
    rep, rel = _verdict("ragged key tile dropped in head 0's dQ (Sk 4097, H 4)", dQ, b.dQ, b.e_dQ, b.var_dQ, 2e-2, extra_round=b.dQ_part)
    assert rel < 2e-2 and not rep.ok


@pytest.mark.parametrize("mode", ["twice", "none"])
def test_dq_tail_twice_or_never_fails(mode):
    """dq64 + tail with the one-key tail tile (Sk = 4096 + 1) added twice or not at all"""
    _bwd_defect(f"dQ tail {mode}", 64, "dQ", Sq=128, Sk=4097, H=2, tail_from=4096, tail=(4096, mode))


@pytest.mark.parametrize("d", [64, 96])
def test_delta_from_neighbouring_row_fails(d):
    """delta of query row i + 1 used for row i over 2 rows of the ragged last query tile of head 1"""
    _bwd_defect("delta from the next row, 2 rows", d, "dQ", delta_shift=(1, [320, 321]))


@pytest.mark.parametrize("d", [64, 96])
def test_dk_tile_from_wrong_head_fails(d):
    """one 64-key tile of head 0's dK taken from head 1, where the two heads' inputs agree to 2 %"""
    _bwd_defect("dK tile 2 from head 1", d, "dK", data_kw={"head_corr": 0.02}, dk_wrong_head=2)


@pytest.mark.parametrize("lse_in_chain", [True, False])
@pytest.mark.parametrize("which", ["dK", "dV"])
def test_prescaled_k_rerounding_fails_either_route(lse_in_chain, which):
    """K pre-scaled by scale2 and re-rounded to bf16 (the first dkv4 version, tools/kgen/dkv.py) fails the dkv4 model (lse_in_chain) and the dkv3 / dkv2 one"""
    _bwd_defect(f"K pre-scaled + re-rounded, lse_in_chain={lse_in_chain}", 64, which, prescale_k=True, lse_in_chain=lse_in_chain,
                data_kw={"common": 3.0})


def test_dkv4_term_is_route_specific():
    """the dkv4 chain term widens the dK / dV bound of that route only, by (d + 3) u |lse2| in the exponent"""
    q, k, v, dO, scale = _case(128, Sq=200, Sk=200)
    O, lse2 = emu_fwd(q, k, v, scale)
    b3 = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale, lse_in_chain=False)
    b4 = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale, lse_in_chain=True)
    assert torch.all(b4.e_dK >= b3.e_dK) and torch.all(b4.e_dV >= b3.e_dV)
    assert (b4.e_dV > b3.e_dV).float().mean() > 0.99
    assert torch.equal(b4.e_dQ, b3.e_dQ)


def test_forward_ragged_tail_tile_dropped_for_one_head_fails():
    """the forward skips the ragged last key tile (one key: Sk = 8192 + 1) for head 0 of four"""
    q, k, v, dO, scale = _case(64, Sq=128, Sk=8193, H=4)
    f = _fwd_ref(q, k, v, scale)
    O, _ = emu_fwd(q, k, v, scale, drop_tail_head=0)
    rep, rel = _verdict("forward ragged key tile dropped in head 0 (Sk 8193, H 4)", O, f.O, f.e_O, f.var_O, 8e-3)
    assert rel < 8e-3 and not rep.ok


def _emu_rope_epilogue(g, z, r, w, cos, sin):
    """rope_bwd_finish in fp32 on the stored bf16 gradient g: dy = R^T g, y = R^T z, out = bf16(r (w dy - y / w mean(dy y)))"""
    g, z, w = g.float(), z.float(), w.float()
    c, s = cos.float().repeat_interleave(2, -1), sin.float().repeat_interleave(2, -1)

    def rt(x):
        o = torch.empty_like(x)
        o[..., 0::2] = x[..., 0::2] * c[..., 0::2] + x[..., 1::2] * s[..., 0::2]
        o[..., 1::2] = x[..., 1::2] * c[..., 0::2] - x[..., 0::2] * s[..., 0::2]
        return o

    dy, y = rt(g), rt(z)
    m = (dy * y).sum(-1, keepdim=True) / 128
    return _bf(r[..., None].float() * (w * dy - y * (1.0 / w) * m))


@pytest.mark.parametrize("defect", [None, "norm weight set ignores the position split", "dK's rrms column read for dQ"])
def test_rope_epilogue_model(defect):
    """the fused RoPE + RMSNorm backward: the emulated epilogue on the kernel-like bf16 dQ passes the Jacobian-carried bound; a wrong weight set for the text
    positions, or the neighbouring head's 1 / rms, fails it"""
    q, k, v, dO, scale = _case(128, Sq=300, Sk=300)
    O, lse2 = emu_fwd(q, k, v, scale)
    dQ, _, _ = emu_bwd(q, k, v, dO, O, lse2, scale)
    b = AB.attn_bwd_model(q, k, v, dO, O, lse2, scale)
    g = torch.Generator().manual_seed(3)
    rr = torch.rand(1, 2, 300, generator=g) * 1.5 + 0.5
    w_lo, w_hi = [_bf(1.0 + 0.2 * torch.randn(128, generator=g)) for _ in range(2)]
    ang = torch.rand(300, 64, generator=g) * (2 * math.pi)
    cos, sin = torch.cos(ang), torch.sin(ang)
    wtok = torch.where(torch.arange(300)[:, None] < 77, w_lo[None], w_hi[None])[None, None].expand(1, 2, 300, 128)
    w_used, r_used = wtok, rr
    if defect == "norm weight set ignores the position split":
        w_used = w_hi[None, None, None].expand(1, 2, 300, 128)
    elif defect == "dK's rrms column read for dQ":
        r_used = rr.flip(1)
    out = _emu_rope_epilogue(dQ, q, r_used, w_used, cos, sin)
    tg, vg = AB.stored_tol_var(b.dQ, b.e_dQ, b.var_dQ)
    want, e, var = AB.rope_norm_bwd_model(b.dQ, tg, vg, q, rr, wtok, cos, sin)
    rep, rel = _verdict(f"rope epilogue, {defect or 'correct'}", out, want, e, var, 2e-2)
    if defect is None:
        AB.assert_bound(rep)
    else:
        assert not rep.ok

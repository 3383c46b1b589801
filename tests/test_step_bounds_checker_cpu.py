"""The loss / LoRA-gradient / optimizer bound checker (tests/step_bounds.py) bites: fp32 emulations of the kernels' summation trees and rounding points, written in
torch on the CPU, pass every check with err / e < 1 and the block statistic below 0.5, and each planted defect is reported by the check it was planted for.
The inputs are those of tests/test_step_bounds_gpu.py scaled down."""
import math

import numpy as np
import pytest
import torch

from tests import gemm_bounds as GB
from tests import step_bounds as SB

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(x):
    return x.float().to(BF16)


def _lane_tree(v):
    """wave_sum: xor-shuffle tree over the last axis (64 lanes), offsets 32 ... 1"""
    o = v.shape[-1] // 2
    while o >= 1:
        idx = torch.arange(v.shape[-1]) ^ o
        v = v + v[..., idx]
        o //= 2
    return v[..., 0]


def _passes(ok, what):
    assert ok, f"{what}: a correct emulation fails the check"


def _caught(ok, what):
    print(f"[defect] {what}: new checker {'pass' if ok else 'FAIL'}")
    assert not ok, f"{what}: the checker misses it"


# ---- skinny -------------------------------------------------------------------------------------------------------------------------------------------
def emu_skinny(Lbuf, n_off, P, Rbuf, c0, Rn, r_used, M, mc, alpha, prior, accumulate, seg=None, defect=None):
    """Lbuf [rows, ldl] / Rbuf [rows, ldr] physical bf16 buffers; logical row m lives at physical row (m // seg_rows) * seg_x + lo + m % seg_rows (seg = (seg_rows,
    seg_l, lo_l, seg_r, lo_r)) or at row m.  fp32 chunk partials, four interleaved lane sums, two shuffle adds, alpha, the prior.  Returns out [P, Rn_written]"""
    def rows(buf, seg_x, lo, m0, m1, ignore_stride=False):
        m = torch.arange(m0, m1)
        if seg is None:
            return buf[m]
        sr = seg[0]
        if ignore_stride:
            seg_x = sr
        return buf[(m // sr) * seg_x + lo + m % sr]

    nchunks = SB.cdiv(M, mc)
    pcols = slice(n_off, n_off + P)
    parts = []
    for c in range(nchunks):
        m0 = c * mc
        m1 = min(M, m0 + mc)
        if defect == "drop_ragged_chunk" and m1 - m0 < mc:
            parts.append(torch.zeros(P, Rn))
            continue
        hi = m1
        if defect == "read_past_M" and m1 - m0 < mc:
            hi = min(Lbuf.shape[0], m0 + SB.cdiv(m1 - m0, 64) * 64)        # the whole last 64-row sub-tile, rows >= M included
        sl, lol, sr_, lor = (seg[1], seg[2], seg[3], seg[4]) if seg is not None else (0, 0, 0, 0)
        l = rows(Lbuf, sl, lol, m0, hi)[:, pcols].float()
        r = rows(Rbuf, sr_, lor, m0, hi, ignore_stride=(defect == "r_seg_stride_ignored"))[:, c0:c0 + Rn].float()
        if defect == "p_edge_leak":                                     # the last 128-column tile read whole: neighbour columns of the last 8-column group leak
            l = l.clone()
            l[:, P - 8:] = rows(Lbuf, sl, lol, m0, hi)[:, n_off + P:n_off + P + 8].float()
        parts.append(l.t() @ r)
    lanes = []
    for q in range(4):
        s = torch.zeros(P, Rn)
        for c in range(q, nchunks, 4):
            if defect == "reduce_skips_q3" and c % 4 == 3:
                continue
            s = s + parts[c]
        lanes.append(s)
    s = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])
    a = torch.tensor(alpha, dtype=F32)
    width = Rn if defect == "writes_past_r_used" else r_used
    pr = prior[:, :width].float()
    if defect == "alpha_on_prior":
        out = a * (pr + s[:, :width])
    elif accumulate and defect != "accumulate_drops_prior":
        out = pr + a * s[:, :width]
    else:
        out = a * s[:, :width]
    full = prior.clone().float()
    full[:, :width] = out
    return full


def _skinny_case(seed, M, P, Rn, r_used, mc, seg=None):
    g = _gen(seed)
    if seg is None:
        rowsL = rowsR = M + 64
        segt = None
    else:
        sr, B = seg
        SL, SR, lol, lor = sr + 96, sr + 32, 64, 32
        rowsL, rowsR = B * SL, B * SR
        segt = (sr, SL, lol, SR, lor)
    n_off, c0 = 72, Rn
    Lbuf = _bf(torch.randn(rowsL, 2 * P + 16, generator=g))
    Rbuf = _bf(torch.randn(rowsR, 3 * Rn, generator=g) + 0.25)
    prior = torch.randn(P, Rn, generator=g)
    return dict(Lbuf=Lbuf, n_off=n_off, P=P, Rbuf=Rbuf, c0=c0, Rn=Rn, r_used=r_used, M=M, mc=mc, prior=prior, seg=segt)


def _skinny_check(cs, out, alpha, accumulate, name):
    """the GPU test's checks: the bound on the owned [P, r_used] block, and everything else of the output buffer untouched"""
    M, P, Rn, r_used, mc, seg = cs["M"], cs["P"], cs["Rn"], cs["r_used"], cs["mc"], cs["seg"]
    m = torch.arange(M)
    rl = m if seg is None else (m // seg[0]) * seg[1] + seg[2] + m % seg[0]
    rr = m if seg is None else (m // seg[0]) * seg[3] + seg[4] + m % seg[0]
    Lm = cs["Lbuf"][rl][:, cs["n_off"]:cs["n_off"] + P]
    R = cs["Rbuf"][rr][:, cs["c0"]:cs["c0"] + r_used]
    want, e = SB.skinny(Lm, R, alpha, mc, SB.cdiv(M, mc), prior=cs["prior"][:, :r_used] if accumulate else None)
    rep = SB.check_sum(name, out[:, :r_used], want, e)
    untouched = torch.equal(out[:, r_used:], cs["prior"][:, r_used:].float())
    return rep.ok and untouched, rep


@pytest.mark.parametrize("M,P,Rn,r_used,mc,seg,acc", [(300, 136, 32, 16, 256, None, False), (577, 320, 64, 48, 256, None, True),
                                                      (1040, 136, 64, 64, 512, None, True), (2080, 136, 32, 32, 1024, None, False),
                                                      (768, 136, 32, 16, 256, (256, 3), True), (1536, 64, 64, 48, 512, (512, 3), False)])
def test_skinny_correct_emulation_passes(M, P, Rn, r_used, mc, seg, acc):
    cs = _skinny_case(1, M, P, Rn, r_used, mc, seg)
    out = emu_skinny(alpha=0.37, accumulate=acc, **cs)
    ok, rep = _skinny_check(cs, out, 0.37, acc, f"skinny emu M={M} P={P} Rn={Rn} mc={mc} seg={seg}")
    _passes(ok, "skinny")
    assert rep.worst < 1.0 and rep.block_rms < 0.5


@pytest.mark.parametrize("defect,M,seg,acc", [("drop_ragged_chunk", 528, None, False), ("read_past_M", 528, None, False), ("p_edge_leak", 300, None, False),
                                              ("writes_past_r_used", 300, None, False), ("r_seg_stride_ignored", 768, (256, 3), False),
                                              ("reduce_skips_q3", 1000, None, False), ("accumulate_drops_prior", 300, None, True),
                                              ("alpha_on_prior", 300, None, True)])
def test_skinny_defect_is_caught(defect, M, seg, acc):
    cs = _skinny_case(2, M, 136, 32, 16, 256, seg)
    out = emu_skinny(alpha=0.37, accumulate=acc, defect=defect, **cs)
    ok, _ = _skinny_check(cs, out, 0.37, acc, f"skinny defect {defect}")
    _caught(ok, f"skinny: {defect}")


# ---- losses -------------------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(seed, B, n, period=None):
    g = _gen(seed)
    c = (0.01 + 0.99 * torch.rand(B, generator=g)).float()
    sc = torch.stack([torch.ones(B), c, 1e-3 * c], 1)[:, torch.arange(n) % 3]          # residuals at three scales: |d| ~ 1, ~ c, ~ 1e-3 c
    target = _bf(3.0 * sc * torch.randn(B, n, generator=g))                            # (the target at the residual's scale, or bf16 could not hold the small ones)
    pred = _bf(target.float() + sc * torch.randn(B, n, generator=g))
    w = (0.5 + torch.rand(B, generator=g)).float()
    em = None
    if period:
        em = torch.rand(B, period, generator=g).float()
        em[:, ::5] = 0.0
        em[:, 1::7] = 2.5
    return pred, target, c, w, em


def emu_loss(pred, target, loss_type, c, w, em, grad_scale, defect=None):
    B, n = pred.shape
    vecs = n // 8
    passes = SB.cdiv(vecs, 1024)
    ds = torch.tensor(SB.dscale32(grad_scale, n, B), dtype=F32)
    d = pred.float() - target.float()
    if em is None:
        m = torch.ones(B, n)
    else:
        period = em.shape[1]
        if defect == "mask_period_is_per_sample":              # sample b reads emask[b * period + i]: past its own row into the next samples' masks
            flat = em.reshape(-1)
            m = flat[(torch.arange(B)[:, None] * period + torch.arange(n)[None, :]) % flat.numel()]
        else:
            m = em[:, torch.arange(n) % period]
    wv = torch.ones(B) if w is None else w
    if loss_type == "l2":
        term = d * d * m
        dp = ds * wv[:, None] * d * m
        if defect == "weight_missing_from_dpred":
            dp = ds * d * m
    else:
        cc = (c[0:1].expand(B) if defect == "huber_c_of_sample_0" else c)[:, None]
        k = 2.0 * cc if loss_type == "huber" else torch.full_like(cc, 2.0)
        r = torch.sqrt(d * d + cc * cc)
        term = k * (r - cc) * m
        dp = 0.5 * ds * wv[:, None] * k * d / r * m
        if defect == "weight_missing_from_dpred":
            dp = 0.5 * ds * k * d / r * m
    t = torch.zeros(B, passes * 1024 * 8)
    t[:, :n] = term
    t = t.view(B, passes, 1024, 8)
    if defect == "last_partial_pass_dropped" and vecs % 1024:
        t[:, passes - 1] = 0
    acc = torch.zeros(B, 1024)
    for ps_ in range(passes):
        for j in range(8):
            acc = acc + t[:, ps_, :, j]
    wave = _lane_tree(acc.view(B, 16, 64))
    s = torch.zeros(B)
    for i in range(16):
        s = s + wave[:, i]
    per = (s * wv) * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(n), dtype=F32))
    lo = torch.zeros(())
    for b in range(B):
        lo = lo + per[b]
    lo = lo / torch.tensor(float(B))
    return lo.reshape(1), per, _bf(dp)


def _loss_check(pred, target, loss_type, c, w, em, grad_scale, outs, name):
    lo, per, dp = outs
    ref = SB.loss(pred, target, loss_type, huber_c=c, weight=w, emask=em, grad_scale=grad_scale)
    r1 = SB.check_sum(f"{name} per-sample", per.reshape(1, -1), ref["per_sample"][0].reshape(1, -1), ref["per_sample"][1].reshape(1, -1))
    r2 = SB.check_sum(f"{name} loss", lo.reshape(1, 1), ref["loss"][0].reshape(1, 1), ref["loss"][1].reshape(1, 1))
    r3 = SB.check_bf16(f"{name} dpred", dp, *ref["dpred"])
    return r1.ok and r2.ok and r3.ok, (r1, r2, r3)


@pytest.mark.parametrize("loss_type", ["l2", "huber", "smooth_l1"])
@pytest.mark.parametrize("B,n,period", [(1, 8, None), (3, 8 * 1024 - 8, None), (3, 8 * 1024 + 8, None), (5, 4 * 32 * 32, 32 * 32), (3, 8200, 8200)])
def test_loss_correct_emulation_passes(loss_type, B, n, period):
    pred, target, c, w, em = _loss_inputs(3, B, n, period)
    outs = emu_loss(pred, target, loss_type, c, w, em, 0.7)
    ok, reps = _loss_check(pred, target, loss_type, c, w, em, 0.7, outs, f"{loss_type} emu B={B} n={n}")
    _passes(ok, "loss")
    assert all(r.worst < 1.0 for r in reps) and reps[0].block_rms < 0.5 and reps[1].block_rms < 0.5


@pytest.mark.parametrize("defect,loss_type,n,period", [("mask_period_is_per_sample", "l2", 4 * 1024, 1024), ("weight_missing_from_dpred", "l2", 4096, None),
                                                      ("weight_missing_from_dpred", "huber", 4096, None), ("last_partial_pass_dropped", "l2", 8 * 1024 + 8, None),
                                                      ("last_partial_pass_dropped", "smooth_l1", 8 * 1024 + 8, None), ("huber_c_of_sample_0", "huber", 4096, None)])
def test_loss_defect_is_caught(defect, loss_type, n, period):
    pred, target, c, w, em = _loss_inputs(4, 3, n, period)
    outs = emu_loss(pred, target, loss_type, c, w, em, 0.7, defect=defect)
    ok, _ = _loss_check(pred, target, loss_type, c, w, em, 0.7, outs, f"{loss_type} defect {defect}")
    _caught(ok, f"loss: {defect} ({loss_type})")


# ---- grad_norm / clip -------------------------------------------------------------------------------------------------------------------------------------
def emu_grad_norm(g, skip_beyond_cap=False):
    n = g.numel()
    blocks = SB.grad_norm_blocks(n)
    stride = blocks * 256
    it = SB.cdiv(n, stride)
    f = torch.zeros(it * stride)
    f[:n] = g.float().reshape(-1)
    f = f.view(it, blocks, 256)
    if skip_beyond_cap:
        f = f[:1]
    acc = torch.zeros(blocks, 256)
    for i in range(f.shape[0]):
        acc = acc + f[i] * f[i]
    wave = _lane_tree(acc.view(blocks, 4, 64))
    part = torch.zeros(blocks)
    for i in range(4):
        part = part + wave[:, i]
    per = SB.cdiv(blocks, 64)
    pp = torch.zeros(per * 64)
    pp[:blocks] = part
    pp = pp.view(per, 64)
    lane = torch.zeros(64)
    for i in range(per):
        lane = lane + pp[i]
    return _lane_tree(lane.view(1, 64))[0], f.abs().max()


@pytest.mark.parametrize("n", [1, 255, 257, 70001, 300001])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_grad_norm_correct_emulation_passes(n, dtype):
    g = (torch.randn(n, generator=_gen(5)) * 0.02).to(dtype)
    ss, mx = emu_grad_norm(g)
    want, e, wmx = SB.grad_norm(g)
    rep = SB.check_sum(f"grad_norm emu n={n}", ss.reshape(1, 1), want, e)
    _passes(rep.ok, "grad_norm")
    assert rep.worst < 1.0 and rep.block_rms < 0.5
    assert float(mx) == float(wmx)


def test_grad_norm_defect_second_pass_skipped():
    n = 1024 * 256 + 4097                                      # the grid cap of k_grad_norm: the elements beyond blocks * 256 need a second pass
    g = torch.randn(n, generator=_gen(6)) * 0.02
    ss, _ = emu_grad_norm(g, skip_beyond_cap=True)
    want, e, _ = SB.grad_norm(g)
    _caught(SB.check_sum("grad_norm defect", ss.reshape(1, 1), want, e).ok, "grad_norm: elements beyond the grid's first pass skipped")


def emu_clip(g, ss, max_norm, pre_scale, ignore_pre_scale=False):
    norm = torch.sqrt(ss.float()) * (1.0 if ignore_pre_scale else np.float32(pre_scale))
    coef = torch.minimum(torch.tensor(np.float32(max_norm)) / (norm + np.float32(1e-6)), torch.tensor(1.0))
    if float(coef) >= 1.0:
        return g.clone()
    return (g.float() * coef).to(g.dtype)


def _clip_check(g, out, ss, max_norm, pre_scale, name):
    coef = SB.clip_coef(float(ss), max_norm, pre_scale)
    if coef >= 1.0:
        return torch.equal(SB.bits(out), SB.bits(g))
    want, e = SB.grad_clip(g, coef)
    rep = SB.check_f32(name, out, want, e) if g.dtype == F32 else SB.check_bf16(name, out, want, e, flat=True)
    return rep.ok


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_grad_clip_emulation_and_pre_scale_defect(dtype):
    g = (torch.randn(60001, generator=_gen(7)) * 0.02).to(dtype)
    ss, _ = emu_grad_norm(g)                                   # norm ~ 4.9
    for max_norm, pre in ((1.0, 0.5), (100.0, 0.5)):
        _passes(_clip_check(g, emu_clip(g, ss, max_norm, pre), ss, max_norm, pre, f"clip emu max_norm={max_norm}"), "grad_clip_norm")
    _caught(_clip_check(g, emu_clip(g, ss, 1.0, 0.5, ignore_pre_scale=True), ss, 1.0, 0.5, "clip defect"), "grad_clip_norm: pre_scale ignored")
    # a clip that scales although coef >= 1 is a bit difference
    _caught(_clip_check(g, (g.float() * (1 - 2.0 ** -6)).to(dtype), ss, 100.0, 0.5, "clip defect"), "grad_clip_norm: elements changed at coef >= 1")


# ---- AdamW / EMA ------------------------------------------------------------------------------------------------------------------------------------------
def _adam_state(seed, n, dtype=F32):
    g_ = _gen(seed)
    p = (torch.randn(n, generator=g_) * 0.05).to(dtype)
    g = (torch.randn(n, generator=g_) * 1e-3).to(dtype)
    m = torch.randn(n, generator=g_) * 1e-3
    v = (torch.randn(n, generator=g_) * 1e-3) ** 2
    m[::22] = 0
    v[::11] = 0
    g[::11] = 0                                                # v = 0 and g = 0: the denominator is eps; m = 0 on half of them, on the others the update is
                                                               # step_size m' / eps, so that a wrong denominator there moves p
    ema = (p.float() + 1e-3 * torch.randn(n, generator=g_)).to(dtype)
    return p, g, m, v, ema


def emu_adamw(p, g, m, v, ema, c, defect=None, step1_consts=None):
    f = lambda x: torch.tensor(x, dtype=F32)
    k = step1_consts if defect == "bias_correction_of_step_1" else c
    one = f(1.0)
    g1 = g.float() * f(c["gs"])
    p1 = p.float() * (one - f(c["lr"]) * f(c["wd"]))
    m1 = m + (g1 - m) * (one - f(c["b1"]))
    v1 = v * f(c["b2"]) + (one - f(c["b2"])) * g1 * g1
    denom = torch.sqrt(v1) / f(k["bc2_sqrt"]) + f(c["eps"])
    if defect == "eps_inside_bias_correction":                 # (sqrt(v') + eps) / bc2_sqrt: differs only where sqrt(v') is not far above eps
        denom = (torch.sqrt(v1) + f(c["eps"])) / f(k["bc2_sqrt"])
    p2 = p1 - f(k["step_size"]) * (m1 / denom)
    src = p.float() if defect == "ema_from_old_parameter" else p2.to(p.dtype).float()
    if p.dtype == F32:
        e2 = ema - f(c["omd"]) * (ema - src)
    else:
        diff = (ema.float() - src).to(BF16).float()
        e2 = (ema.float() - f(c["omd"]) * diff).to(BF16)
    outs = [p2.to(p.dtype), m1, v1, e2]
    n = p.numel()
    if defect == "tail_skipped":
        t = n - n % 4
        for o, old in zip(outs, (p, m, v, ema)):
            o[t:] = old[t:]
    if defect == "beyond_grid_skipped":
        t = 2048 * 256 * 4
        for o, old in zip(outs, (p, m, v, ema)):
            o[t:] = old[t:]
    return outs


def _adam_check(p, g, m, v, ema, c, outs, name):
    p2, m1, v1, e2 = outs
    ref = SB.adamw(p, g, m, v, c)
    ok = SB.check_f32(f"{name} m", m1, *ref["m"]).ok and SB.check_f32(f"{name} v", v1, *ref["v"]).ok
    if p.dtype == F32:
        ok = ok and SB.check_f32(f"{name} p", p2, *ref["p"]).ok and SB.check_f32(f"{name} ema", e2, *SB.ema_f32(ema, p2, c["omd"])).ok
    else:
        ok = ok and SB.check_bf16(f"{name} p", p2, *ref["p"], flat=True).ok and SB.check_bf16(f"{name} ema", e2, *SB.ema_bf16(ema, p2, c["omd"]), flat=True).ok
    return ok


@pytest.mark.parametrize("step,wd", [(1, 0.0), (1000, 1e-2)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_adamw_correct_emulation_passes(step, wd, dtype):
    st = _adam_state(8, 8 * 4099 if dtype == BF16 else 100003, dtype)
    c = SB.adam_consts(1e-3, 0.9, 0.999, 1e-8, wd, step, 0.5, 0.99)
    _passes(_adam_check(*st, c, emu_adamw(*st, c), f"adamw emu step {step} {dtype}"), "adamw")


@pytest.mark.parametrize("defect,n", [("tail_skipped", 100003), ("beyond_grid_skipped", 2048 * 256 * 4 + 7), ("bias_correction_of_step_1", 4099),
                                      ("ema_from_old_parameter", 4099), ("eps_inside_bias_correction", 4099)])
def test_adamw_defect_is_caught(defect, n):
    st = _adam_state(9, n)
    c = SB.adam_consts(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1000, 0.5, 0.99)
    c1 = SB.adam_consts(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0.5, 0.99)
    _caught(_adam_check(*st, c, emu_adamw(*st, c, defect=defect, step1_consts=c1), f"adamw defect {defect}"), f"adamw: {defect}")


def test_ema_update_emulations():
    g_ = _gen(10)
    omd = float(np.float32(1.0) - np.float32(0.999))
    s, p = torch.randn(60001, generator=g_), torch.randn(60001, generator=g_)
    o = s - torch.tensor(omd, dtype=F32) * (s - p)
    _passes(SB.check_f32("ema fp32 emu", o, *SB.ema_f32(s, p, omd)).ok, "ema_update fp32")
    sb, pb = s.to(BF16), p.to(BF16)
    ob = (sb.float() - torch.tensor(omd, dtype=F32) * (sb.float() - pb.float()).to(BF16).float()).to(BF16)
    _passes(SB.check_bf16("ema bf16 emu", ob, *SB.ema_bf16(sb, pb, omd), flat=True).ok, "ema_update bf16")
    _caught(SB.check_f32("ema fp32 defect", s - torch.tensor(omd, dtype=F32) * (s - 0.9 * p), *SB.ema_f32(s, p, omd)).ok, "ema_update: wrong parameter")

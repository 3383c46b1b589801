"""The norm / parameter-sum bound checker (tests/norm_bounds.py) bites: on CPU emulations of the kernels' rounding points (fp32 two-pass or pivoted statistics,
fp32 partial sums, one RNE per stored bf16 output), a correct computation passes every check, and each modelled kernel defect fails the new checker while the
suite's existing global rel-L2 check for that output (LN 4e-3 / 6e-3, layernorm_param_grads 3e-3, GroupNorm 5e-3 / 8e-3, q / k norm 4e-3 / 6e-3, wgrad 1.5e-2,
stats.hip fp32 sums 2e-5) still passes.  Each defect prints its old rel-L2 next to the new verdict."""
import math

import pytest
import torch

from tests import norm_bounds as NB

BF16 = torch.bfloat16
F64 = torch.float64


def _bf(x):
    return x.float().to(BF16).float()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(defect, old, bar, failed):
    print(f"[defect] {defect}: old rel-L2 = {old:.2e} (bar {bar:g}) -> new checker {'FAIL' if failed else 'pass'}")
    assert old < bar, f"{defect}: the old check would already catch it ({old:.2e} >= {bar:g})"
    assert failed, f"{defect}: the new checker misses it"


# ---- LayerNorm + modulation ---------------------------------------------------------------------------------------------------------------------------
def _ln_inputs(R, D, seed, rpb=None, offset=0.0):
    g = _gen(seed)
    x = _bf(torch.randn(R, D, generator=g) * 1.3 + offset + 0.3 * torch.randn(1, D, generator=g))
    nb = 1 if rpb is None else R // rpb
    sc = _bf(0.2 * torch.randn(nb, D, generator=g))
    sh = _bf(0.2 * torch.randn(nb, D, generator=g))
    return x, sc, sh


def emu_ln_stats(x, eps, wrong_rstd_row=None, tail_rows=None, D_seen=None):
    """fp32 two-pass statistics; defects: rstd x (1 + 2^-7) on one row; the mean of rows tail_rows taken over the first D_seen columns (a dropped masked tail)"""
    D = x.shape[1]
    xf = x.float()
    s = xf.sum(1)
    if tail_rows is not None:
        s[tail_rows] = xf[tail_rows, :D_seen].sum(1)
    mean = s / D
    d = xf - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(1) / D + eps)
    if wrong_rstd_row is not None:
        rstd[wrong_rstd_row] *= 1 + 2.0 ** -7
    return mean, rstd


def emu_ln_fwd(x, sc, sh, rpb, eps, **defect):
    mean, rstd = emu_ln_stats(x, eps, **defect)
    b = torch.arange(x.shape[0]) // rpb
    y = (x.float() - mean[:, None]) * rstd[:, None] * (1 + sc[b]) + sh[b]
    return _bf(y)


def _ln_fwd_check(x, sc, sh, rpb, eps, out, name):
    D = x.shape[1]
    st = NB.ln_stats(x.double(), eps, NB.L_ln(NB.cdiv(D, 512)))
    b = torch.arange(x.shape[0]) // rpb
    a, bb = 1 + sc.double()[b], sh.double()[b]
    want, e, dmu, dlr = NB.norm_fwd(x.double(), st, a, bb)
    rep = NB.check(name, out, want, e)
    fit = NB.fit_rows(name, out, want, e, dmu, dlr, st.e_mu, st.e_r)
    return rep.ok and fit.ok, NB.rel_l2(out, want)


def test_ln_fwd_correct_passes():
    for D, off in ((256, 0.0), (520, 0.0), (1160, 3.0), (3072, 0.0), (4096, 16.0)):
        x, sc, sh = _ln_inputs(70, D, 1, rpb=35, offset=off)
        ok, _ = _ln_fwd_check(x, sc, sh, 35, 1e-6, emu_ln_fwd(x, sc, sh, 35, 1e-6), f"ln fwd D={D} offset {off}")
        assert ok


def test_defect_ln_rstd_one_row():
    x, sc, sh = _ln_inputs(64, 1536, 2, rpb=32)
    ok, old = _ln_fwd_check(x, sc, sh, 32, 1e-6, emu_ln_fwd(x, sc, sh, 32, 1e-6, wrong_rstd_row=17), "ln fwd, rstd x (1+2^-7) on row 17")
    _report("LN rstd x (1+2^-7) on one row", old, 4e-3, not ok)


def test_defect_ln_dropped_masked_tail():
    x, sc, sh = _ln_inputs(64, 520, 3, rpb=64)
    ok, old = _ln_fwd_check(x, sc, sh, 64, 1e-6, emu_ln_fwd(x, sc, sh, 64, 1e-6, tail_rows=slice(8, 12), D_seen=512), "ln fwd D=520, mean of rows 8-11 over 512")
    _report("LN mean of one 4-row workgroup over D rounded down to 512 (D = 520)", old, 4e-3, not ok)


def emu_ln_bwd(dy, x, sc, rpb, eps, dres=None, dres_twice_row=None):
    mean, rstd = emu_ln_stats(x, eps)
    b = torch.arange(x.shape[0]) // rpb
    g = dy.float() * (1 + sc[b])
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    o = rstd[:, None] * (g - c1 - xh * c2)
    if dres is not None:
        o = o + dres
        if dres_twice_row is not None:
            o[dres_twice_row] += dres[dres_twice_row]
    return _bf(o)


def _ln_bwd_check(dy, x, sc, rpb, eps, dres, out, name):
    D = x.shape[1]
    L = NB.L_ln(NB.cdiv(D, 512))
    st = NB.ln_stats(x.double(), eps, L)
    b = torch.arange(x.shape[0]) // rpb
    want, e = NB.ln_bwd(dy.double(), x.double(), 1 + sc.double()[b], st, L, dres=dres.double())
    return NB.check(name, out, want, e).ok, NB.rel_l2(out, want)


def test_ln_bwd_correct_and_dres_twice():
    x, sc, _ = _ln_inputs(64, 2432, 4, rpb=32)
    g = _gen(5)
    dy, dres = _bf(torch.randn(64, 2432, generator=g)), _bf(0.03 * torch.randn(64, 2432, generator=g))
    ok, _ = _ln_bwd_check(dy, x, sc, 32, 1e-6, dres, emu_ln_bwd(dy, x, sc, 32, 1e-6, dres), "ln bwd D=2432")
    assert ok
    ok, old = _ln_bwd_check(dy, x, sc, 32, 1e-6, dres, emu_ln_bwd(dy, x, sc, 32, 1e-6, dres, dres_twice_row=40), "ln bwd, dres added twice on row 40")
    _report("LN bwd dres added twice on one row", old, 6e-3, not ok)


# ---- layernorm_param_grads ----------------------------------------------------------------------------------------------------------------------------
def test_ln_param_grads_last_wave_dropped():
    R, D = 16384, 256
    g = _gen(6)
    x = _bf(torch.randn(R, D, generator=g) + 2 * torch.randn(1, D, generator=g))
    dy = _bf(torch.randn(R, D, generator=g) * 0.5 + 1.0)
    mean, rstd = emu_ln_stats(x, 1e-5)
    t = dy.float() * (x.float() - mean[:, None]) * rstd[:, None]
    L = NB.L_ln_params(R)
    st = NB.ln_stats(x.double(), 1e-5, NB.L_ln(1))
    xh = (x.double() - st.mu[:, None]) * st.r[:, None]
    e_xh = st.r[:, None] * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * NB.U)
    want, e = NB.colsum(dy.double() * xh, L, dy.double().abs() * e_xh + NB.U * (dy.double() * xh).abs())
    good = t.view(32, 512, D).sum(1).sum(0)             # wave w owns rows w, w + 512, ...: 512 partials, summed in fp32
    assert NB.check_f32("lnp dweight", good, want, e).ok
    bad = t.view(32, 512, D)[:, :511].sum(1).sum(0)
    rep = NB.check_f32("lnp dweight, last wave's partial dropped", bad, want, e)
    _report("layernorm_param_grads dropping the last wave's partial", NB.rel_l2(bad, want), 3e-3, not rep.ok)


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------------------
def _gn_chunks(B, H, W):
    rows_img = (H + 2) * (W + 2)
    nch = max(1, min((768 + B - 1) // B, (rows_img + 31) // 32))
    rpc = (rows_img + nch - 1) // nch
    return (rows_img + rpc - 1) // rpc, rpc


def emu_gn_stats(xg, B, H, W, G, eps, one_pass=False, drop_last_chunk_img=None):
    """k_gn_stats<0> + k_gn_finalize_fwd on a zero-bordered grid xg [B, (H+2)(W+2), C] in fp32 chunk partials.  Correct form: sums shifted by a pivot per
    (image, chunk, channel) from the chunk's first interior row, merged exactly about one reference pivot of the group.  one_pass: sum x, sum x^2, var = E x^2 - mean^2."""
    C = xg.shape[-1]
    cg = C // G
    rows_img = (H + 2) * (W + 2)
    nch, rpc = _gn_chunks(B, H, W)
    pos = torch.arange(rows_img)
    yy, xx = pos // (W + 2), pos % (W + 2)
    inside = (yy >= 1) & (yy <= H) & (xx >= 1) & (xx <= W)
    mean = torch.zeros(B, G)
    rstd = torch.zeros(B, G)
    n = H * W * cg
    for b in range(B):
        parts = []
        for k in range(nch):
            if drop_last_chunk_img == b and k == nch - 1:
                continue
            sl = slice(k * rpc, min(rows_img, (k + 1) * rpc))
            v, m = xg[b, sl].float(), inside[sl]
            cnt = int(m.sum())
            if one_pass:
                parts.append((cnt, torch.zeros(C), v.sum(0), (v * v).sum(0)))
            else:
                p = v[m][0] if cnt else torch.zeros(C)
                dv = (v - p) * m[:, None]
                parts.append((cnt, p, dv.sum(0), (dv * dv).sum(0)))
        for gi in range(G):
            cs = slice(gi * cg, (gi + 1) * cg)
            if one_pass:
                s0 = sum(pt[2][cs].sum() for pt in parts)
                s1 = sum(pt[3][cs].sum() for pt in parts)
                mu = s0 / n
                var = torch.clamp(s1 / n - mu * mu, min=0)
            else:               # one pass about the reference pivot p0 (the group's first channel in the chunk holding the first interior row)
                p0 = parts[(W + 3) // rpc][1][cs][0]
                a1 = sum((pt[0] * (pt[1][cs] - p0) + pt[2][cs]).sum() for pt in parts)
                a2 = sum((pt[3][cs] + 2 * (pt[1][cs] - p0) * pt[2][cs] + pt[0] * (pt[1][cs] - p0) ** 2).sum() for pt in parts)
                d = a1 / n
                mu = p0 + d
                var = torch.clamp(a2 / n - d * d, min=0)
            mean[b, gi], rstd[b, gi] = mu, torch.rsqrt(var + eps)
    return mean, rstd


def _gn_problem(B, H, W, C, seed, offsets=(0.0,)):
    g = _gen(seed)
    x = torch.randn(B, H, W, C, generator=g)
    G = 32
    cg = C // G
    for gi in range(G):
        x[..., gi * cg:(gi + 1) * cg] += offsets[gi % len(offsets)]
    x = _bf(x)
    xg = torch.zeros(B, H + 2, W + 2, C)
    xg[:, 1:H + 1, 1:W + 1] = x
    gamma = _bf(1 + 0.2 * torch.randn(C, generator=g))
    beta = _bf(0.3 * torch.randn(C, generator=g))
    return x, xg.view(B, -1, C), gamma, beta


def _gn_fwd_check(x, gamma, beta, B, H, W, eps, mean, rstd, name, silu=False):
    C = x.shape[-1]
    G, cg = 32, C // 32
    nch, rpc = _gn_chunks(B, H, W)
    L = NB.L_gn(rpc, NB.gn_stats_RT(C), nch, cg)
    xs = x.double().view(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
    st = NB.ln_stats(xs, eps, L, pivoted=True)
    gam = gamma.double().view(1, 1, G, cg).expand(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
    bet = beta.double().view(1, 1, G, cg).expand(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
    want, e, dmu, dlr = NB.norm_fwd(xs, st, gam, bet, silu=silu)
    mu = mean.view(B * G, 1)
    rs = rstd.view(B * G, 1)
    z = (xs.float() - mu) * rs * gam.float() + bet.float()
    out = _bf(z * torch.sigmoid(z) if silu else z)
    rep = NB.check(name, out, want, e)
    fit = NB.fit_rows(name, out, want, e, dmu, dlr, st.e_mu, st.e_r)
    return rep.ok and fit.ok, NB.rel_l2(out, want)


def test_gn_correct_passes_every_offset():
    for off in (0.0, 16.0, 64.0, 256.0):
        B, H, W, C = 1, 32, 32, 512
        x, xg, gamma, beta = _gn_problem(B, H, W, C, 7, offsets=(off, 0.0))
        mean, rstd = emu_gn_stats(xg, B, H, W, 32, 1e-6)
        ok, _ = _gn_fwd_check(x, gamma, beta, B, H, W, 1e-6, mean, rstd, f"gn fwd offset {off}", silu=True)
        assert ok


def test_defect_gn_one_pass_variance_offset256():
    B, H, W, C = 2, 32, 32, 512
    offs = tuple([256.0] + [0.0] * 31)
    x, xg, gamma, beta = _gn_problem(B, H, W, C, 8, offsets=offs)
    mean, rstd = emu_gn_stats(xg, B, H, W, 32, 1e-6, one_pass=True)
    ok, old = _gn_fwd_check(x, gamma, beta, B, H, W, 1e-6, mean, rstd, "gn fwd one-pass variance, offset 256 on group 0")
    _report("GroupNorm one-pass variance on an offset-256 group", old, 5e-3, not ok)


def test_defect_gn_last_ragged_chunk_dropped():
    B, H, W, C = 2, 1000, 2, 64
    x, xg, gamma, beta = _gn_problem(B, H, W, C, 9, offsets=(0.5,))
    nch, rpc = _gn_chunks(B, H, W)
    assert (H + 2) * (W + 2) % rpc != 0
    mean, rstd = emu_gn_stats(xg, B, H, W, 32, 1e-6, drop_last_chunk_img=1)
    ok, old = _gn_fwd_check(x, gamma, beta, B, H, W, 1e-6, mean, rstd, "gn fwd, last ragged chunk of image 1 dropped")
    _report("GroupNorm dropping the last ragged chunk of one image", old, 5e-3, not ok)


def test_defect_gn_param_grads_swapped_window():
    """k_gn_stats<1> leaves per (image, chunk, channel) A = sum g, B = sum g x_hat; k_gn_param_grads sums them into dbeta / dgamma.  The defect: A and B
    swapped for the second channel window (channels 2048..2559) of one chunk.  On a gradient whose g follows 0.5 + 0.5 x_hat the two sums are close."""
    B, H, W, C = 2, 24, 24, 2560
    g = _gen(10)
    xh = torch.randn(B, (H + 2) * (W + 2), C, generator=g).double()
    nch, rpc = _gn_chunks(B, H, W)
    pos = torch.arange((H + 2) * (W + 2))
    yy, xx = pos // (W + 2), pos % (W + 2)
    inside = ((yy >= 1) & (yy <= H) & (xx >= 1) & (xx <= W)).double()[None, :, None]
    xh = xh * inside
    gg = _bf((0.5 + 0.5 * xh + 0.1 * torch.randn(xh.shape, generator=g).double()) * inside).double()
    L = NB.L_gn_params(rpc, NB.gn_stats_RT(C), nch, B)
    dg_w, dg_e = NB.colsum((gg * xh).view(-1, C), L, NB.U * (gg * xh).abs().view(-1, C))
    db_w, db_e = NB.colsum(gg.view(-1, C), L)
    pad = nch * rpc - (H + 2) * (W + 2)
    A = torch.nn.functional.pad(gg.float(), (0, 0, 0, pad)).view(B, nch, rpc, C).sum(2)
    Bp = torch.nn.functional.pad((gg * xh).float(), (0, 0, 0, pad)).view(B, nch, rpc, C).sum(2)
    assert NB.check_f32("gn dgamma", Bp.sum((0, 1)), dg_w, dg_e).ok and NB.check_f32("gn dbeta", A.sum((0, 1)), db_w, db_e).ok
    A2, B2 = A.clone(), Bp.clone()
    A2[1, nch // 2, 2048:], B2[1, nch // 2, 2048:] = Bp[1, nch // 2, 2048:], A[1, nch // 2, 2048:]
    dg, db = B2.sum((0, 1)), A2.sum((0, 1))
    r1, r2 = NB.check_f32("gn dgamma, one chunk's window swapped", dg, dg_w, dg_e), NB.check_f32("gn dbeta, one chunk's window swapped", db, db_w, db_e)
    old = max(NB.rel_l2(dg, dg_w), NB.rel_l2(db, db_w))
    _report("GroupNorm dgamma / dbeta partials swapped on one channel window of one chunk", old, 5e-3, not (r1.ok and r2.ok))


# ---- q / k RMSNorm + RoPE -----------------------------------------------------------------------------------------------------------------------------
def _tables(S, hd, base=10000.0):
    """1-D RoPE tables, one angle pos * base^(-2i / hd) per interleaved pair, duplicated per channel (the layout of st355_qk_norm_rope_fwd)"""
    freq = base ** (-torch.arange(0, hd, 2, dtype=F64) / hd)
    ang = torch.arange(S, dtype=F64)[:, None] * freq[None, :]
    return ang.cos().repeat_interleave(2, 1).float(), ang.sin().repeat_interleave(2, 1).float()


def emu_qk_fwd(x, w, cs, sn, eps, wrong_angle_head=None):
    r = torch.rsqrt((x.float() ** 2).mean(-1, keepdim=True) + eps)
    y = x.float() * r * w.float()
    c, s = cs.clone().expand(x.shape[0], *cs.shape).clone(), sn.expand(x.shape[0], *sn.shape).clone()
    if wrong_angle_head is not None:          # the last 8-channel chunk of that head reads the angles of the pair to its left
        hd = x.shape[-1]
        c[wrong_angle_head, :, hd - 8:] = cs[:, hd - 10:hd - 2]
        s[wrong_angle_head, :, hd - 8:] = sn[:, hd - 10:hd - 2]
    y0, y1 = y[..., 0::2], y[..., 1::2]
    o = torch.stack([y0 * c[..., 0::2] - y1 * s[..., 0::2], y1 * c[..., 1::2] + y0 * s[..., 1::2]], -1).flatten(-2)
    return _bf(o)


def test_qk_fwd_correct_and_wrong_angle():
    H, S, hd = 24, 256, 128
    g = _gen(11)
    x = _bf(torch.randn(H, S, hd, generator=g) * 2)
    w = _bf(1 + 0.2 * torch.randn(hd, generator=g))
    cs, sn = _tables(S, hd)
    want, e, dlr = NB.qk_fwd(x.double(), w.double(), cs.double(), sn.double(), 1e-6)
    ok = lambda out, nm: (NB.check(nm, out, want, e).ok and NB.fit_rows(nm, out.view(-1, hd), want.view(-1, hd), e.view(-1, hd), torch.ones_like(e.view(-1, hd)),
                                                                       dlr.view(-1, hd), torch.zeros(H * S, dtype=F64), torch.zeros(H * S, dtype=F64)).ok)
    assert ok(emu_qk_fwd(x, w, cs, sn, 1e-6), "qk fwd")
    bad = emu_qk_fwd(x, w, cs, sn, 1e-6, wrong_angle_head=5)
    _report("RoPE using the neighbouring pair's angle on one head (its last 8 channels)", NB.rel_l2(bad, want), 4e-3,
            not ok(bad, "qk fwd, neighbouring pair's angle on head 5"))


def test_qk_wgrad_last_slice_dropped():
    B, H, hd, S = 1, 32, 64, 65 * 64 - 10              # nblk = 2080 workgroups: 64 slices of per = 33, the last slice holds one workgroup
    g = _gen(13)
    x = _bf(torch.randn(B * H, S, hd, generator=g) + 1.0)
    w = _bf(1 + 0.2 * torch.randn(hd, generator=g))
    dq = _bf(torch.randn(B * H, S, hd, generator=g) + 0.5)
    cs, sn = _tables(S, hd)
    cs, sn = torch.ones_like(cs), torch.zeros_like(sn)  # identity rotation (SD3): keeps the per-channel mean of dy x r that a real gradient has
    _, _, dy, e_dy, r, e_r = NB.qk_bwd(dq.double(), x.double(), w.double(), cs.double(), sn.double(), 1e-6)
    t = dy * x.double() * r
    gx = (S + 63) // 64
    nblk = gx * B * H
    ns, per = 64, (nblk + 63) // 64
    assert nblk >= 2048 and nblk % per != 0
    L = NB.L_qk_wgrad(hd, ns, per)
    want, e = NB.colsum(t.view(-1, hd), L, (x.double().abs() * r * e_dy + t.abs() * (e_r + 2 * NB.U)).view(-1, hd))
    blocks = torch.zeros(B * H, gx * 64, hd)
    blocks[:, :S] = t.float()
    part = blocks.view(nblk, 64, hd).sum(1)            # workgroup blk = (b H + h) gx + bx
    slices = torch.stack([part[i * per:(i + 1) * per].sum(0) for i in range(ns)])
    assert NB.check("qk wgrad", _bf(slices.sum(0)).view(1, hd), want.view(1, hd), e.view(1, hd)).ok
    bad = _bf(slices[:ns - 1].sum(0))
    rep = NB.check("qk wgrad, last slice dropped", bad.view(1, hd), want.view(1, hd), e.view(1, hd))
    _report("QK wgrad losing the last slice when nblk is not a multiple of per", NB.rel_l2(bad, want), 1.5e-2, not rep.ok)


# ---- stats.hip ----------------------------------------------------------------------------------------------------------------------------------------
def test_stats_ragged_final_chunk_dropped():
    nb, rpb, D = 64, 8193, 16
    g = _gen(15)
    dy = _bf(torch.randn(nb, rpb, D, generator=g) + 1.0)
    chunks = NB.cdiv(rpb, 64)
    want, e = NB.colsum(dy.double(), NB.L_stats(chunks))
    good = dy.float().sum(1)
    assert NB.check_f32("d_shift", good, want, e).ok
    bad = good.clone()
    bad[3] = dy[3, :64 * (chunks - 1)].float().sum(0)            # rows_per_batch = 128 x 64 + 1: the last chunk holds one row
    rep = NB.check_f32("d_shift, ragged final chunk of batch 3 dropped", bad, want, e)
    _report("ln_modulate_bwd_stats dropping the ragged final 64-row chunk of a batch", NB.rel_l2(bad, want), 2e-5, not rep.ok)


def test_colsum_rows_ignoring_batch_stride():
    nb, rpb, stride, N = 2, 65536, 65537, 64
    g = _gen(16)
    a = _bf(torch.randn(nb * stride, N, generator=g) + 1.0)
    rows = torch.stack([a[b * stride:b * stride + rpb] for b in range(nb)])
    want, e = NB.colsum(rows.double(), NB.L_stats(NB.cdiv(rpb, 64)))
    assert NB.check_f32("colsum_rows", rows.float().sum(1), want, e).ok
    bad = torch.stack([a[b * rpb:(b + 1) * rpb] for b in range(nb)]).float().sum(1)
    rep = NB.check_f32("colsum_rows, batch_stride_rows ignored", bad, want, e)
    _report("colsum_rows ignoring batch_stride_rows", NB.rel_l2(bad, want), 2e-5, not rep.ok)

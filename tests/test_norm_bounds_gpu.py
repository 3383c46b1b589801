"""Every normalisation and parameter-sum route, element-wise against an fp64 reference (tests/norm_bounds.py), at the model widths and the edges where these
kernels go wrong.

Each case asserts the instance it runs on (ops.norm_plan -> st355_norm_plan: the helpers the launchers call), bounds every output element, fits each
normalised row / GroupNorm (image, group) for a coherent mean or rstd error, and runs twice: the reductions are fixed-order, so the two runs must be
bit-identical.  GroupNorm runs in both apply forms (ops.gn_set_apply).  The last test asserts that the cases reached every instance of the enumeration below:
run the module as a whole."""
import math

import pytest
import torch

from tests import norm_bounds as NB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
HIT = set()
WORST = {}
ALL_ROUTES = ({f"ln_fwd<{nc}>" for nc in (1, 2, 3, 4, 6, 8)} | {f"ln_bwd<{nc}>" for nc in (1, 2, 3, 4, 6, 8)} | {f"lnp<{nc}>" for nc in (1, 2, 3, 4)}
              | {f"ln_stats<{nc},{gs}>" for nc in (1, 2, 3, 4, 6) for gs in (0, 1)} | {f"gn{form}_win{w}" for form in (1, 2) for w in (1, 2)}
              | {"qk_fwd<64>", "qk_fwd<128>", "qk_bwd<64>", "qk_bwd<128>", "qk_wgrad<64,few>", "qk_wgrad<128,few>", "qk_wgrad<128,64>", "qk_rope_norm_bwd<128>",
                 "scale_cols_stats", "colsum_rows", "colsum_prod<0>", "colsum_prod<1>"})


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device=dev(), generator=g) * scale + shift).to(BF16)


def _note(family, rep):
    """keep the worst element ratio and row statistic per family for the report"""
    w = WORST.setdefault(family, {"err/tol": 0.0, "offset SE": 0.0, "slope SE": 0.0, "block": 0.0})
    if isinstance(rep, NB.FitReport):
        w["offset SE"] = max(w["offset SE"], rep.offset)
        w["slope SE"] = max(w["slope SE"], rep.slope)
        assert rep.ok, rep.line()
    elif isinstance(rep, NB.SumReport):
        w["err/tol"] = max(w["err/tol"], rep.worst)
        w["block"] = max(w["block"], rep.block_rms)
        assert rep.ok, rep.line()
    else:
        w["err/tol"] = max(w["err/tol"], rep.worst)
        w["block"] = max(w["block"], rep.block_rms)
        NB.GB.assert_bound(rep)


def _same(a, b, what):
    for x, y in zip(a, b):
        if x is None:
            continue
        bx = x.view(torch.int16) if x.dtype == BF16 else x.view(torch.int32)
        by = y.view(torch.int16) if y.dtype == BF16 else y.view(torch.int32)
        assert torch.equal(bx, by), f"{what}: two runs differ (the reduction order must be fixed)"


def _clone(ts):
    return [None if t is None else t.clone() for t in ts]


# ------------------------------------------------------------------------------------------------
# LayerNorm + modulation, affine LayerNorm, layer_norm_xhat
# ------------------------------------------------------------------------------------------------
LN_D = [256, 512, 520, 1024, 1152, 1160, 1536, 2048, 2432, 2440, 3072, 4096]


@pytest.mark.parametrize("D", LN_D)
def test_ln_modulate(ops, D):
    g = _gen(100 + D)
    B, rpb = 2, 35                         # rows 70: not a multiple of 4; rows_per_batch 35
    rows = B * rpb
    nc = ops.norm_plan("ln", D)["nc"]
    xbuf = _randn(g, rows, D + 24, scale=1.3, shift=0.4)
    xbuf[:, :D] += (0.5 * torch.randn(1, D, device=dev(), generator=g)).to(BF16)
    x = xbuf[:, :D]                        # ldx = D + 24
    mod = _randn(g, B, 6 * D, scale=0.3)   # the [B, 6D] modulation table: shift | scale | gate | ...
    shift, scale, gate = mod[:, 0:D], mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    ybuf = torch.empty(rows, D + 40, device=dev(), dtype=BF16)
    y = ybuf[:, :D]
    ops.ln_modulate_fwd(x, scale, shift, rpb, eps=1e-6, out=y)
    y0 = y.clone()
    ops.ln_modulate_fwd(x, scale, shift, rpb, eps=1e-6, out=y)
    _same([y], [y0], f"ln fwd D={D}")
    HIT.add(f"ln_fwd<{nc}>")
    L = NB.L_ln(nc)
    xd = x.double()
    st = NB.ln_stats(xd, 1e-6, L)
    b = torch.arange(rows, device=dev()) // rpb
    a, bb = 1 + scale.double()[b], shift.double()[b]
    want, e, dmu, dlr = NB.norm_fwd(xd, st, a, bb)
    _note("ln", NB.check(f"ln_modulate_fwd D={D} (NC {nc})", y, want, e))
    _note("ln", NB.fit_rows(f"ln_modulate_fwd D={D}", y, want, e, dmu, dlr, st.e_mu, st.e_r))
    # layer_norm_xhat: scale = shift = 0
    xh = ops.layer_norm_xhat(x, eps=1e-6)
    w2, e2, _, _ = NB.norm_fwd(xd, st, torch.ones_like(xd), torch.zeros_like(xd))
    _note("ln", NB.check(f"layer_norm_xhat D={D}", xh, w2, e2))
    # (no row fit here: the statistics are the ones fitted above, same kernel and rows; without a per-column scale the outputs of neighbouring bf16 inputs
    # land on a regular lattice and their roundings are not independent)

    # backward: dres / gate on and off, strided dy and dres
    dybuf = _randn(g, rows, D + 8)
    dy = dybuf[:, :D]
    dresbuf = _randn(g, rows, D + 16, scale=0.05)
    dres = dresbuf[:, 8:D + 8]
    for use_dres, gated in ((False, False), (True, True), (True, False)):
        outs = ops.ln_modulate_bwd(dy, x, scale, rpb, dres=dres if use_dres else None, gate=gate, eps=1e-6, want_gated=gated)
        outs2 = ops.ln_modulate_bwd(dy, x, scale, rpb, dres=dres if use_dres else None, gate=gate, eps=1e-6, want_gated=gated)
        _same(outs, outs2, f"ln bwd D={D}")
        HIT.add(f"ln_bwd<{nc}>")
        dx, dxg = outs
        want, e = NB.ln_bwd(dy.double(), xd, a, st, L, dres=dres.double() if use_dres else None)
        _note("ln bwd", NB.check(f"ln_modulate_bwd D={D} dres={use_dres}", dx, want, e))
        if gated:
            w3, e3 = NB.mul_stored(dx.double(), gate.double()[b])
            _note("ln bwd", NB.check(f"ln_modulate_bwd D={D} dxg (from dx as stored)", dxg, w3, e3))


@pytest.mark.parametrize("D", [320, 640, 1280, 2048])
def test_layernorm_affine(ops, D):
    g = _gen(200 + D)
    rows = 77
    nc = ops.norm_plan("ln", D)["nc"]
    x = _randn(g, rows, D, scale=2.0, shift=-0.7)
    w, bias = _randn(g, D, scale=0.3, shift=1.0), _randn(g, D, scale=0.2)
    y = ops.layernorm_fwd(x, w, bias, eps=1e-5)
    _same([y], [ops.layernorm_fwd(x, w, bias, eps=1e-5)], "layernorm_fwd")
    HIT.add(f"ln_fwd<{nc}>")
    L = NB.L_ln(nc)
    st = NB.ln_stats(x.double(), 1e-5, L)
    a, bb = w.double()[None].expand(rows, D), bias.double()[None].expand(rows, D)
    want, e, dmu, dlr = NB.norm_fwd(x.double(), st, a, bb)
    _note("ln", NB.check(f"layernorm_fwd D={D}", y, want, e))
    _note("ln", NB.fit_rows(f"layernorm_fwd D={D}", y, want, e, dmu, dlr, st.e_mu, st.e_r))
    dy, dres = _randn(g, rows, D), _randn(g, rows, D, scale=0.1)
    dx = ops.layernorm_bwd(dy, x, w, dres=dres, eps=1e-5)
    _same([dx], [ops.layernorm_bwd(dy, x, w, dres=dres, eps=1e-5)], "layernorm_bwd")
    HIT.add(f"ln_bwd<{nc}>")
    want, e = NB.ln_bwd(dy.double(), x.double(), a, st, L, dres=dres.double())
    _note("ln bwd", NB.check(f"layernorm_bwd D={D}", dx, want, e))


# ------------------------------------------------------------------------------------------------
# parameter sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rows,accumulate", [(320, 8192, False), (640, 8200, True), (1280, 16384, False), (2048, 9000, True)])
def test_layernorm_param_grads(ops, D, rows, accumulate):
    g = _gen(300 + D)
    nc = ops.norm_plan("ln_params", D)["nc"]
    x = _randn(g, rows, D, scale=1.5, shift=0.3)
    dy = _randn(g, rows, D, scale=0.5, shift=0.2)
    c0w, c0b = torch.randn(D, device=dev(), generator=g), torch.randn(D, device=dev(), generator=g)
    dw, db = c0w.clone(), c0b.clone()
    ops.layernorm_param_grads(dy, x, dw, db, eps=1e-5, accumulate=accumulate)
    dw2, db2 = c0w.clone(), c0b.clone()
    ops.layernorm_param_grads(dy, x, dw2, db2, eps=1e-5, accumulate=accumulate)
    _same([dw, db], [dw2, db2], "layernorm_param_grads")
    HIT.add(f"lnp<{nc}>")
    st = NB.ln_stats(x.double(), 1e-5, NB.L_ln(nc))
    xh = (x.double() - st.mu[:, None]) * st.r[:, None]
    e_xh = st.r[:, None] * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * NB.U)
    Lp = NB.L_ln_params(rows) + (1 if accumulate else 0)
    t = dy.double() * xh
    ww, ew = NB.colsum(t, Lp, dy.double().abs() * e_xh + NB.U * t.abs())
    wb, eb = NB.colsum(dy.double(), Lp)
    if accumulate:
        ww, wb = ww + c0w.double(), wb + c0b.double()
    _note("param sums", NB.check_f32(f"layernorm_param_grads D={D} rows={rows} dweight", dw, ww, ew))
    _note("param sums", NB.check_f32(f"layernorm_param_grads D={D} rows={rows} dbias", db, wb, eb))


@pytest.mark.parametrize("D,rpb,nb,gs,bias_bf16", [(256, 200, 2, False, False), (512, 4097, 2, True, False), (1024, 64, 2, False, False),
                                                   (1024, 130, 3, True, False), (1152, 100, 2, False, False), (1536, 64, 2, True, True),
                                                   (2048, 333, 2, False, False), (2048, 130, 2, True, False), (2432, 70, 2, False, False),
                                                   (3072, 70, 2, True, True)])
def test_ln_modulate_bwd_stats(ops, D, rpb, nb, gs, bias_bf16):
    g = _gen(400 + D)
    rows = nb * rpb
    plan = ops.norm_plan("ln_stats", D, rpb, int(gs))
    assert plan["chunks"] == NB.cdiv(rpb, 64) and plan["gs"] == int(gs)
    x = _randn(g, rows, D, scale=1.2, shift=0.5)
    dy = _randn(g, rows, D, scale=0.7, shift=0.1)
    mod = _randn(g, nb, 6 * D, scale=0.3)
    scale, gate = mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    dres = _randn(g, rows, D, scale=0.05)
    yb = _randn(g, rows, D)

    def run():
        d_shift = torch.empty(nb, D, device=dev())
        d_scale = torch.empty(nb, D, device=dev())
        d_gate = torch.empty(nb, D, device=dev()) if gs else None
        d_bias = torch.empty(D, device=dev(), dtype=BF16 if bias_bf16 else F32) if gs else None
        dx, dxg = ops.ln_modulate_bwd_stats(dy, x, scale, rpb, d_shift, d_scale, dres=dres, gate=gate, y_branch=yb if gs else None, d_gate=d_gate,
                                            d_bias=d_bias, eps=1e-6, want_gated=gs)
        return [dx, dxg, d_shift, d_scale, d_gate, d_bias]

    r1 = run()
    r2 = run()
    _same(r1, r2, "ln_modulate_bwd_stats")
    HIT.add(f"ln_stats<{plan['nc']},{int(gs)}>")
    dx, dxg, d_shift, d_scale, d_gate, d_bias = r1
    L = NB.L_ln(plan["nc"])
    st = NB.ln_stats(x.double(), 1e-6, L)
    b = torch.arange(rows, device=dev()) // rpb
    want, e = NB.ln_bwd(dy.double(), x.double(), 1 + scale.double()[b], st, L, dres=dres.double())
    _note("ln bwd", NB.check(f"ln_modulate_bwd_stats D={D} dx", dx, want, e))
    Ls = NB.L_stats(plan["chunks"])
    xh = (x.double() - st.mu[:, None]) * st.r[:, None]
    e_xh = st.r[:, None] * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * NB.U)
    v = lambda t: t.view(nb, rpb, D)
    w1, e1 = NB.colsum(v(dy.double()), Ls)
    _note("param sums", NB.check_f32(f"ln_modulate_bwd_stats D={D} rpb={rpb} d_shift", d_shift, w1, e1))
    t = dy.double() * xh
    w2, e2 = NB.colsum(v(t), Ls, v(dy.double().abs() * e_xh + NB.U * t.abs()))
    _note("param sums", NB.check_f32(f"ln_modulate_bwd_stats D={D} d_scale", d_scale, w2, e2))
    if gs:
        w3, e3 = NB.mul_stored(dx.double(), gate.double()[b])
        _note("ln bwd", NB.check(f"ln_modulate_bwd_stats D={D} dxg", dxg, w3, e3))
        t = dx.double() * yb.double()
        w4, e4 = NB.colsum(v(t), Ls, v(NB.U * t.abs()))
        _note("param sums", NB.check_f32(f"ln_modulate_bwd_stats D={D} d_gate (dx as stored)", d_gate, w4, e4))
        w5, e5 = NB.colsum(dxg.double(), NB.L_stats(nb * plan["chunks"]))
        if bias_bf16:
            _note("param sums", NB.check(f"ln_modulate_bwd_stats D={D} d_bias bf16 (dxg as stored)", d_bias.view(1, D), w5.view(1, D), e5.view(1, D)))
        else:
            _note("param sums", NB.check_f32(f"ln_modulate_bwd_stats D={D} d_bias (dxg as stored)", d_bias, w5, e5))


@pytest.mark.parametrize("M,N,rpb", [(2 * 300, 1536, 300), (4 * 1024, 3072, 1024)])
def test_scale_cols_stats(ops, M, N, rpb):
    g = _gen(500 + N)
    nb = M // rpb
    assert ops.norm_plan("cols", rpb)["chunks"] == NB.cdiv(rpb, 64)
    x, yb = _randn(g, M, N, shift=0.1), _randn(g, M, N)
    gate = _randn(g, nb, 6 * N, scale=0.5)[:, N:2 * N]

    def run():
        d_gate, d_bias = torch.empty(nb, N, device=dev()), torch.empty(N, device=dev())
        out = ops.scale_cols_stats(x, gate, rpb, y_branch=yb, d_gate=d_gate, d_bias=d_bias)
        return [out, d_gate, d_bias]

    r1, r2 = run(), run()
    _same(r1, r2, "scale_cols_stats")
    HIT.add("scale_cols_stats")
    out, d_gate, d_bias = r1
    b = torch.arange(M, device=dev()) // rpb
    w0, e0 = NB.mul_stored(x.double(), gate.double()[b])
    _note("param sums", NB.check(f"scale_cols_stats {M}x{N} out", out, w0, e0))
    Ls = NB.L_stats(NB.cdiv(rpb, 64))
    t = (x.double() * yb.double()).view(nb, rpb, N)
    w1, e1 = NB.colsum(t, Ls, NB.U * t.abs())
    _note("param sums", NB.check_f32(f"scale_cols_stats {M}x{N} d_gate", d_gate, w1, e1))
    w2, e2 = NB.colsum(out.double(), NB.L_stats(nb * NB.cdiv(rpb, 64)))
    _note("param sums", NB.check_f32(f"scale_cols_stats {M}x{N} d_bias (out as stored)", d_bias, w2, e2))


@pytest.mark.parametrize("rpb,stride,nb,N", [(4096, 4608, 2, 3072), (333, 410, 3, 1152)])
def test_colsum_rows(ops, rpb, stride, nb, N):
    g = _gen(600 + N)
    a = _randn(g, nb * stride, N, shift=0.3)
    rows = torch.stack([a[i * stride:i * stride + rpb] for i in range(nb)]).double()
    Ls = NB.L_stats(NB.cdiv(rpb, 64))
    per = torch.empty(nb, N, device=dev())
    ops.colsum_rows(a, rpb, stride, nb, per, per_batch=True)
    per2 = torch.empty(nb, N, device=dev())
    ops.colsum_rows(a, rpb, stride, nb, per2, per_batch=True)
    _same([per], [per2], "colsum_rows")
    HIT.add("colsum_rows")
    w1, e1 = NB.colsum(rows, Ls)
    _note("param sums", NB.check_f32(f"colsum_rows per batch rpb={rpb} stride={stride}", per, w1, e1))
    c0 = _randn(g, N)
    one = c0.clone()
    ops.colsum_rows(a, rpb, stride, nb, one, per_batch=False, accumulate=True)
    w2, e2 = NB.colsum(rows.reshape(-1, N), NB.L_stats(nb * NB.cdiv(rpb, 64)) + 1)
    w2 = w2 + c0.double()
    _note("param sums", NB.check(f"colsum_rows reduced bf16 accumulate rpb={rpb}", one.view(1, N), w2.view(1, N), (e2 + NB.U * w2.abs()).view(1, N)))


@pytest.mark.parametrize("S,D,nb", [(4096, 3072, 2), (1024, 1152, 4)])          # Flux, PixArt-Sigma
def test_colsum_prod(ops, S, D, nb):
    g = _gen(700 + D)
    rows = nb * S
    x = _randn(g, rows, D, scale=1.2, shift=0.2)
    dy = _randn(g, rows, D, scale=0.5, shift=0.05)
    xh = ops.layer_norm_xhat(x, eps=1e-6)
    Ls = NB.L_stats(NB.cdiv(S, 64))
    out0 = torch.empty(nb, D, device=dev())
    ops.colsum_prod(dy, out0, b=xh, rows_per_batch=S)
    out0b = torch.empty(nb, D, device=dev())
    ops.colsum_prod(dy, out0b, b=xh, rows_per_batch=S)
    _same([out0], [out0b], "colsum_prod")
    HIT.add("colsum_prod<0>")
    t = (dy.double() * xh.double()).view(nb, S, D)
    w0, e0 = NB.colsum(t, Ls, NB.U * t.abs())
    _note("param sums", NB.check_f32(f"colsum_prod mode 0 (dy x xhat as stored) S={S} D={D}", out0, w0, e0))
    # mode 1: d scale = (sum dy n - shift d shift) / (1 + scale) from the saved modulated output n
    mod = _randn(g, nb, 6 * D, scale=0.3)
    shift, scale = mod[:, 0:D], mod[:, D:2 * D]
    scale[(1 + scale.float()).abs() < 0.05] = 0          # mode 1 divides by 1 + scale (layer_norm_xhat exists for the entries where that is singular)
    n = ops.ln_modulate_fwd(x, scale, shift, S, eps=1e-6)
    dsh = torch.empty(nb, D, device=dev())
    ops.colsum_prod(dy, dsh, rows_per_batch=S)
    w_sh, e_sh = NB.colsum(dy.double().view(nb, S, D), Ls)
    _note("param sums", NB.check_f32(f"colsum_prod plain S={S} D={D}", dsh, w_sh, e_sh))
    c0 = torch.randn(nb, D, device=dev(), generator=g)
    out1 = c0.clone()
    ops.colsum_prod(dy, out1, b=n, rows_per_batch=S, mode=1, prev=dsh, shift=shift, scale=scale, accumulate=True)
    HIT.add("colsum_prod<1>")
    t = (dy.double() * n.double()).view(nb, S, D)
    Sn, eS = NB.colsum(t, Ls, NB.U * t.abs())
    sp = shift.double() * dsh.double()
    den = 1 + scale.double()
    w1 = (Sn - sp) / den
    e1 = (eS + 2 * NB.U * (Sn.abs() + sp.abs())) / den.abs() + 2 * NB.U * w1.abs()
    w1 = w1 + c0.double()
    _note("param sums", NB.check_f32(f"colsum_prod mode 1 accumulate S={S} D={D}", out1, w1, e1 + NB.U * w1.abs()))


# ------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU), both apply forms
# ------------------------------------------------------------------------------------------------
GN_CASES = [
    # B, H, W, C, silu, out_tokens, dy_tokens, dadd, accumulate, eps
    (1, 4, 4, 128, True, False, False, False, False, 1e-5),
    (4, 17, 23, 320, True, False, True, True, True, 1e-5),
    (1, 32, 32, 512, False, True, False, False, False, 1e-6),
    (4, 16, 16, 640, True, False, False, True, False, 1e-5),
    (1, 33, 31, 960, True, True, True, False, True, 1e-6),
    (4, 8, 8, 1280, True, False, False, False, False, 1e-5),
    (1, 64, 64, 1920, False, False, False, False, True, 1e-6),
    (1, 128, 128, 2048, True, False, False, False, False, 1e-5),
    (4, 12, 20, 2560, True, False, True, True, False, 1e-5),
    (1, 1024, 1024, 128, True, False, False, False, False, 1e-6),          # VAE decoder up-block count (~10^6 positions)
]


def _gn_offsets(g, B, C, G=32):
    """per (image, group) offset classes 0, 16, 64, 256 x std, plus one near-constant group (image 0, group 5)"""
    cg = C // G
    cls = torch.tensor([0.0, 16.0, 64.0, 256.0], device=dev())
    off = cls[torch.arange(B * G, device=dev()) % 4].view(B, G)
    off = off * torch.where(torch.rand(B, G, device=dev(), generator=g) < 0.5, -1.0, 1.0)
    return off.repeat_interleave(cg, 1)           # [B, C]


@pytest.mark.parametrize("form", [2, 1])
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: f"B{c[0]}_{c[1]}x{c[2]}_C{c[3]}")
def test_groupnorm(ops, form, case):
    B, H, W, C, silu, out_tokens, dy_tokens, dadd_on, accumulate, eps = case
    G, cg = 32, C // 32
    g = _gen(800 + C + H)
    prev = ops.gn_set_apply(form)
    try:
        plan = ops.norm_plan("gn", B, H, W, C)
        assert plan["form"] == form
        HIT.add(f"gn{form}_win{plan['nwin']}")
        std = 1.0 if H * W > 4096 else 0.7
        off = _gn_offsets(g, B, C)
        xt = torch.randn(B, H * W, C, device=dev(), generator=g) * std + off[:, None, :] * std
        xt[0, :, 5 * cg:6 * cg] = 3.0 + 2.0 ** -6 * (torch.arange(H * W * cg, device=dev()) % 3 == 0).view(H * W, cg)   # near-constant group
        xt = xt.to(BF16)
        n_img = (H + 2) * (W + 2)
        xg = torch.zeros(B * n_img + 64, C, device=dev(), dtype=BF16)
        xg[:B * n_img].view(B, H + 2, W + 2, C)[:, 1:H + 1, 1:W + 1] = xt.view(B, H, W, C)
        gamma, beta = _randn(g, C, scale=0.2, shift=1.0), _randn(g, C, scale=0.3)
        y, stats = ops.groupnorm_fwd(xg, gamma, beta, B, H, W, groups=G, eps=eps, silu=silu, out_tokens=out_tokens)
        y2, stats2 = ops.groupnorm_fwd(xg, gamma, beta, B, H, W, groups=G, eps=eps, silu=silu, out_tokens=out_tokens)
        _same([y, stats], [y2, stats2], "groupnorm_fwd")
        del y2, stats2
        name = f"groupnorm form {form} B{B} {H}x{W} C{C}{' silu' if silu else ''}"
        # the statistics: bound per (image, group)
        L = NB.L_gn(plan["rows_per_chunk"], NB.gn_stats_RT(C), plan["nch"], cg)
        xs = xt.double().view(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
        st = NB.ln_stats(xs, eps, L, pivoted=True)
        smu = stats[..., 0].double().view(B, G, cg)
        srs = stats[..., 1].double().view(B, G, cg)
        assert torch.equal(smu, smu[..., :1].expand_as(smu)) and torch.equal(srs, srs[..., :1].expand_as(srs)), "stats differ inside a group"
        r_mu = ((smu[..., 0].reshape(-1) - st.mu).abs() / st.e_mu).max()
        r_rs = ((srs[..., 0].reshape(-1) / st.r - 1).abs() / st.e_r).max()
        print(f"[stats] {name}: worst |mean err| / bound = {float(r_mu):.3f}, worst |rstd rel err| / bound = {float(r_rs):.3f}")
        assert float(r_mu) <= 1 and float(r_rs) <= 1, (name, float(r_mu), float(r_rs))
        gam = gamma.double().view(1, 1, G, cg).expand(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
        bet = beta.double().view(1, 1, G, cg).expand(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
        want, e, dmu, dlr = NB.norm_fwd(xs, st, gam, bet, silu=silu)
        if out_tokens:
            yt = y.view(B, H * W, C)
        else:
            yg = y[:B * n_img].view(B, H + 2, W + 2, C)
            border = torch.ones(H + 2, W + 2, dtype=torch.bool, device=dev())
            border[1:H + 1, 1:W + 1] = False
            assert not bool(yg[:, border].view(torch.int16).any()), f"{name}: grid border not exactly zero"
            yt = yg[:, 1:H + 1, 1:W + 1].reshape(B, H * W, C)
        ys = yt.view(B, H * W, G, cg).permute(0, 2, 1, 3).reshape(B * G, -1)
        _note("groupnorm", NB.check(name + " y", ys.reshape(B * G * H * W, cg), want.reshape(-1, cg), e.reshape(-1, cg), blocks=False))
        _note("groupnorm", NB.fit_rows(name + " y", ys, want, e, dmu, dlr, st.e_mu, st.e_r))
        del want, e, dmu, dlr, ys, yt, y
        # backward, chained on the statistics the forward stored
        dyt = _randn(g, B, H * W, C, scale=0.5, shift=0.05)
        if dy_tokens:
            dy = dyt.view(B * H * W, C)
        else:
            dy = torch.zeros(B * n_img + 64, C, device=dev(), dtype=BF16)
            dy[:B * n_img].view(B, H + 2, W + 2, C)[:, 1:H + 1, 1:W + 1] = dyt.view(B, H, W, C)
        dadd = None
        if dadd_on:
            dadd = torch.zeros(B * n_img + 64, C, device=dev(), dtype=BF16)
            dadd[:B * n_img].view(B, H + 2, W + 2, C)[:, 1:H + 1, 1:W + 1] = _randn(g, B, H, W, C, scale=0.1)
        c0 = torch.randn(2, C, device=dev(), generator=g)

        def bwd():
            dg_, db_ = c0[0].clone(), c0[1].clone()
            dx_ = ops.groupnorm_bwd(dy, xg, gamma, beta, stats, B, H, W, groups=G, silu=silu, dy_tokens=dy_tokens, dadd=dadd, dgamma=dg_, dbeta=db_,
                                    accumulate_params=accumulate)
            return [dx_, dg_, db_]

        r1 = bwd()
        _same(r1, bwd(), "groupnorm_bwd")
        dx, dgam, dbet = r1
        mu_f = stats[..., 0].double()[:, None, :]
        r_f = stats[..., 1].double()[:, None, :]
        xd = xt.double()
        xh = (xd - mu_f) * r_f
        ga, be = gamma.double(), beta.double()
        dyd = dyt.double()
        if silu:
            z = xh * ga + be
            s = torch.sigmoid(z)
            sp = s * (1 + z * (1 - s))
            spp = s * (1 - s) * (2 + z * (1 - 2 * s))
            gg = dyd * sp
            e_g = gg.abs() * (2.0 ** -21 * (2 + z.abs()) + 6 * NB.U) + dyd.abs() * spp.abs() * (ga.abs() * 2 * NB.U * xh.abs() + NB.U * z.abs())
            del z, s, sp, spp
        else:
            gg = dyd
            e_g = torch.zeros_like(gg)
        Lb = L + 3
        n = H * W * cg
        grp = lambda t: t.view(B, H * W, G, cg).sum((1, 3))          # [B, G]
        S1, S2 = grp(ga * gg), grp(ga * gg * xh)
        eS1 = Lb * NB.U * grp((ga * gg).abs()) + grp(ga.abs() * e_g)
        eS2 = Lb * NB.U * grp((ga * gg * xh).abs()) + grp(ga.abs() * (e_g * xh.abs() + gg.abs() * 2 * NB.U * xh.abs()))
        ex = lambda t: t.repeat_interleave(cg, 1)[:, None, :]          # [B, G] -> [B, 1, C]
        c2, c3 = -r_f * ex(S2) / n, -r_f * ex(S1) / n
        c1 = r_f * ga
        want = c1 * gg + c2 * xh + c3
        e = r_f * (ga.abs() * e_g + xh.abs() * ex(eS2) / n + ex(eS1) / n) + 4 * NB.U * ((c1 * gg).abs() + (c2 * xh).abs() + c3.abs()) + c2.abs() * 2 * NB.U * xh.abs()
        if dadd_on:
            want = want + dadd[:B * n_img].view(B, H + 2, W + 2, C)[:, 1:H + 1, 1:W + 1].reshape(B, H * W, C).double()
        e = e + NB.U * want.abs()
        dxg = dx[:B * n_img].view(B, H + 2, W + 2, C)
        border = torch.ones(H + 2, W + 2, dtype=torch.bool, device=dev())
        border[1:H + 1, 1:W + 1] = False
        assert not bool(dxg[:, border].view(torch.int16).any()), f"{name}: dx grid border not exactly zero"
        _note("groupnorm bwd", NB.check(name + " dx", dxg[:, 1:H + 1, 1:W + 1].reshape(-1, C), want.view(-1, C), e.view(-1, C)))
        del want, e
        Lp = NB.L_gn_params(plan["rows_per_chunk"], NB.gn_stats_RT(C), plan["nch"], B) + (1 if accumulate else 0)
        t = (gg * xh).view(-1, C)
        wg, eg = NB.colsum(t, Lp, (e_g * xh.abs() + gg.abs() * 2 * NB.U * xh.abs() + NB.U * (gg * xh).abs()).view(-1, C))
        wb, eb = NB.colsum(gg.view(-1, C), Lp, e_g.view(-1, C))
        if accumulate:
            wg, wb = wg + c0[0].double(), wb + c0[1].double()
        _note("groupnorm bwd", NB.check_f32(name + " dgamma", dgam, wg, eg))
        _note("groupnorm bwd", NB.check_f32(name + " dbeta", dbet, wb, eb))
    finally:
        ops.gn_set_apply(prev)


# ------------------------------------------------------------------------------------------------
# q / k RMSNorm + RoPE
# ------------------------------------------------------------------------------------------------
def _rope_tables(S, hd, base=10000.0):
    freq = base ** (-torch.arange(0, hd, 2, device=dev(), dtype=F64) / hd)
    ang = torch.arange(S, device=dev(), dtype=F64)[:, None] * freq[None, :] * 0.37
    return ang.cos().repeat_interleave(2, 1).float().contiguous(), ang.sin().repeat_interleave(2, 1).float().contiguous()


QK_CASES = [
    # B, H, d, split (txt rows or 0), S, Sp, with weights, Qt/Kt
    (2, 4, 64, 0, 200, 256, True, True),
    (2, 3, 64, 77, 77 + 250, 384, False, False),
    (1, 4, 128, 100, 100 + 300, 448, True, True),
    (2, 2, 128, 0, 129, 192, True, False),
    (2, 24, 128, 0, 1024, 1024, True, False),
]


def _qk_inputs(g, B, H, d, S, wts):
    D = H * d
    qkv_buf = _randn(g, B * S, 3 * D + 8, scale=1.3, shift=0.1)
    qkv = qkv_buf[:, :3 * D]
    wq, wk = (_randn(g, d, scale=0.2, shift=1.0), _randn(g, d, scale=0.2, shift=1.0)) if wts else (None, None)
    return qkv, wq, wk


def _head_major(qkv, B, H, d, S, part):
    D = H * d
    return qkv[:, part * D:(part + 1) * D].reshape(B, S, H, d).permute(0, 2, 1, 3)


@pytest.mark.parametrize("case", QK_CASES, ids=lambda c: f"B{c[0]}H{c[1]}d{c[2]}_S{c[4]}_split{c[3]}_w{int(c[6])}_t{int(c[7])}")
def test_qk_norm_rope(ops, case):
    B, H, d, St, S, Sp, wts, with_t = case
    g = _gen(900 + S + d)
    qkv, wq, wk = _qk_inputs(g, B, H, d, S, wts)
    cs, sn = _rope_tables(S, d)
    parts = [(St, 0), (S - St, St)] if St else [(S, 0)]
    Q = torch.zeros(B, H, S, d, device=dev(), dtype=BF16)
    K = torch.zeros_like(Q)
    Qt = torch.zeros(B, H, d, Sp, device=dev(), dtype=BF16) if with_t else None
    Kt = torch.zeros_like(Qt) if with_t else None
    Vt = torch.zeros(B, H, d, Sp, device=dev(), dtype=BF16)
    for S_part, pos0 in parts:
        plan = ops.norm_plan("qk", d, B, H, S_part)
        assert plan["hd"] == d
        ops.qk_norm_rope_fwd(qkv, wq, wk, cs, sn, Q, K, Qt, Kt, Vt, B, H, d, S_part, pos0, S, Sp, eps=1e-6)
    first = _clone([Q, K, Qt, Kt, Vt])
    for S_part, pos0 in parts:
        ops.qk_norm_rope_fwd(qkv, wq, wk, cs, sn, Q, K, Qt, Kt, Vt, B, H, d, S_part, pos0, S, Sp, eps=1e-6)
    _same([Q, K, Qt, Kt, Vt], first, "qk_norm_rope_fwd")
    HIT.add(f"qk_fwd<{d}>")
    cs4, sn4 = cs.double()[None, None], sn.double()[None, None]
    for part, w, out, outT in ((0, wq, Q, Qt), (1, wk, K, Kt)):
        x = _head_major(qkv, B, H, d, S, part).double()
        want, e, dlr = NB.qk_fwd(x, None if w is None else w.double(), cs4, sn4, 1e-6)
        nm = f"qk_norm_rope_fwd B{B} H{H} d{d} S{S} {'q' if part == 0 else 'k'}{' norm' if w is not None else ''}"
        _note("qk", NB.check(nm, out.reshape(-1, d), want.reshape(-1, d), e.reshape(-1, d)))
        R = B * H * S
        _note("qk", NB.fit_rows(nm, out.reshape(R, d), want.reshape(R, d), e.reshape(R, d), torch.ones(R, d, device=dev(), dtype=F64), dlr.reshape(R, d),
                                torch.zeros(R, device=dev(), dtype=F64), torch.zeros(R, device=dev(), dtype=F64)))
        if outT is not None:
            assert torch.equal(outT[..., :S].view(torch.int16), out.transpose(-1, -2).contiguous().view(torch.int16)), f"{nm}: transposed copy"
            assert not bool(outT[..., S:].view(torch.int16).any()), f"{nm}: Sp > S padding not zero"
    V = _head_major(qkv, B, H, d, S, 2)
    assert torch.equal(Vt[..., :S].view(torch.int16), V.transpose(-1, -2).contiguous().view(torch.int16)), "V is passed through bit-exact"
    assert not bool(Vt[..., S:].view(torch.int16).any()), "Vt padding not zero"

    # backward (+ the norm-weight gradient with accumulate over the txt / img parts)
    dQ, dK = _randn(g, B, H, S, d, scale=0.5, shift=0.05), _randn(g, B, H, S, d, scale=0.5, shift=0.05)
    D = H * d

    def bwd(wgrad):
        dqkv = torch.full((B * S, 3 * D + 8), 7.0, device=dev(), dtype=BF16)
        gw = [None if w is None else torch.zeros(d, device=dev(), dtype=BF16) for w in (wq, wk)]
        for i, (S_part, pos0) in enumerate(parts):
            if wgrad:
                ops.qk_norm_rope_bwd_wgrad(dQ, dK, qkv, wq, wk, cs, sn, dqkv, B, H, d, S_part, pos0, S, gw[0], gw[1], accumulate=i > 0, eps=1e-6)
            else:
                ops.qk_norm_rope_bwd(dQ, dK, qkv, wq, wk, cs, sn, dqkv, B, H, d, S_part, pos0, S, eps=1e-6)
        return [dqkv] + gw

    r1 = bwd(False)
    _same(r1, bwd(False), "qk_norm_rope_bwd")
    HIT.add(f"qk_bwd<{d}>")
    dqkv = r1[0]
    assert bool((dqkv[:, 2 * D:] == 7.0).all()), "the backward wrote into the v / padding columns"
    terms = {}
    for part, w, gI in ((0, wq, dQ), (1, wk, dK)):
        x = _head_major(qkv, B, H, d, S, part).double()
        want, e, dy, e_dy, r, e_r = NB.qk_bwd(gI.double(), x, None if w is None else w.double(), cs4, sn4, 1e-6)
        got = _head_major(dqkv, B, H, d, S, part)
        _note("qk bwd", NB.check(f"qk_norm_rope_bwd B{B} H{H} d{d} S{S} part {part}", got.reshape(-1, d), want.reshape(-1, d), e.reshape(-1, d)))
        if w is not None:
            terms[part] = (dy * x * r, x.abs() * r * e_dy + (dy * x * r).abs() * (e_r + 2 * NB.U))
    if wts:
        r3 = bwd(True)
        _same(r3, bwd(True), "qk_norm_rope_bwd_wgrad")
        assert torch.equal(r3[0].view(torch.int16), dqkv.view(torch.int16)), "the wgrad form must write the same dqkv"
        for part in (0, 1):
            t, et = terms[part]
            want = torch.zeros(d, device=dev(), dtype=F64)
            e = torch.zeros(d, device=dev(), dtype=F64)
            for S_part, pos0 in parts:
                plan = ops.norm_plan("qk", d, B, H, S_part)
                HIT.add(f"qk_wgrad<{d},{'64' if plan['ns'] == 64 else 'few'}>")
                sl = t[:, :, pos0:pos0 + S_part].reshape(-1, d)
                w_, e_ = NB.colsum(sl, NB.L_qk_wgrad(d, plan["ns"], plan["per"]) + 1, et[:, :, pos0:pos0 + S_part].reshape(-1, d))
                if pos0 > 0:            # accumulate: the first part was stored as bf16 (one rounding) and is read back
                    e = e + 0.5 * NB.ulp_bf16(want.abs() + e)
                want = want + w_
                e = e + e_ + NB.U * want.abs()
            _note("qk wgrad", NB.check(f"qk wgrad B{B} H{H} d{d} S{S} part {part}", r3[1 + part].view(1, d), want.view(1, d), e.view(1, d), blocks=False))


@pytest.mark.parametrize("B,H,S,accumulate", [(8, 24, 4608, True), (1, 24, 512 + 40, False)])       # Flux (nblk = 13 824: 64 slices) and a short one
def test_qk_wgrad_slices(ops, B, H, S, accumulate):
    d = 128
    g = _gen(950 + S)
    qkv, wq, wk = _qk_inputs(g, B, H, d, S, True)
    cs, sn = _rope_tables(S, d)
    plan = ops.norm_plan("qk", d, B, H, S)
    assert (plan["ns"] == 64) == (plan["nblk"] >= 2048)
    HIT.add(f"qk_wgrad<{d},{'64' if plan['ns'] == 64 else 'few'}>")
    dQ, dK = _randn(g, B, H, S, d, scale=0.5, shift=0.05), _randn(g, B, H, S, d, scale=0.5, shift=0.05)
    c0 = _randn(g, 2, d, scale=5.0)

    def run():
        dqkv = torch.empty(B * S, 3 * H * d + 8, device=dev(), dtype=BF16)
        gwq, gwk = c0[0].clone(), c0[1].clone()
        ops.qk_norm_rope_bwd_wgrad(dQ, dK, qkv, wq, wk, cs, sn, dqkv, B, H, d, S, 0, S, gwq, gwk, accumulate=accumulate, eps=1e-6)
        return [gwq, gwk]

    r1 = run()
    _same(r1, run(), "qk wgrad")
    cs4, sn4 = cs.double()[None, None], sn.double()[None, None]
    for part, w, gI in ((0, wq, dQ), (1, wk, dK)):
        x = _head_major(qkv, B, H, d, S, part).double()
        _, _, dy, e_dy, r, e_r = NB.qk_bwd(gI.double(), x, w.double(), cs4, sn4, 1e-6)
        t = dy * x * r
        want, e = NB.colsum(t.reshape(-1, d), NB.L_qk_wgrad(d, plan["ns"], plan["per"]) + 1,
                            (x.abs() * r * e_dy + t.abs() * (e_r + 2 * NB.U)).reshape(-1, d))
        del x, dy, e_dy, t
        if accumulate:
            want = want + c0[part].double()
        _note("qk wgrad", NB.check(f"qk wgrad B{B} H{H} S{S} nblk={plan['nblk']} ns={plan['ns']} per={plan['per']} part {part}", r1[part].view(1, d),
                                   want.view(1, d), (e + NB.U * want.abs()).view(1, d), blocks=False))


@pytest.mark.parametrize("B,H,St,Si,wts", [(2, 2, 256, 512, True), (1, 4, 0, 256, False)])       # the fused epilogue: H even, streams of 256k rows
def test_qk_rope_norm_bwd(ops, B, H, St, Si, wts):
    """chained on the stored Q / K / 1/rms of the fused EPI_QK_NORM_ROPE projection (st355_gemm_bf16)"""
    d, Kin = 128, 192
    S, D = St + Si, H * d
    g = _gen(990 + S)
    cs, sn = _rope_tables(S, d)
    cs_p, sn_p = cs[:, 0::2].contiguous(), sn[:, 0::2].contiguous()
    Q = torch.zeros(B, H, S, d, device=dev(), dtype=BF16)
    Kh = torch.zeros_like(Q)
    rrms = torch.zeros(B * S, 2 * H, device=dev())
    V = torch.zeros(B * S, D, device=dev(), dtype=BF16)
    wq, wk = (_randn(g, d, scale=0.2, shift=1.0), _randn(g, d, scale=0.2, shift=1.0)) if wts else (None, None)
    parts = [(St, 0), (Si, St)] if St else [(Si, 0)]
    for rows, pos0 in parts:
        x = _randn(g, B * rows, Kin)
        W = _randn(g, 3 * D, Kin, scale=0.08)
        ops.gemm(x, W, out=V.view(B, S, D)[:, pos0:pos0 + rows], epilogue=ops.EPI_QK_NORM_ROPE,
                 rope=ops.qk_rope(Q, Kh, rrms, wq, wk, cs_p, sn_p, H, S, pos0), rows_per_batch=rows)
    dQ, dK = _randn(g, B, H, S, d, scale=0.5), _randn(g, B, H, S, d, scale=0.5)

    def run():
        dqkv = torch.full((B * S, 3 * D), 7.0, device=dev(), dtype=BF16)
        for rows, pos0 in parts:
            ops.qk_rope_norm_bwd(dQ, dK, Q, Kh, rrms, wq, wk, cs, sn, dqkv, B, H, d, rows, pos0, S)
        return [dqkv]

    r1 = run()
    _same(r1, run(), "qk_rope_norm_bwd")
    HIT.add("qk_rope_norm_bwd<128>")
    dqkv = r1[0]
    assert bool((dqkv[:, 2 * D:] == 7.0).all())
    cs4, sn4 = cs.double()[None, None], sn.double()[None, None]
    for part, w, gI, z in ((0, wq, dQ, Q), (1, wk, dK, Kh)):
        rr = rrms.view(B, S, 2, H)[:, :, part].permute(0, 2, 1).double()[..., None] if w is not None else None
        want, e = NB.qk_rope_norm_bwd(gI.double(), z.double(), rr, None if w is None else w.double(), cs4, sn4)
        got = _head_major(dqkv, B, H, d, S, part)
        _note("qk bwd", NB.check(f"qk_rope_norm_bwd B{B} H{H} S{S} part {part}{' norm' if w is not None else ''}", got.reshape(-1, d), want.reshape(-1, d),
                                 e.reshape(-1, d)))


def test_every_route_reached():
    for fam, w in sorted(WORST.items()):
        print(f"[worst] {fam}: err/tol {w['err/tol']:.3f}, block {w['block']:.3f}, row offset {w['offset SE']:.2f} SE, row slope {w['slope SE']:.2f} SE")
    missing = ALL_ROUTES - HIT
    assert not missing, f"instances no case reached: {sorted(missing)} (run the module as a whole)"

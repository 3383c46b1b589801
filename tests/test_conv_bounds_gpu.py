"""Every instance of the convolution path, element-wise against fp64 references built in image space (tests/conv_bounds.py).

Each case first asserts what it runs on (ops.conv_plan / ops.conv_wgrad_plan -> st355_conv_plan: the helpers the launchers call), runs twice into fresh buffers
(bit-identical, split-K included), then checks the exact part of the contract (kept rows, zero border, every computed row written) and bounds every interior output
element by element and per 64 x 64 block.  Operands and outputs (the grid buffers the wrappers allocate for the layout passes included) are views into larger allocations whose surroundings hold NaN (inputs) or a
sentinel (outputs): a
read from outside a grid buffer that reaches an output, or a write outside the documented range, fails.  The last test asserts that the cases reached every
instance: run the module as a whole."""
import ctypes as C
import math

import pytest
import torch

from tests import conv_bounds as CB
from tests import gemm_bounds as GB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GUARD = 320                       # rows of NaN / sentinel on either side of every operand / output
HIT = set()
WORST = {}                        # family -> (worst err/tol, worst block RMS)
ALL = ({("fwd", k, e, t) for k in ("pq_conv", "s2") for e in ("NONE", "ADD") for t in (9, 1)}
       | {("dead", d) for d in (0, 2, 3)}
       | {("wgrad", t, s) for t in (9, 1) for s in ("SPLITK", "NONE", "ADD")}
       | {("layout", k) for k in ("grid_from_nchw", "grid_to_nchw", "im2col3x3", "col2im3x3", "upsample2x", "upsample2x_bwd", "tokens_to_grid",
                                  "tokens_to_grid+residual", "grid_to_tokens")})


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, scale=1.0, data="unit"):
    """unit: N(0, scale^2); offset: a large common offset, mean / std = 16; outlier: a few 2^8-scaled values per row of the last axis"""
    v = torch.randn(*shape, device=dev(), generator=g)
    if data == "offset":
        v += 16.0
    if data == "outlier":
        hit = torch.rand(*shape, device=dev(), generator=g) < 4.0 / shape[-1]
        v = torch.where(hit, v * 256.0, v)
    return (v * scale).to(BF16)


def _guarded2(t, fill=float("nan")):
    """(whole, view): a copy of t inside a larger allocation filled with NaN (or the sentinel); 16-byte alignment kept"""
    flat = t.reshape(-1)
    pad = GUARD * (t.shape[-1] if t.dim() > 1 else 8)
    whole = torch.full((flat.numel() + 2 * pad,), fill, dtype=t.dtype, device=t.device)
    view = whole[pad:pad + flat.numel()].view(t.shape)
    view.copy_(t)
    return whole, view


def _guarded(t, fill=float("nan")):
    return _guarded2(t, fill)[1]


def _twice(name, fn):
    """run a pass twice into fresh outputs: bit-identical"""
    a, b = fn(), fn()
    assert a.shape == b.shape and torch.equal(CB._bits(a), CB._bits(b)), f"{name}: a second launch differs"
    return a


def _note(family, rep):
    w = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(w[0], rep.worst), max(w[1], rep.block_rms))
    GB.assert_bound(rep)


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------------------
def _forward(ops, name, B, H, W, Cin, Cout, taps, epi, kernel, dead, data="unit", seed=0, wide_img_add=False, sel=None, x_img=None):
    g = _gen(seed)
    if x_img is None:
        x_img = _randn(g, B, H, W, Cin, data=data)
    w = _guarded(_randn(g, Cout, taps * Cin, scale=1 / math.sqrt(taps * Cin)))
    bias = _guarded(_randn(g, Cout, scale=0.5)) if epi >= 1 else None
    temb = None
    if epi >= 2:
        temb = torch.full((B, Cout + (64 if wide_img_add else 0)), float("nan"), dtype=BF16, device=dev())
        temb[:, :Cout] = _randn(g, B, Cout)
        temb = temb[:, :Cout]                                            # row stride Cout + 64: the columns beyond Cout are NaN
    res_img = _randn(g, B, H, W, Cout, data=data) if epi >= 3 else None
    plan = ops.conv_plan(B, H, W, Cin, Cout, taps, residual=res_img is not None)
    assert (plan["kernel"], plan["epilogue"], plan["dead"]) == (kernel, "ADD" if epi >= 3 else "NONE", dead), f"{name}: planned {plan}"
    HIT.add(("fwd", kernel, plan["epilogue"], taps))
    if kernel == "pq_conv":
        HIT.add(("dead", dead))
    xg = _guarded(CB.image_to_grid(x_img))
    rg = _guarded(CB.image_to_grid(res_img)) if res_img is not None else None
    outs = []
    for _ in range(2):
        whole, out = CB.conv_out_buffer(B, H, W, Cout, dev(), guard=GUARD)
        ops.conv(xg, w, B, H, W, bias=bias, img_add=temb, residual=rg, taps=taps, out=out)
        outs.append((whole, out))
    assert torch.equal(CB._bits(outs[0][0]), CB._bits(outs[1][0])), f"{name}: a second launch differs"
    whole, out = outs[0]
    del outs
    CB.check_conv_exact(name, out, B, H, W, whole=whole, guard=GUARD)
    want, e = CB.conv_ref(x_img, w, taps, bias, temb, res_img, sel=sel)
    tile = (256, 256) if kernel == "pq_conv" else (128, 128)
    _note("forward", CB.check_conv(f"{kernel} {name}", out, want, e, B, H, W, sel=sel, tile=tile))
    return out


EPI_NAMES = ["none", "bias", "bias+img_add", "bias+img_add+residual"]


@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
@pytest.mark.parametrize("kernel,B,H,W,dead", [("pq_conv", 4, 64, 64, 3), ("s2", 2, 32, 32, 0)])
def test_forward_every_epilogue_on_both_kernels(ops, kernel, B, H, W, dead, epi, taps):
    _forward(ops, f"{EPI_NAMES[epi]} taps {taps} B{B} {H}x{W} 64->320", B, H, W, 64, 320, taps, epi, kernel, dead, seed=10 + epi, wide_img_add=(epi == 2))


FWD_SHAPES = [
    # B, H, W, Cin, Cout, taps, epilogue, kernel, dead wave groups, data                     the SDXL 1024^2 levels at batch 4, down and up path widths
    (4, 128, 128, 320, 320, 9, 3, "pq_conv", 3, "unit"),
    (4, 128, 128, 960, 320, 9, 2, "pq_conv", 3, "unit"),
    (4, 64, 64, 640, 640, 9, 3, "pq_conv", 2, "offset"),
    (4, 64, 64, 1920, 640, 9, 2, "pq_conv", 2, "unit"),
    (4, 64, 64, 320, 640, 1, 0, "pq_conv", 2, "outlier"),          # the 1x1 shortcut
    (4, 32, 32, 1280, 1280, 9, 3, "s2", 0, "unit"),
    (4, 32, 32, 2560, 1280, 9, 2, "s2", 0, "outlier"),
    (4, 32, 32, 640, 1280, 1, 1, "s2", 0, "offset"),
    (4, 128, 128, 320, 8, 9, 1, "pq_conv", 3, "unit"),             # conv_out: 4 channels padded to 8
    (4, 128, 128, 128, 320, 1, 1, "pq_conv", 3, "unit"),           # conv_in from pre-gathered columns (K 72 -> 128)
    (4, 128, 128, 64, 72, 9, 1, "pq_conv", 2, "unit"),
    (2, 32, 32, 64, 72, 9, 3, "s2", 0, "unit"),                    # ragged last column tile on s2
    (2, 32, 32, 64, 8, 9, 1, "s2", 0, "unit"),
    (4, 152, 104, 320, 320, 9, 3, "pq_conv", 3, "unit"),           # a non-square bucket
    # SD 1.5 at batch 1
    (1, 64, 64, 320, 320, 9, 3, "s2", 0, "unit"),
    (1, 32, 32, 640, 640, 9, 2, "s2", 0, "unit"),
    (1, 16, 16, 1280, 1280, 9, 3, "s2", 0, "offset"),
    (1, 8, 8, 1280, 1280, 9, 2, "s2", 0, "unit"),
    # VAE widths
    (2, 128, 128, 128, 128, 9, 1, "pq_conv", 2, "unit"),
    (1, 512, 512, 256, 256, 9, 3, "pq_conv", 0, "unit"),
    (1, 256, 256, 512, 512, 9, 1, "pq_conv", 0, "outlier"),
    # edges: odd sizes, 1 x 1, W = 1, a 256-row tile over four images
    (1, 9, 7, 64, 72, 9, 3, "s2", 0, "unit"),
    (3, 1, 1, 64, 64, 9, 3, "s2", 0, "unit"),
    (2, 5, 1, 64, 64, 9, 2, "s2", 0, "unit"),
    (9, 6, 6, 64, 64, 9, 3, "s2", 0, "unit"),
    (9, 6, 6, 64, 64, 1, 3, "s2", 0, "unit"),
    (72, 14, 14, 64, 320, 9, 3, "pq_conv", 3, "unit"),             # 256 grid positions per image: every 256-row tile of the big kernel straddles two images
    (264, 6, 6, 64, 320, 9, 3, "pq_conv", 3, "unit"),              # 64 per image: four or five images in every 256-row tile
]


@pytest.mark.parametrize("case", FWD_SHAPES, ids=lambda c: "B{}_{}x{}_{}to{}_t{}_e{}_{}".format(*c[:7], c[9]))
def test_forward_at_the_model_shapes_and_edges(ops, case):
    B, H, W, Cin, Cout, taps, epi, kernel, dead, data = case
    _forward(ops, f"B{B} {H}x{W} {Cin}->{Cout} taps {taps} {EPI_NAMES[epi]} {data}", B, H, W, Cin, Cout, taps, epi, kernel, dead, data=data, seed=sum(case[:5]),
             wide_img_add=True)


def test_forward_grid_larger_than_4_gib_on_sampled_rows(ops):
    """VAE width 128 at 1024^2, batch 16: input and output grids of 4.3 GB each.  The sample holds the first and the last 256-row tile in full, the first and last
    interior row of every image, and one position in 64 overall; border, kept rows and the NaN pre-fill are checked over the whole output."""
    B, H, W, Cn = 16, 1024, 1024, 128
    g = _gen(77)
    x_img = torch.empty(B, H, W, Cn, dtype=BF16, device=dev())
    for b in range(B):
        x_img[b] = _randn(g, H, W, Cn)
    rows = CB.interior_rows(B, H, W, dev())
    assert (rows.numel() + 64) * Cn * 2 > 4 << 30
    m = rows - (W + 3)
    n_pos = B * H * W
    y = (torch.arange(n_pos, device=dev()) // W) % H
    pick = (m < 256) | (m >= (int(m[-1]) // 256) * 256) | (y == 0) | (y == H - 1) | (torch.arange(n_pos, device=dev()) % 64 == 17)
    sel = pick.nonzero().view(-1)
    assert sel.numel() * 64 >= n_pos and bool(pick[m < 256].all()) and bool(pick[m >= (int(m[-1]) // 256) * 256].all())
    del pick, y, m, rows
    _forward(ops, "B16 1024x1024 128->128 (> 4 GiB), sampled", B, H, W, Cn, Cn, 9, 1, "pq_conv", 2, seed=78, sel=sel, x_img=x_img)


# ---- input gradient, as the UNet runs it ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,taps,kernel,dead,data", [(4, 64, 64, 320, 640, 9, "pq_conv", 3, "unit"), (4, 32, 32, 1280, 640, 9, "s2", 0, "offset"),
                                                                  (4, 64, 64, 320, 640, 1, "pq_conv", 3, "outlier"), (1, 9, 7, 64, 128, 9, "s2", 0, "unit")])
def test_input_gradient_with_the_models_flipped_transposed_weight(ops, B, H, W, Cin, Cout, taps, kernel, dead, data):
    g = _gen(5 + Cin)
    w = _randn(g, Cout, taps * Cin, scale=1 / math.sqrt(taps * Cin))
    dy_img = _randn(g, B, H, W, Cout, data=data)
    wT = torch.empty(Cin, taps * Cout, dtype=BF16, device=dev())
    wT.view(Cin, taps, Cout).copy_(w.view(Cout, taps, Cin).flip(1).permute(2, 1, 0))            # unet.py: flipped taps, transposed
    plan = ops.conv_plan(B, H, W, Cout, Cin, taps)
    assert (plan["kernel"], plan["dead"]) == (kernel, dead), plan
    HIT.add(("fwd", kernel, "NONE", taps))
    dyg, wTg = _guarded(CB.image_to_grid(dy_img)), _guarded(wT)
    whole, out = CB.conv_out_buffer(B, H, W, Cin, dev(), guard=GUARD)
    ops.conv(dyg, wTg, B, H, W, taps=taps, out=out)
    whole2, out2 = CB.conv_out_buffer(B, H, W, Cin, dev(), guard=GUARD)
    ops.conv(dyg, wTg, B, H, W, taps=taps, out=out2)
    assert torch.equal(CB._bits(whole), CB._bits(whole2)), "input gradient: a second launch differs"
    CB.check_conv_exact("input gradient", out, B, H, W, whole=whole, guard=GUARD)
    want, e = CB.dgrad_ref(dy_img, w, taps)
    _note("input gradient", CB.check_conv(f"{kernel} dgrad B{B} {H}x{W} {Cout}->{Cin} taps {taps} {data}", out, want, e, B, H, W))


def test_input_gradient_of_conv_out_in_column_form(ops):
    """conv_out (Cin 320 -> 4 channels padded to 8): dy gathered to columns (72 -> 128), one taps-1 convolution with wT[:, :72] = flipped, transposed taps"""
    B, H, W, Cin = 4, 128, 128, 320
    g = _gen(9)
    w = _randn(g, 8, 9 * Cin, scale=1 / math.sqrt(9 * Cin))
    w[4:] = 0
    dy_img = _randn(g, B, H, W, 8)
    dy_img[..., 4:] = 0
    wT = torch.zeros(Cin, 128, dtype=BF16, device=dev())
    wT[:, :72].view(Cin, 9, 8).copy_(w.view(8, 9, Cin).flip(1).permute(2, 1, 0))
    dcol = ops.im2col3x3(CB.image_to_grid(dy_img), B, H, W, stride=1)
    CB.check_grid_copy("im2col3x3 of dy (8 channels, K 72 -> 128)", dcol, CB.im2col_expect(dy_img, 1, 1, 128))
    HIT.add(("layout", "im2col3x3"))
    assert ops.conv_plan(B, H, W, 128, Cin, 1)["kernel"] == "pq_conv"
    whole, out = CB.conv_out_buffer(B, H, W, Cin, dev(), guard=GUARD)
    ops.conv(_guarded(dcol), _guarded(wT), B, H, W, taps=1, out=out)
    CB.check_conv_exact("conv_out input gradient", out, B, H, W, whole=whole, guard=GUARD)
    want, e = CB.dgrad_ref(dy_img, w, 9, K=128)
    _note("input gradient", CB.check_conv("pq_conv conv_out dgrad (column form)", out, want, e, B, H, W))


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------------------------
def _wgrad(ops, name, B, H, W, Cin, Cout, taps, accumulate, store, ks, data="unit", seed=0, workspace_bytes=None):
    from simpletuner_amd import lib

    g = _gen(seed)
    x_img = _randn(g, B, H, W, Cin, data=data)
    dy_img = _randn(g, B, H, W, Cout, data="unit" if data == "offset" else data)
    old = _randn(g, Cout, taps * Cin, scale=math.sqrt(B * H * W)) if accumulate else None
    ws_bytes = workspace_bytes if workspace_bytes is not None else ops._gemm_workspace(dev()).numel()
    plan = ops.conv_wgrad_plan(B, H, W, Cin, Cout, taps, accumulate=accumulate, workspace_bytes=ws_bytes)
    assert (plan["taps"], plan["store"], plan["ks"]) == (taps, store, ks), f"{name}: planned {plan}"
    assert plan["Mc"] == (CB.grid_positions(B, H, W) - 2 * (W + 3) + 63) // 64 * 64
    HIT.add(("wgrad", taps, store))
    xg, dyg = _guarded(CB.image_to_grid(x_img)), _guarded(CB.image_to_grid(dy_img))
    got = []
    for _ in range(2):
        whole, dw = _guarded2(old if accumulate else torch.full((Cout, taps * Cin), float("nan"), dtype=BF16, device=dev()), fill=CB.SENTINEL)
        if workspace_bytes is None:
            ops.conv_wgrad(xg, dyg, dw, B, H, W, taps=taps, accumulate=accumulate)
        else:
            ws = torch.full((workspace_bytes // 4,), float("nan"), device=dev())
            lib.check(lib.load().st355_conv_wgrad_bf16(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(xg.data_ptr()), C.c_void_p(dyg.data_ptr()),
                                                       C.c_void_p(dw.data_ptr()), B, H, W, Cin, Cout, taps, 1 if accumulate else 0, C.c_void_p(ws.data_ptr()),
                                                       workspace_bytes), "conv_wgrad_bf16")
        got.append((whole, dw))
    assert torch.equal(CB._bits(got[0][0]), CB._bits(got[1][0])), f"{name}: a second launch differs"
    pad = GUARD * taps * Cin
    s = torch.tensor(CB.SENTINEL, dtype=BF16, device=dev()).view(torch.int16)
    assert bool((CB._bits(got[0][0][:pad]) == s).all()) and bool((CB._bits(got[0][0][-pad:]) == s).all()), f"{name}: a write outside dw"
    want, e = CB.wgrad_ref(x_img, dy_img, taps, plan["Mc"], plan["ks"], old)
    _note("weight gradient", GB.check(f"wgrad {name}", got[0][1], want, e))


WGRAD = [
    # B, H, W, Cin, Cout, taps, accumulate, store, ks, data
    (4, 128, 128, 320, 320, 9, False, "SPLITK", 7, "unit"),         # the largest real contraction: batch 4 x the 128^2 level, 67392 rows
    (4, 128, 128, 320, 320, 9, True, "SPLITK", 7, "offset"),
    (4, 128, 128, 320, 320, 1, True, "SPLITK", 16, "unit"),
    (4, 64, 64, 640, 320, 9, True, "SPLITK", 4, "outlier"),         # Cin != Cout
    (4, 64, 64, 640, 320, 1, False, "SPLITK", 16, "unit"),
    (4, 32, 32, 1280, 1280, 9, False, "NONE", 1, "unit"),           # 225 tiles: no split-K
    (4, 32, 32, 1280, 1280, 9, True, "ADD", 1, "unit"),
    (4, 128, 128, 320, 8, 9, False, "SPLITK", 14, "unit"),
    (4, 128, 128, 64, 72, 9, True, "SPLITK", 16, "unit"),
    (1, 9, 7, 64, 72, 9, False, "NONE", 1, "unit"),                 # two K-tiles: too few to slice
    (1, 9, 7, 64, 72, 9, True, "ADD", 1, "offset"),
    (1, 8, 8, 1280, 1280, 1, False, "NONE", 1, "unit"),
    (2, 16, 16, 64, 64, 1, True, "ADD", 1, "outlier"),
]


@pytest.mark.parametrize("case", WGRAD, ids=lambda c: "B{}_{}x{}_{}to{}_t{}_acc{}_{}_ks{}_{}".format(*c))
def test_weight_gradient(ops, case):
    B, H, W, Cin, Cout, taps, acc, store, ks, data = case
    _wgrad(ops, f"B{B} {H}x{W} {Cin}->{Cout} taps {taps} acc {acc} {data}", B, H, W, Cin, Cout, taps, acc, store, ks, data=data, seed=sum(case[:5]) + taps)


def test_weight_gradient_slices_limited_by_the_workspace(ops):
    """7 slices would need 25.8 MB of slabs; a 12 MB workspace holds 3"""
    _wgrad(ops, "B4 128x128 320->320 taps 9, 12 MB workspace", 4, 128, 128, 320, 320, 9, True, "SPLITK", 3, seed=3, workspace_bytes=12 << 20)


# ---- the layout passes and the sequences the models run them in -------------------------------------------------------------------------------------------
@pytest.fixture
def guarded_grids(ops, monkeypatch):
    """every grid buffer the ops wrappers allocate for a layout pass becomes a view into a larger allocation filled with the sentinel; at the end of the test
    the rows on either side must still hold it bit for bit (a write outside the buffer fails)"""
    made = []

    def grid_out(B, H, W, C_, device, conv=False):
        n = B * (H + 2) * (W + 2)
        whole = torch.full((n + 64 + 2 * GUARD, C_), CB.SENTINEL, dtype=BF16, device=device)
        t = whole[GUARD:GUARD + n + 64]
        if conv:
            t[:W + 3].zero_()
            t[n - (W + 3):].zero_()
        else:
            t[n:].zero_()
        made.append(whole)
        return t

    monkeypatch.setattr(ops, "_grid_out", grid_out)
    yield made
    assert made, "no layout pass allocated through ops._grid_out"
    s = torch.tensor(CB.SENTINEL, dtype=BF16, device=dev()).view(torch.int16)
    for whole in made:
        assert bool((CB._bits(whole[:GUARD]) == s).all()) and bool((CB._bits(whole[-GUARD:]) == s).all()), "a layout pass wrote outside its grid buffer"


def _layout_roundtrip(ops, B, H, W, Cn, seed, data="unit"):
    g = _gen(seed)
    img = _randn(g, B, H, W, Cn, data=data)
    grid = _guarded(CB.image_to_grid(img))
    # NCHW <-> grid (channels zero-padded)
    lat = _guarded(_randn(g, B, 4, H, W))
    CB.check_grid_copy("grid_from_nchw", _twice("grid_from_nchw", lambda: ops.grid_from_nchw(lat, 8)), torch.cat([lat.permute(0, 2, 3, 1), torch.zeros(B, H, W, 4, dtype=BF16, device=dev())], 3))
    Cc = Cn - 8 if Cn > 8 else Cn                                         # fewer channels than the grid holds
    assert torch.equal(_twice("grid_to_nchw", lambda: ops.grid_to_nchw(grid, B, Cc, H, W)), CB.nchw(img)[:, :Cc].contiguous())
    # tokens
    assert torch.equal(_twice("grid_to_tokens", lambda: ops.grid_to_tokens(grid, B, H, W)), img.reshape(B * H * W, Cn))
    tok = _guarded(_randn(g, B * H * W, Cn, data=data))
    CB.check_grid_copy("tokens_to_grid", _twice("tokens_to_grid", lambda: ops.tokens_to_grid(tok, B, H, W)), tok.view(B, H, W, Cn))
    want, e = CB.tokens_residual_expect(tok.view(B, H, W, Cn), img)
    _note("summing layout", CB.check_grid_sum(f"tokens_to_grid + residual B{B} {H}x{W} C{Cn}",
                                                  _twice("tokens_to_grid + residual", lambda: ops.tokens_to_grid(tok, B, H, W, residual=grid)), want, e))
    # nearest 2x and its adjoint
    CB.check_grid_copy("upsample2x", _twice("upsample2x", lambda: ops.upsample2x(grid, B, H, W)), CB.upsample_expect(img))
    if H % 2 == 0 and W % 2 == 0:
        want, e = CB.upsample_bwd_expect(img)
        _note("summing layout", CB.check_grid_sum(f"upsample2x_bwd B{B} {H // 2}x{W // 2} C{Cn}",
                                                  _twice("upsample2x_bwd", lambda: ops.upsample2x_bwd(grid, B, H // 2, W // 2)), want, e))
        HIT.add(("layout", "upsample2x_bwd"))
    HIT.update(("layout", k) for k in ("grid_from_nchw", "grid_to_nchw", "grid_to_tokens", "tokens_to_grid", "tokens_to_grid+residual", "upsample2x"))
    return img, grid


def _columns(ops, img, grid, stride, pad, data="unit", seed=0):
    B, H, W, Cn = img.shape
    Kpad = (9 * Cn + 63) // 64 * 64
    col = _twice("im2col3x3", lambda: ops.im2col3x3(grid, B, H, W, stride=stride, pad=pad))
    CB.check_grid_copy(f"im2col3x3 stride {stride} pad {pad}", col, CB.im2col_expect(img, stride, pad, Kpad))
    dcol_img = _randn(_gen(seed), B, H // stride, W // stride, Kpad, data=data)
    want, e = CB.col2im_expect(dcol_img, H, W, Cn, stride, pad)
    dcol = _guarded(CB.image_to_grid(dcol_img))
    dx = _twice("col2im3x3", lambda: ops.col2im3x3(dcol, B, H, W, Cn, stride=stride, pad=pad))
    _note("summing layout", CB.check_grid_sum(f"col2im3x3 B{B} {H}x{W} C{Cn} stride {stride} pad {pad} {data}", dx, want, e))
    HIT.update({("layout", "im2col3x3"), ("layout", "col2im3x3")})
    return col


@pytest.mark.parametrize("B,H,W,Cn,data", [(2, 6, 10, 16, "unit"), (1, 2, 2, 8, "offset"), (3, 16, 12, 64, "outlier"), (1, 5, 3, 24, "unit")])
def test_layout_passes_small_and_odd(ops, guarded_grids, B, H, W, Cn, data):
    img, grid = _layout_roundtrip(ops, B, H, W, Cn, 40 + H, data=data)
    _columns(ops, img, grid, 1, 1, data=data, seed=H)
    if H % 2 == 0 and W % 2 == 0:
        _columns(ops, img, grid, 2, 1, data=data, seed=H + 1)
        _columns(ops, img, grid, 2, 0, data=data, seed=H + 2)


def test_layout_passes_beyond_one_trip_of_the_grid_stride_loops(ops, guarded_grids):
    """B 2 at 1024^2 x 128 channels: 33.7 M sixteen-byte chunks per grid, twice the 65536 x 256 threads of one trip"""
    B, H, W, Cn = 2, 1024, 1024, 128
    assert B * (H + 2) * (W + 2) * Cn // 8 > 65536 * 256
    img, grid = _layout_roundtrip(ops, B, H, W, Cn, 60)
    assert B * (H // 2 + 2) * (W // 2 + 2) * (9 * Cn // 8) > 65536 * 256
    _columns(ops, img, grid, 2, 0, seed=61)                             # the VAE's (0,1,0,1) form
    del img, grid
    dy_img = _randn(_gen(62), B, 2 * H, 2 * W, Cn)                      # upsample2x_bwd writing a grid of that size
    want, e = CB.upsample_bwd_expect(dy_img)
    _note("summing layout", CB.check_grid_sum("upsample2x_bwd B2 1024x1024 C128", ops.upsample2x_bwd(CB.image_to_grid(dy_img), B, H, W), want, e))


@pytest.mark.parametrize("pad,Cn,Cout,B,H,W", [(1, 320, 320, 4, 128, 128), (0, 128, 128, 1, 256, 256)])
def test_stride_2_downsampling_as_the_models_sequence_it(ops, guarded_grids, pad, Cn, Cout, B, H, W):
    """im2col3x3 (stride 2) -> taps-1 convolution; backward GEMM -> col2im3x3.  pad 1: the UNet's Downsample2D; pad 0: the VAE's (0,1,0,1) form"""
    g = _gen(70 + pad)
    img = _randn(g, B, H, W, Cn)
    col = _columns(ops, img, _guarded(CB.image_to_grid(img)), 2, pad, seed=71)
    Ho, Wo, K = H // 2, W // 2, 9 * Cn
    w = _randn(g, Cout, K, scale=1 / math.sqrt(K))
    bias = _randn(g, Cout, scale=0.5)
    kernel = ops.conv_plan(B, Ho, Wo, K, Cout, 1)["kernel"]
    HIT.add(("fwd", kernel, "NONE", 1))
    whole, out = CB.conv_out_buffer(B, Ho, Wo, Cout, dev(), guard=GUARD)
    ops.conv(_guarded(col), w, B, Ho, Wo, bias=bias, taps=1, out=out)
    CB.check_conv_exact("stride-2 conv", out, B, Ho, Wo, whole=whole, guard=GUARD)
    want, e = CB.conv_ref(CB.im2col_expect(img, 2, pad, K), w, 1, bias)                      # = the stride-2 convolution of the padded image
    _note("forward", CB.check_conv(f"{kernel} stride-2 conv pad {pad} B{B} {H}x{W} {Cn}->{Cout}", out, want, e, B, Ho, Wo))
    # backward: dcol = dy w (plain GEMM, bounded in test_gemm_bounds_gpu.py), then the adjoint gather from the kernel's own dcol
    dy_img = _randn(g, B, Ho, Wo, Cout)
    dyg = CB.image_to_grid(dy_img)
    n = CB.grid_positions(B, Ho, Wo)
    dcol = torch.zeros(n + 64, K, dtype=BF16, device=dev())
    ops.gemm(dyg[:n], w.t().contiguous(), out=dcol[:n])
    dx = ops.col2im3x3(dcol, B, H, W, Cn, stride=2, pad=pad)
    want, e = CB.col2im_expect(CB.grid_to_image(dcol, B, Ho, Wo), H, W, Cn, 2, pad)
    _note("summing layout", CB.check_grid_sum(f"col2im3x3 of the backward GEMM, pad {pad}", dx, want, e))


def test_upsample_then_convolution(ops, guarded_grids):
    B, H, W, Cn = 4, 32, 32, 640
    g = _gen(80)
    img = _randn(g, B, H, W, Cn)
    up = ops.upsample2x(CB.image_to_grid(img), B, H, W)
    CB.check_grid_copy("upsample2x", up, CB.upsample_expect(img))
    w = _randn(g, Cn, 9 * Cn, scale=1 / math.sqrt(9 * Cn))
    bias = _randn(g, Cn, scale=0.5)
    assert ops.conv_plan(B, 2 * H, 2 * W, Cn, Cn)["kernel"] == "pq_conv"
    whole, out = CB.conv_out_buffer(B, 2 * H, 2 * W, Cn, dev(), guard=GUARD)
    ops.conv(_guarded(up), w, B, 2 * H, 2 * W, bias=bias, out=out)
    CB.check_conv_exact("upsample conv", out, B, 2 * H, 2 * W, whole=whole, guard=GUARD)
    want, e = CB.conv_ref(CB.upsample_expect(img), w, 9, bias)
    _note("forward", CB.check_conv("pq_conv Upsample2D 32^2 -> 64^2, 640", out, want, e, B, 2 * H, 2 * W))


def test_pad_0_is_the_stride_2_form_for_both_column_passes(ops):
    """documented contracts: st355_col2im3x3 takes pad 0 only in the stride-2 (0,1,0,1) form, like st355_im2col3x3"""
    from simpletuner_amd import lib

    img = _randn(_gen(1), 1, 4, 4, 8)
    with pytest.raises(lib.St355Error):
        ops.im2col3x3(CB.image_to_grid(img), 1, 4, 4, stride=1, pad=0)
    with pytest.raises(lib.St355Error):
        ops.col2im3x3(torch.zeros(CB.grid_rows(1, 4, 4), 128, dtype=BF16, device=dev()), 1, 4, 4, 8, stride=1, pad=0)


def test_the_checks_bite_on_a_kernel_output(ops):
    """one real output, then three single-element corruptions of it: each must fail its check (the checks above are not vacuous on real outputs)"""
    B, H, W, Cin, Cout = 2, 32, 32, 64, 320
    g = _gen(99)
    x_img = _randn(g, B, H, W, Cin)
    w = _randn(g, Cout, 9 * Cin, scale=1 / math.sqrt(9 * Cin))
    whole, out = CB.conv_out_buffer(B, H, W, Cout, dev(), guard=GUARD)
    ops.conv(CB.image_to_grid(x_img), w, B, H, W, out=out)
    want, e = CB.conv_ref(x_img, w, 9)
    CB.check_conv_exact("clean", out, B, H, W, whole=whole, guard=GUARD)
    assert CB.check_conv("clean", out, want, e, B, H, W).ok
    rows = CB.interior_rows(B, H, W, dev())
    bad = out.clone()
    bad[rows[777], 300] += 4 * GB.ulp_bf16(want[777, 300].abs()).to(BF16)                   # four ulps on one interior element
    rep = CB.check_conv("four ulps on one element", bad, want, e, B, H, W)
    assert not rep.ok_elem and rep.worst_at == (int(rows[777]) - (W + 3), 300)
    bad = out.clone()
    bad[2 * (W + 2), 5] = 2.0 ** -10                                                        # a border position inside the computed range
    with pytest.raises(AssertionError):
        CB.check_conv_exact("border", bad, B, H, W)
    bad = out.clone()
    bad[1, 0] = 0.0                                                                         # a row the kernel must keep
    with pytest.raises(AssertionError):
        CB.check_conv_exact("kept row", bad, B, H, W)


def test_every_instance_was_reached():
    for fam, (w, r) in sorted(WORST.items()):
        print(f"[conv bounds] {fam}: worst err/tol {w:.3f}, worst 64x64 block RMS {r:.3f}")
    assert HIT == ALL, f"not reached: {sorted(ALL - HIT, key=str)}; unknown: {sorted(HIT - ALL, key=str)}"

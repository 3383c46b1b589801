"""The convolution bound checker (tests/conv_bounds.py) bites: computed in torch on the CPU (no GPU, no library), an honest emulation of the kernels (fp32
accumulation, one RNE) passes every bound, and each modelled defect fails while the bar it would have slipped through (tests/test_unet_kernels_gpu.py: global rel-L2
< 6e-3 forward, < 8e-3 gradients) still passes.  A defect that cannot pass the old bar at a CPU-affordable shape prints the number of outputs from which it would
(a defect confined to a fixed set of outputs has rel-L2 ~ 1 / sqrt(outputs): computed from the measured rel-L2, not guessed) and must still fail the new check.

The layout helpers of conv_bounds.py are pinned first against F.conv2d in fp64."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import conv_bounds as CB
from tests import gemm_bounds as GB

BF16 = torch.bfloat16
OLD_FWD, OLD_GRAD = 6e-3, 8e-3


def _rand(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF16)


def _oihw(w, taps):
    k = 3 if taps == 9 else 1
    return w.view(w.shape[0], k, k, -1).permute(0, 3, 1, 2)


def _verdict(name, rep, rel, bar, outputs=None):
    extra = ""
    if rel >= bar and outputs:
        extra = f"; passes the old bar from {outputs * (rel / bar) ** 2:.3g} outputs ({(rel / bar) ** 2:.1f} x this shape)"
    print(f"[mutation] {name}: new checker {'PASS' if rep.ok else 'FAIL'} (worst err/tol {rep.worst:.2f}, block RMS {rep.block_rms:.3f}), old rel-L2 {rel:.2e} "
          f"(bar {bar:g}: {'passes' if rel < bar else 'FAILS'}){extra}")


# ---- the layout helper and the reference, pinned --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,taps", [(2, 5, 7, 8, 16, 9), (3, 1, 1, 8, 8, 9), (1, 6, 1, 16, 8, 1), (2, 4, 4, 8, 8, 1)])
def test_reference_and_layout_against_conv2d_fp64(B, H, W, Cin, Cout, taps):
    g = torch.Generator().manual_seed(1)
    x = _rand(g, B, H, W, Cin)
    w = _rand(g, Cout, taps * Cin)
    bias, temb, res = _rand(g, Cout), _rand(g, B, Cout + 8), _rand(g, B, H, W, Cout)
    want, e = CB.conv_ref(x, w, taps, bias, temb, res)
    ref = F.conv2d(CB.nchw(x).double(), _oihw(w, taps).double(), bias.double(), padding=1 if taps == 9 else 0) + temb.double()[:, :Cout, None, None] + CB.nchw(res).double()
    assert torch.allclose(want.view(B, H, W, Cout), ref.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
    # the grid layout: row (b (H+2) + y + 1) (W+2) + x + 1, everything else zero, 64 tail rows; sel picks the same rows
    gx = CB.image_to_grid(x)
    assert gx.shape[0] == B * (H + 2) * (W + 2) + 64
    for (b, y, xx) in ((0, 0, 0), (B - 1, H - 1, W - 1), (B // 2, H // 2, W // 2)):
        assert torch.equal(gx[(b * (H + 2) + y + 1) * (W + 2) + xx + 1], x[b, y, xx])
    assert int((gx != 0).any(1).sum()) <= B * H * W and torch.equal(CB.grid_to_image(gx, B, H, W), x)
    assert len(CB.border_rows(B, H, W)) == B * ((H + 2) * (W + 2) - H * W)
    sel = torch.arange(0, B * H * W, 3)
    ws, es = CB.conv_ref(x, w, taps, bias, temb, res, sel=sel)
    assert torch.equal(ws, want[sel]) and torch.equal(es, e[sel])
    # the weight-gradient reference and the input-gradient weight against autograd in fp64
    dy = _rand(g, B, H, W, Cout)
    xd = CB.nchw(x).double().requires_grad_(True)
    wd = _oihw(w, taps).double().requires_grad_(True)
    (F.conv2d(xd, wd, padding=1 if taps == 9 else 0) * CB.nchw(dy).double()).sum().backward()
    dw, _ = CB.wgrad_ref(x, dy, taps, 64, 1)
    assert torch.allclose(dw, CB.ohwi(wd.grad), rtol=1e-12, atol=1e-12)
    dx, _ = CB.conv_ref(dy, CB.input_grad_weight(w, taps), taps)
    assert torch.allclose(dx.view(B, H, W, Cin), xd.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dx2, _ = CB.dgrad_ref(dy, w, taps)
    assert torch.allclose(dx2.view(B, H, W, Cin), xd.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_layout_expectations_against_unfold_and_autograd():
    g = torch.Generator().manual_seed(2)
    B, H, W, C = 2, 6, 8, 8
    x = _rand(g, B, H, W, C)
    for stride, pad in ((1, 1), (2, 1), (2, 0)):
        col = CB.im2col_expect(x, stride, pad, 128)
        xin = CB.nchw(x).double() if pad else F.pad(CB.nchw(x).double(), (0, 1, 0, 1))
        u = F.unfold(xin, 3, padding=pad, stride=stride)                                     # [B, C 9, L], channel-major
        u = u.view(B, C, 9, H // stride, W // stride).permute(0, 3, 4, 2, 1).reshape(B, H // stride, W // stride, 9 * C)
        assert torch.equal(col[..., :72].double(), u) and not col[..., 72:].any()
        d = _rand(g, B, H // stride, W // stride, 128)
        want, e = CB.col2im_expect(d, H, W, C, stride, pad)
        xx = x.double().requires_grad_(True)
        (CB.im2col_expect(xx, stride, pad, 128) * d.double()).sum().backward()
        assert torch.allclose(want, xx.grad, atol=1e-12) and bool((e >= 0).all())
    up = CB.upsample_expect(x)
    assert torch.equal(CB.nchw(up).float(), F.interpolate(CB.nchw(x).float(), scale_factor=2, mode="nearest"))
    want, _ = CB.upsample_bwd_expect(up)
    assert torch.equal(want, 4 * x.double())


# ---- forward: the honest emulation and the defects --------------------------------------------------------------------------------------------------------
class _Fwd:
    """one forward case: operands, the fp64 reference, the honest fp32 pre-rounding value v [B, H, W, Cout]"""

    def __init__(self, B, H, W, Cin, Cout, seed, close_temb=False):
        g = torch.Generator().manual_seed(seed)
        self.dims = (B, H, W)
        self.x = _rand(g, B, H, W, Cin)
        self.w = _rand(g, Cout, 9 * Cin, scale=1 / math.sqrt(9 * Cin))
        self.bias = _rand(g, Cout, scale=0.5)
        self.temb = (torch.randn(1, Cout, generator=g) + (0.02 if close_temb else 1.0) * torch.randn(B, Cout, generator=g)).to(BF16)
        self.res = _rand(g, B, H, W, Cout)
        self.want, self.e = CB.conv_ref(self.x, self.w, 9, self.bias, self.temb, self.res)
        acc = F.conv2d(CB.nchw(self.x).float(), _oihw(self.w, 9).float(), padding=1).permute(0, 2, 3, 1)
        self.v = acc + self.bias.float() + self.temb.float()[:, None, None, :] + self.res.float()
        self.xp = F.pad(self.x.float(), (0, 0, 1, 1, 1, 1))                                   # [B, H+2, W+2, Cin]
        self.rows = CB.interior_rows(B, H, W)

    def tap(self, t, ci=slice(None)):
        """fp32 contribution of tap t (channels ci) at every position: [B, H, W, Cout]"""
        B, H, W = self.dims
        ky, kx = divmod(t, 3)
        wt = self.w.float().view(self.w.shape[0], 9, -1)[:, t, ci]
        return self.xp[:, ky:ky + H, kx:kx + W, ci] @ wt.t()

    def grid(self, v):
        """what the kernel leaves in an output buffer prepared by conv_out_buffer"""
        B, H, W = self.dims
        _, out = CB.conv_out_buffer(B, H, W, v.shape[3], "cpu")
        p0, n = W + 3, CB.grid_positions(B, H, W)
        out[p0:n - p0] = 0
        out[self.rows] = GB.to_bf16_rne(v).reshape(-1, v.shape[3])
        return out

    def judge(self, name, out, expect_exact=True):
        B, H, W = self.dims
        exact = True
        try:
            CB.check_conv_exact(name, out, B, H, W)
        except AssertionError as ex:
            exact = False
            print(f"[mutation] {name}: exact contract FAIL ({ex})")
        rep = CB.check_conv(name, out, self.want, self.e, B, H, W)
        rel = GB.rel_l2(CB.grid_to_image(out, B, H, W).reshape(self.want.shape).float().nan_to_num(0.0), self.want)
        return rep, rel, exact


@pytest.fixture(scope="module")
def big():
    return _Fwd(3, 153, 139, 640, 64, 11, close_temb=True)        # 63801 positions; 65281 GEMM rows = 255 tiles of 256 + ONE row


@pytest.fixture(scope="module")
def small():
    return _Fwd(2, 32, 32, 320, 320, 12)


def test_forward_honest_emulation_passes(big, small):
    for s, name in ((big, "big"), (small, "small 320 -> 320")):
        rep, rel, exact = s.judge(f"honest {name}", s.grid(s.v))
        _verdict(f"honest {name}", rep, rel, OLD_FWD)
        GB.assert_bound(rep)
        assert exact and rel < OLD_FWD


def _fails_new_passes_old(name, s, out, bar=OLD_FWD):
    rep, rel, exact = s.judge(name, out)
    _verdict(name, rep, rel, bar, outputs=s.want.numel())
    assert not rep.ok or not exact
    return rep, rel, exact


def test_tap_dropped_at_one_position_per_image(big):
    v = big.v.clone()
    t = big.tap(8)
    for b in range(3):
        v[b, 70 + b, 5] -= t[b, 70 + b, 5]
    rep, rel, _ = _fails_new_passes_old("tap (2,2) dropped at one position per image", big, big.grid(v))
    assert not rep.ok_elem and rel < OLD_FWD


def test_row_wrap_around_on_one_row(big):
    """tap (1,0) of column 0 reads the last column of the previous row instead of the zero border"""
    B, H, W = big.dims
    v = big.v.clone()
    w10 = big.w.float().view(64, 9, -1)[:, 3]
    v[1, 40, 0] += w10 @ big.x.float()[1, 39, W - 1]
    rep, rel, _ = _fails_new_passes_old("row wrap-around, one row", big, big.grid(v))
    assert not rep.ok_elem and rel < OLD_FWD


def test_img_add_of_the_neighbouring_image_on_a_straddling_tile():
    """a 256-row tile holds interior rows of two images only when 2 W + 7 < 256 (the rows between them are border), and then only where the tile
    boundaries fall that way: a 56 x 56 grid, per-sample embeddings of nearby timesteps (close, not equal)"""
    s = _Fwd(4, 56, 56, 64, 64, 13, close_temb=True)
    B, H, W = s.dims
    per, p0 = (H + 2) * (W + 2), W + 3
    m = s.rows - p0
    img = s.rows // per
    tile_img = ((m // 256) * 256 + p0) // per                      # the image of the tile's first row
    hit = img != tile_img
    assert 0 < int(hit.sum()) < 256 * (B - 1)
    v = s.v.clone().view(-1, 64)
    v[hit] += s.temb.float()[tile_img[hit]] - s.temb.float()[img[hit]]
    rep, rel, _ = _fails_new_passes_old("img_add of the tile's first image", s, s.grid(v.view(s.v.shape)))
    assert not rep.ok_elem and rel < OLD_FWD


def test_last_ragged_tile_shifted_by_one_position(big):
    B, H, W = big.dims
    out = big.grid(big.v)
    last = CB.grid_positions(B, H, W) - (W + 3) - 1                 # the single row of the last 256-row tile = the last interior position
    assert (last - (W + 3)) % 256 == 0 and int(big.rows[-1]) == last
    out[last] = out[last - 1]
    rep, rel, _ = _fails_new_passes_old("last ragged tile one position early", big, out)
    assert not rep.ok_elem and rep.worst_at[0] == last - (W + 3) and rel < OLD_FWD


def test_one_k_tile_of_one_tap_skipped_for_one_row_tile(big):
    B, H, W = big.dims
    m = big.rows - (W + 3)
    hit = m // 256 == 100
    v = big.v.clone().view(-1, 64)
    v[hit] -= big.tap(4, slice(64, 128)).reshape(-1, 64)[hit]
    rep, rel, _ = _fails_new_passes_old("one K-tile of tap (1,1) skipped in row tile 100", big, big.grid(v.view(big.v.shape)))
    assert not rep.ok and rep.block_tile[0] == 100 or not rep.ok_elem
    assert rel < OLD_FWD


def test_nonzero_border_position(big):
    """the old rel-L2 is taken on the interior and cannot see it at all; the old exact-border assertion ran at three small shapes only"""
    B, H, W = big.dims
    out = big.grid(big.v)
    out[(1 * (H + 2) + 60) * (W + 2) + W + 1, 3] = 2.0 ** -9
    rep, rel, exact = _fails_new_passes_old("non-zero border position", big, out)
    assert not exact and rel < OLD_FWD


def test_round_toward_zero(small):
    rtz = (small.v.view(torch.int32) & ~0xFFFF).view(torch.float32)
    rep, rel, _ = _fails_new_passes_old("round toward zero", small, small.grid(rtz))
    assert rel < OLD_FWD


def test_four_positions_scaled(small):
    v = small.v.clone()
    for (b, y, x) in ((0, 3, 3), (0, 20, 31), (1, 0, 0), (1, 31, 16)):
        v[b, y, x] *= 1 + 2.0 ** -6
    rep, rel, _ = _fails_new_passes_old("four positions x (1 + 2^-6)", small, small.grid(v))
    assert rel < OLD_FWD


@pytest.mark.parametrize("kind", ["unwritten", "stale"])
def test_last_live_columns_of_the_dead_column_tile(small, kind):
    """Cout 320: the second column tile has 64 live columns; one 256-row tile leaves them unwritten (the NaN pre-fill) or stale (another launch's values).  Every
    such output is wrong, so the old bar sees it at this size; the printed line gives the size from which it would not."""
    B, H, W = small.dims
    m = small.rows - (W + 3)
    hit = m // 256 == 2
    out = small.grid(small.v)
    blk = out[small.rows[hit], 256:]
    out[small.rows[hit], 256:] = torch.full_like(blk, float("nan")) if kind == "unwritten" else blk.flip(0)
    rep, rel, _ = _fails_new_passes_old(f"last 64 live columns {kind} in one row tile", small, out)
    assert not rep.ok_elem and rep.worst_at[1] >= 256


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------------------------
class _Wgrad:
    """the kernel's form emulated in grid space: K-slices of `per` 64-row K-tiles from the first GEMM row, fp32 partial sums, fixed-order fp32 adds, one RNE"""

    def __init__(self, B, H, W, Cin, Cout, ks, seed, shift=0.0, old=False):
        g = torch.Generator().manual_seed(seed)
        self.dims, self.ks = (B, H, W), ks
        self.x = _rand(g, B, H, W, Cin, shift=shift)
        self.dy = _rand(g, B, H, W, Cout)
        self.old = _rand(g, Cout, 9 * Cin, scale=8.0) if old else None
        p0 = W + 3
        self.Mc = (CB.grid_positions(B, H, W) - 2 * p0 + 63) // 64 * 64
        self.want, self.e = CB.wgrad_ref(self.x, self.dy, 9, self.Mc, ks, self.old)
        xg, dyg = CB.image_to_grid(self.x).float(), CB.image_to_grid(self.dy).float()
        nt = self.Mc // 64
        per = (nt + ks - 1) // ks
        self.parts = []
        for s in range(ks):
            a, b = s * per * 64, min(nt, (s + 1) * per) * 64
            self.parts.append(torch.cat([dyg[p0 + a:p0 + b].t() @ xg[a + sh:b + sh] for sh in self.shifts()], 1))

    def shifts(self):
        Wp = self.dims[2] + 2
        return [ky * Wp + kx for ky in range(3) for kx in range(3)]

    def total(self, parts=None, old_times=1):
        s = None
        for p in (parts or self.parts):
            s = p.clone() if s is None else s + p
        if self.old is not None:
            s = s + old_times * self.old.float()
        return s

    def judge(self, name, v):
        out = GB.to_bf16_rne(v)
        rep = GB.check(name, out, self.want, self.e)
        return rep, GB.rel_l2(out, self.want)


def test_wgrad_honest_emulation_passes_up_to_the_largest_contraction():
    for (B, H, W, Cin, Cout, ks, shift, old) in ((2, 32, 32, 320, 320, 4, 0.0, False), (2, 32, 32, 64, 64, 1, 16.0, True), (4, 128, 128, 128, 64, 7, 0.0, True)):
        s = _Wgrad(B, H, W, Cin, Cout, ks, 21, shift=shift, old=old)
        rep, rel = s.judge(f"honest wgrad Mc {s.Mc} ks {ks}", s.total())
        _verdict(f"honest wgrad B{B} {H}x{W} {Cin}->{Cout} Mc {s.Mc} ks {ks}", rep, rel, OLD_GRAD)
        GB.assert_bound(rep)
        assert rel < OLD_GRAD


@pytest.fixture(scope="module")
def wg():
    return _Wgrad(2, 32, 32, 320, 320, 4, 22, old=True)


def test_wgrad_tap_block_with_the_wrong_shift():
    """the column block of tap (1,2) contracted with the shift of tap (1,1).  With white-noise activations the whole block is wrong at any size (rel-L2 sqrt(2) / 3):
    the old bar sees it.  On activations with a large common offset (mean / std m = 128) neighbouring positions nearly agree, and what is left is the image edge
    (one column per row reads the zero border instead of the offset, and one the other way round): rel-L2^2 ~ (2 / W + 2 / m^2) / 9, which passes the old bar only
    from the width printed below.  The new check fails it at every size, and names the block column."""
    s = _Wgrad(2, 32, 32, 64, 64, 1, 23, shift=128.0)
    v = s.total()
    xg, dyg = CB.image_to_grid(s.x).float(), CB.image_to_grid(s.dy).float()
    p0, sh = s.dims[2] + 3, s.shifts()[4]
    v[:, 5 * 64:6 * 64] = dyg[p0:p0 + s.Mc].t() @ xg[sh:sh + s.Mc]
    rep, rel = s.judge("tap (1,2) block with the shift of (1,1)", v)
    _verdict("wgrad tap block with the wrong shift (offset data)", rep, rel, OLD_GRAD)
    floor2 = 2 / 128 ** 2 / 9
    print(f"[mutation]   edge term (rel-L2^2 - {floor2:.2e}) W = {(rel ** 2 - floor2) * 32:.3g}: passes the old bar from W = {(rel ** 2 - floor2) * 32 / (OLD_GRAD ** 2 - floor2):.0f}")
    assert not rep.ok_block and rep.block_at[1] == 5 and not rep.ok_elem


def test_wgrad_k_slice_dropped_from_one_tile(wg):
    v = wg.total()
    bad = wg.total([p for i, p in enumerate(wg.parts) if i != 2])
    v[256:, 512:768] = bad[256:, 512:768]
    rep, rel = wg.judge("K-slice 2 dropped from tile (1, 2)", v)
    _verdict("wgrad K-slice dropped from one tile", rep, rel, OLD_GRAD, outputs=wg.want.numel())
    assert not rep.ok and rep.block_tile == (1, 2)


@pytest.mark.parametrize("times", [0, 2])
def test_wgrad_accumulate_wrong_on_one_tile(wg, times):
    v = wg.total()
    v[:256, 256:512] = wg.total(old_times=times)[:256, 256:512]
    rep, rel = wg.judge(f"old dw added {times} times on tile (0, 1)", v)
    _verdict(f"wgrad accumulate adds the old value {times} times on one tile", rep, rel, OLD_GRAD, outputs=wg.want.numel())
    assert not rep.ok_elem and rep.block_tile == (0, 1)


# ---- summing layout passes --------------------------------------------------------------------------------------------------------------------------------
def test_summing_layout_passes_honest_and_one_term_lost():
    g = torch.Generator().manual_seed(31)
    B, H, W, C = 2, 64, 64, 64
    d = _rand(g, B, H // 2, W // 2, 9 * C)
    want, e = CB.col2im_expect(d, H, W, C, 2, 1)
    honest = CB.image_to_grid(GB.to_bf16_rne(want))
    GB.assert_bound(CB.check_grid_sum("col2im honest", honest, want, e))
    dy = _rand(g, B, 2 * H, 2 * W, C)
    want_u, e_u = CB.upsample_bwd_expect(dy)
    GB.assert_bound(CB.check_grid_sum("upsample2x_bwd honest", CB.image_to_grid(GB.to_bf16_rne(want_u)), want_u, e_u))
    lost = want_u.clone()
    lost[1, 63, 63] -= dy[1, 127, 127].double()                                             # the last of the four terms at the last position
    bad = CB.image_to_grid(GB.to_bf16_rne(lost))
    rep = CB.check_grid_sum("upsample2x_bwd, one term lost at the last position", bad, want_u, e_u)
    rel = GB.rel_l2(CB.grid_to_image(bad, B, H, W), want_u)
    _verdict("upsample2x_bwd one term lost at one position", rep, rel, OLD_FWD)
    assert not rep.ok_elem and rel < OLD_FWD
    honest[5, 0] = 2.0 ** -8                                                                 # a border position
    with pytest.raises(AssertionError):
        CB.check_grid_sum("col2im, non-zero border", honest, want, e)

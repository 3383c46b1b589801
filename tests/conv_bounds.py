"""Element-wise error bounds for the convolution path (gemm.hip: st355_conv_bf16 / st355_conv_wgrad_bf16; conv.hip: the layout passes) against fp64 references built
in IMAGE space.  Built on tests/gemm_bounds.py (check, assert_bound, ulp_bf16, the constants).

The reference never indexes a grid buffer the way the kernels do.  Images are channels-last tensors [B, H, W, C] (a permuted view of NCHW); the convolution
reference zero-pads them with F.pad, takes the nine shifted slices and contracts each in fp64.  Only then is the result compared with the kernel's grid rows through
interior_rows(): position (b, y, x) of the image lives at grid row b (H+2)(W+2) + (y+1)(W+2) + (x+1) — written here from the documented layout of st355.h, and pinned
against F.conv2d in fp64 by tests/test_conv_bounds_checker_cpu.py.

Forward / input gradient (one RNE rounding of an fp32 expression, k_gemm_pq / k_gemm_s2 epilogue: v = acc + bias + img_add[image] (+ residual), f2bf(v)):

    want = acc + bias + img_add[image] + residual
    e    = 2^-24 (taps Cin + 8) (|x| * |w| + |bias| + |img_add| + |residual|) + 2^-20 (1 + |want|)
    tol  = 1/2 ulp_bf16(|want| + e) + e

the GEMM family's form with K = taps Cin.  The block statistic (RMS of min(err / ulp, 4) over 64 x 64 blocks, limit 0.5) is taken over the INTERIOR positions in
grid order, so the zero border rows cannot dilute a block.  Border positions inside the computed range [W+3, rows - W - 3) must be exactly zero; the first / last W+3
positions and the 64 tail rows must keep the caller's bits; every computed row must have been written (the callers pre-fill with NaN / a sentinel).

Weight gradient: want[co, tap, ci] = sum_pos dy[pos, co] x[pos + shift(tap), ci] (+ the old dw when accumulating), from the image tensors.
    e = 2^-24 (Mc + 8 + ks) mag,   mag = sum |dy| |x| (+ |old dw|)
Mc is the kernel's rounded contraction length and ks its K-slice count (both from st355_conv_plan).  ONE rounding in both forms: the direct store rounds
acc (+ old dw) once in the k_gemm_pq epilogue (EPI_NONE / EPI_ADD: f2bf(acc + aux_in)); under split-K the slices write fp32 slabs unrounded and k_splitk_reduce adds
them in slice order in fp32, adds the old bf16 value and rounds once (gemm.hip: o = f2bf(s + bf2f(c0))).  The ks slab adds are the "+ ks".  The worst-case bound is
loose at Mc = 17 k ... 68 k; the 64 x 64 block statistic over dw viewed as [Cout, taps Cin] localises: a lost tap is Cin whole columns, a lost K-slice moves every
block of its tile.  The honest emulation (fp32 partial sums per slice, fixed-order fp32 adds, one RNE) stays under the 0.5 limit at the largest Mc a CPU test affords
(test_conv_bounds_checker_cpu.py prints it); the typical fp32 summation error is a random walk of ~2^-24 sqrt(Mc) |terms|, far below one bf16 ulp of the sum.

Layout passes: pure copies are compared with torch.equal against expectations indexed here in image space (zero border and zero pad columns included).  The three
that add (col2im3x3: up to nine terms, upsample2x_bwd: four, tokens_to_grid with a residual: two) sum in fp32 and round once:
tol = 1/2 ulp + 2^-24 n sum|terms| (passed to check() as e).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import gemm_bounds as GB

F64 = torch.float64
BF16 = torch.bfloat16
TAIL = 64


# ---- the documented layout, by index arithmetic -------------------------------------------------------------------------------------------------------
def grid_positions(B, H, W):
    return B * (H + 2) * (W + 2)


def grid_rows(B, H, W):
    return grid_positions(B, H, W) + TAIL


def interior_rows(B, H, W, device=None):
    """grid rows of the interior positions, in (b, y, x) order (= increasing grid row)"""
    b = torch.arange(B, device=device).view(B, 1, 1)
    y = torch.arange(H, device=device).view(1, H, 1)
    x = torch.arange(W, device=device).view(1, 1, W)
    return (b * ((H + 2) * (W + 2)) + (y + 1) * (W + 2) + (x + 1)).reshape(-1)


def border_rows(B, H, W, device=None):
    """grid rows (tail excluded) that are border positions"""
    m = torch.ones(grid_positions(B, H, W), dtype=torch.bool, device=device)
    m[interior_rows(B, H, W, device)] = False
    return m.nonzero().view(-1)


def image_to_grid(img, fill=0.0):
    """[B, H, W, C] -> grid buffer [rows, C]; border and tail = fill"""
    B, H, W, C = img.shape
    g = torch.full((grid_rows(B, H, W), C), fill, dtype=img.dtype, device=img.device)
    g[interior_rows(B, H, W, img.device)] = img.reshape(-1, C)
    return g


def grid_to_image(g, B, H, W):
    return g[interior_rows(B, H, W, g.device)].view(B, H, W, g.shape[1])


def nchw(img):
    return img.permute(0, 3, 1, 2)


def ohwi(w_oihw):
    """torch Conv2d weight -> the [Cout, taps Cin] layout of st355.h"""
    return w_oihw.permute(0, 2, 3, 1).reshape(w_oihw.shape[0], -1).contiguous()


def input_grad_weight(w, taps):
    """the weight of the input-gradient convolution as the UNet builds it (unet.py: flipped taps, transposed): [Cout, taps Cin] -> [Cin, taps Cout]"""
    Cout = w.shape[0]
    Cin = w.shape[1] // taps
    return w.view(Cout, taps, Cin).flip(1).permute(2, 1, 0).reshape(Cin, taps * Cout).contiguous()


# ---- forward / input gradient ---------------------------------------------------------------------------------------------------------------------------
def _taps(taps):
    return [(ky, kx) for ky in range(3) for kx in range(3)] if taps == 9 else [(1, 1)]


def conv_ref(x_img, w, taps, bias=None, img_add=None, residual_img=None, sel=None):
    """fp64 reference of st355_conv_bf16 at the interior positions, in (b, y, x) order: (want, e) [B H W, Cout] (or [len(sel), Cout] for sel, a sorted index tensor
    into that order).  x_img [B, H, W, Cin], w [Cout, taps Cin], img_add [B, >= Cout], residual_img [B, H, W, Cout]."""
    B, H, W, Cin = x_img.shape
    Cout = w.shape[0]
    wt = w.to(F64).view(Cout, len(_taps(taps)), Cin)
    outs, mags = [], []
    for b in range(B):
        xp = F.pad(nchw(x_img[b:b + 1]).to(F64), (1, 1, 1, 1))[0]                    # [Cin, H+2, W+2], zero-padded
        idx = None
        if sel is not None:
            idx = sel[(sel >= b * H * W) & (sel < (b + 1) * H * W)] - b * H * W
            if idx.numel() == 0:
                continue
        acc = mag = None
        for t, (ky, kx) in enumerate(_taps(taps)):
            sl = xp[:, ky:ky + H, kx:kx + W].reshape(Cin, H * W).t()
            if idx is not None:
                sl = sl[idx]
            a = sl @ wt[:, t].t()
            m = sl.abs() @ wt[:, t].abs().t()
            acc = a if acc is None else acc + a
            mag = m if mag is None else mag + m
        for extra in (bias, img_add[b, :Cout] if img_add is not None else None):
            if extra is not None:
                acc = acc + extra.to(F64)
                mag = mag + extra.to(F64).abs()
        if residual_img is not None:
            r = residual_img[b].reshape(H * W, Cout).to(F64)
            if idx is not None:
                r = r[idx]
            acc = acc + r
            mag = mag + r.abs()
        outs.append(acc)
        mags.append(mag)
    want, mag = torch.cat(outs), torch.cat(mags)
    return want, GB.U24 * (taps * Cin + 8) * mag + GB.U20 * (1 + want.abs())


SENTINEL = -1.4140625          # exact in bf16


def conv_out_buffer(B, H, W, Cout, device, guard=0):
    """an output grid buffer for st355_conv_bf16, as a view into a larger allocation: the rows the kernel must write hold NaN, the rows it must keep (first / last
    W+3 positions, 64 tail rows) and `guard` rows on either side hold SENTINEL.  Returns (whole allocation, the grid-buffer view)."""
    rows, n, p0 = grid_rows(B, H, W), grid_positions(B, H, W), W + 3
    whole = torch.full((rows + 2 * guard, Cout), SENTINEL, dtype=BF16, device=device)
    view = whole[guard:guard + rows]
    view[p0:n - p0] = float("nan")
    return whole, view


def _bits(t):
    return t.contiguous().view(torch.int16)


def check_conv_exact(name, out, B, H, W, whole=None, guard=0, computed=None):
    """the exact part of the contract: kept rows and guard rows still hold SENTINEL bit for bit, border positions inside the computed range are zero.
    computed: optional (lo, hi) grid-row window to restrict the border check to (sampled checks of very large grids pass several windows one by one)"""
    n, p0 = grid_positions(B, H, W), W + 3
    s = torch.tensor(SENTINEL, dtype=BF16, device=out.device).view(torch.int16)
    kept = torch.cat([_bits(out[:p0]), _bits(out[n - p0:])])
    assert bool((kept == s).all()), f"{name}: a row outside the computed range [W+3, rows - W - 3) was written"
    if whole is not None and guard:
        assert bool((_bits(whole[:guard]) == s).all()) and bool((_bits(whole[-guard:]) == s).all()), f"{name}: a write outside the grid buffer"
    assert not bool(torch.isnan(out[p0:n - p0]).any()), f"{name}: a row of the computed range was not written (NaN pre-fill left)"
    br = border_rows(B, H, W, out.device)
    br = br[(br >= p0) & (br < n - p0)]
    if computed is not None:
        br = br[(br >= computed[0]) & (br < computed[1])]
    bad = (_bits(out[br]) & 0x7FFF) != 0
    assert not bool(bad.any()), f"{name}: border position (grid row {int(br[bad.any(1).nonzero()[0]])}) is not zero"


def check_conv(name, out, want, e, B, H, W, sel=None, tile=(256, 256)):
    """bound the interior positions (all, or the sorted subset sel of the (b, y, x) order) in grid order; the report names grid rows relative to the first GEMM row"""
    rows = interior_rows(B, H, W, out.device)
    if sel is not None:
        rows = rows[sel]
    return GB.check(name, out[rows], want, e, tile=tile, rows=rows - (W + 3))


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------------
def wgrad_ref(x_img, dy_img, taps, Mc, ks, old=None):
    """(want, e) [Cout, taps Cin] fp64: want[co, tap Cin + ci] = sum_{b,y,x} dy[b,y,x,co] xpad[b, y+ky, x+kx, ci] (+ old)"""
    B, H, W, Cin = x_img.shape
    Cout = dy_img.shape[3]
    tl = _taps(taps)
    want = torch.zeros(Cout, len(tl), Cin, dtype=F64, device=x_img.device)
    mag = torch.zeros_like(want)
    for b in range(B):
        xp = F.pad(nchw(x_img[b:b + 1]).to(F64), (1, 1, 1, 1))[0]
        d = dy_img[b].reshape(H * W, Cout).to(F64).t().contiguous()
        da = d.abs()
        for t, (ky, kx) in enumerate(tl):
            sl = xp[:, ky:ky + H, kx:kx + W].reshape(Cin, H * W).t()
            want[:, t] += d @ sl
            mag[:, t] += da @ sl.abs()
    want, mag = want.view(Cout, -1), mag.view(Cout, -1)
    if old is not None:
        want = want + old.to(F64)
        mag = mag + old.to(F64).abs()
    return want, GB.U24 * (Mc + 8 + ks) * mag


# ---- layout passes: expectations in image space -------------------------------------------------------------------------------------------------------
def im2col_expect(x_img, stride, pad, Kpad):
    """[B, H, W, C] -> [B, H/s, W/s, Kpad]: column tap C + c = the zero-padded image at (s yo + ky - pad, s xo + kx - pad); pad 0 is the (0,1,0,1) form"""
    B, H, W, C = x_img.shape
    Ho, Wo = H // stride, W // stride
    xp = F.pad(x_img, (0, 0, 1, 1, 1, 1)) if pad else F.pad(x_img, (0, 0, 0, 2, 0, 2))
    col = torch.zeros(B, Ho, Wo, Kpad, dtype=x_img.dtype, device=x_img.device)
    for t, (ky, kx) in enumerate(_taps(9)):
        col[..., t * C:(t + 1) * C] = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]
    return col


def col2im_expect(dcol_img, H, W, C, stride, pad):
    """the adjoint of im2col_expect in fp64: (want, e) [B, H, W, C], e = 2^-24 9 sum|terms|"""
    B, Ho, Wo, _ = dcol_img.shape
    lo = 1 if pad else 0
    acc = torch.zeros(B, H + 3, W + 3, C, dtype=F64, device=dcol_img.device)
    mag = torch.zeros_like(acc)
    d = dcol_img.to(F64)
    for t, (ky, kx) in enumerate(_taps(9)):
        acc[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] += d[..., t * C:(t + 1) * C]
        mag[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] += d[..., t * C:(t + 1) * C].abs()
    return acc[:, lo:lo + H, lo:lo + W], GB.U24 * 9 * mag[:, lo:lo + H, lo:lo + W]


def upsample_expect(x_img):
    return x_img.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample_bwd_expect(dy_img):
    B, H2, W2, C = dy_img.shape
    d = dy_img.to(F64).view(B, H2 // 2, 2, W2 // 2, 2, C)
    return d.sum((2, 4)), GB.U24 * 4 * d.abs().sum((2, 4))


def tokens_residual_expect(tok_img, res_img):
    t, r = tok_img.to(F64), res_img.to(F64)
    return t + r, GB.U24 * 2 * (t.abs() + r.abs())


def check_grid_copy(name, g, expect_img):
    """a layout pass that writes a whole grid: interior == expectation, border and tail == 0, bit for bit"""
    B, H, W, _ = expect_img.shape
    assert g.shape[0] == grid_rows(B, H, W), (name, g.shape)
    assert torch.equal(_bits(g), _bits(image_to_grid(expect_img))), f"{name}: differs from the independently indexed expectation"


def check_grid_sum(name, g, want_img, e_img):
    """a summing layout pass: interior bounded, border and tail exactly zero"""
    B, H, W, C = want_img.shape
    rows = interior_rows(B, H, W, g.device)
    z = torch.ones(g.shape[0], dtype=torch.bool, device=g.device)
    z[rows] = False
    assert not bool((_bits(g[z]) & 0x7FFF).any()), f"{name}: border / tail not zero"
    return GB.check(name, g[rows], want_img.reshape(-1, C), e_img.reshape(-1, C), rows=rows)


def dgrad_ref(dy_img, w, taps, K=None):
    """the adjoint of the convolution with respect to its input, scatter form, fp64, no autograd: dx[b, y+ky-1, x+kx-1, ci] += dy[b, y, x, co] w[co, tap Cin + ci].
    (want, e) [B H W, Cin] in (b, y, x) order; K: the kernel's contraction length (taps Cout; more when its columns are zero-padded)"""
    B, H, W, Cout = dy_img.shape
    tl = _taps(taps)
    Cin = w.shape[1] // len(tl)
    wt = w.to(F64).view(Cout, len(tl), Cin)
    acc = torch.zeros(B, H + 2, W + 2, Cin, dtype=F64, device=dy_img.device)
    mag = torch.zeros_like(acc)
    d = dy_img.to(F64)
    for t, (ky, kx) in enumerate(tl):
        acc[:, ky:ky + H, kx:kx + W] += d @ wt[:, t]
        mag[:, ky:ky + H, kx:kx + W] += d.abs() @ wt[:, t].abs()
    want = acc[:, 1:H + 1, 1:W + 1].reshape(-1, Cin)
    return want, GB.U24 * ((K or taps * Cout) + 8) * mag[:, 1:H + 1, 1:W + 1].reshape(-1, Cin) + GB.U20 * (1 + want.abs())

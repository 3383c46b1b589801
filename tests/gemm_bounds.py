"""Element-wise error bounds for the bf16 GEMM family (simpletuner_amd/csrc/gemm.hip) against an fp64 reference of the SAME bf16 (or dequantised fp8) operands.

Why a bound can be derived instead of fitted: a bf16 x bf16 (or e5m2 x e4m3) product is exact in fp32, so the kernel's accumulator differs from the fp64 value of
the same operands only by the fp32 summation error, at most 2^-24 (K + K2 + 8) sum|a b| (standard recursive-summation bound; the + 8 absorbs the bias add and
the fixed-order slab adds of split-K / stream-K).  Each stored output is then ONE round-to-nearest-even of an fp32 expression (f2bf, common.h).  So for an epilogue
f applied to the accumulator:

    err <= tol = 1/2 ulp_bf16(|ref| + e) + e,    e = |f'(ref)| 2^-24 (K + K2 + 8) mag + 2^-20 (1 + |f(ref)| + opmag)

mag = |A| |B|^T (+ |A2| |B2|^T) + |bias|.  The 2^-20 term covers the fp32 arithmetic of the epilogue itself: the exp2 / rcp forms of GELU (common.h; a few fp32
ulps) and the erf approximation of the GEGLU forms (|error| <= 1.5e-7), both far below one bf16 ulp; opmag is the size of the epilogue's fp32 operand that such an
error multiplies (|acc| for x GELU'(h), |value| for GEGLU, |gate acc| for the gated residual).

Epilogues that round twice get one extra ulp: EPI_GEGLU_GRAD rounds d out to bf16 before the products (gemm.hip, k_gemm_pq epilogue) — that rounding moves d by
at most 2^-8 |d|, i.e. the product by at most 2^-8 |f| < ulp_bf16(f).

Stored intermediates are chained: aux_out (the stored pre-activation) is checked against fp64 first; an output the kernel computes FROM that rounded value (GELU
with aux_out, GEGLU's value * gelu(gate)) is checked against the fp64 epilogue of the kernel's own aux_out, so a one-ulp tie difference cannot leak into the next stage.

Localisation: the worst-case bound grows with K and is loose at K ~ 16k, where a whole 64 x 64 block a few ulps off could hide under it.  Over 64 x 64 blocks the
check takes RMS(min(err / ulp_bf16(ref), 4)): one RNE rounding alone is uniform in +-1/2 ulp, RMS 1/sqrt(12) = 0.29, and the typical (random-walk) fp32
summation error adds well under 0.01 ulp at K <= 16384, so a block above 0.5 is wrong.  Twice-rounded outputs: the first rounding (<= 1/2 ulp of d, carried by a
factor of 0.5 ... 2 ulps of the output) adds another ~0.3 in quadrature; limit 0.8.  The cap of 4 keeps a single near-zero output (whose ulp is tiny next to the
fp32 summation error) from failing a block alone: it adds at most 16 / 4096 to the block's mean square, while any defect that covers a block still fails it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

F64 = torch.float64
U24 = 2.0 ** -24
U20 = 2.0 ** -20
RMS_LIMIT = 0.5
RMS_LIMIT_TWICE = 0.8
BLOCK = 64


def ulp_bf16(x):
    """the bf16 ulp at |x| (fp64 tensor): 2^(floor(log2 |x|) - 7); |x| below the smallest normal uses the subnormal spacing"""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def to_bf16_rne(x):
    """RNE to bf16 of an fp32 value (what f2bf does); fp64 input is first rounded to fp32, as the kernel's fp32 registers hold it"""
    return x.float().to(torch.bfloat16)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_tanh_grad(x):
    k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
    t = torch.tanh(k0 * (x + k1 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@dataclass
class Acc:
    """fp64 accumulator of the same operands (+ bias) and its worst-case fp32 summation error s = 2^-24 (K + K2 + 8) mag"""
    ref: torch.Tensor
    s: torch.Tensor


def gemm_ref(A, B, A2=None, B2=None, bias=None, scale=None):
    """acc = A B^T (+ A2 B2^T) (+ bias) in fp64 from the exact operand values (bf16, or dequantised fp8 given as fp32 / fp64); scale: an optional [M, N]-broadcastable
    fp64 factor applied to the product and its magnitude (linear_fp8's sa * sw[n]: the kernel scales the fp32 sum of the raw fp8 products)"""
    a, b = A.to(F64), B.to(F64)
    ref = a @ b.t()
    mag = a.abs() @ b.abs().t()
    K = A.shape[1]
    if A2 is not None:
        a2, b2 = A2.to(F64), B2.to(F64)
        ref += a2 @ b2.t()
        mag += a2.abs() @ b2.abs().t()
        K += A2.shape[1]
    if scale is not None:
        ref *= scale
        mag *= scale.abs() if torch.is_tensor(scale) else abs(scale)
    if bias is not None:
        ref += bias.to(F64)
        mag += bias.to(F64).abs()
    return Acc(ref, U24 * (K + 8) * mag)


# ---- epilogues: each returns [(name, want, e, rounds)] for the stored outputs it owns ------------------------------------------------------------------
def epi_none(acc):
    return acc.ref, acc.s


def epi_add(acc, res):
    r = res.to(F64)
    f = acc.ref + r
    return f, acc.s + U20 * (1 + f.abs())


def epi_gelu(acc):
    """C = gelu_tanh(fp32 acc) — no aux_out: the activation of the unrounded accumulator"""
    f = gelu_tanh(acc.ref)
    return f, gelu_tanh_grad(acc.ref).abs() * acc.s + U20 * (1 + f.abs())


def epi_gelu_of_stored(pre):
    """C = gelu_tanh(aux_out): GELU with aux_out activates the stored (rounded) pre-activation — chained on the kernel's own aux_out"""
    h = pre.to(F64)
    f = gelu_tanh(h)
    return f, U20 * (1 + f.abs())


def epi_gate_residual(acc, res, gate_rows):
    """C = res + gate[m / rows_per_batch] * (acc + bias); gate_rows: the [M, N] expansion of the gate rows"""
    g = gate_rows.to(F64)
    ga = g * acc.ref
    f = res.to(F64) + ga
    return f, g.abs() * acc.s + U20 * (1 + f.abs() + ga.abs())


def epi_mul_gelu_grad(acc, h):
    """C = acc * gelu_tanh'(h), h = aux_in (bf16, exact)"""
    gp = gelu_tanh_grad(h.to(F64))
    f = acc.ref * gp
    return f, gp.abs() * acc.s + U20 * (1 + f.abs() + acc.ref.abs())


def geglu_split(x):
    """[M, 2F] in the interleaved order of st355.h (every 64 columns: 32 values, then the 32 gates of the same features) -> (value [M, F], gate [M, F])"""
    M, N2 = x.shape
    v = x.view(M, N2 // 64, 2, 32)
    return v[:, :, 0].reshape(M, N2 // 2), v[:, :, 1].reshape(M, N2 // 2)


def geglu_join(value, gate):
    M, F_ = value.shape
    return torch.stack([value.reshape(M, F_ // 32, 32), gate.reshape(M, F_ // 32, 32)], dim=2).reshape(M, 2 * F_)


def epi_geglu_of_stored(pre):
    """EPI_GEGLU's C[M, F] = value * gelu_erf(gate), both halves read back as the bf16 values the kernel stored in aux_out (chained)"""
    v, g = geglu_split(pre.to(F64))
    f = v * gelu_erf(g)
    return f, U20 * (1 + f.abs() + v.abs())


def epi_geglu_grad(acc, pre):
    """EPI_GEGLU_GRAD: acc = d out [M, F]; pre = aux_in [M, 2F] (interleaved).  C[M, 2F] (interleaved) = d value | d gate with d = bf16(acc) (the second rounding)"""
    v, g = geglu_split(pre.to(F64))
    ge, gp = gelu_erf(g), gelu_erf_grad(g)
    dv = acc.ref * ge
    dg = acc.ref * v * gp
    e_dv = ge.abs() * acc.s + U20 * (1 + dv.abs() + acc.ref.abs())
    e_dg = (v * gp).abs() * acc.s + U20 * (1 + dg.abs() + (acc.ref * v).abs())
    return geglu_join(dv, dg), geglu_join(e_dv, e_dg)


# ---- the check ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Report:
    name: str
    worst: float            # max err / tol
    worst_at: tuple
    block_rms: float        # max over 64 x 64 blocks of RMS(min(err / ulp, 4))
    block_at: tuple         # (row block, col block) of that block
    block_tile: tuple       # the (row, col) tile of `tile` size holding it
    block_edge: bool        # that tile is a ragged last row / column tile
    rms_limit: float
    n: int

    @property
    def ok_elem(self):
        return self.worst <= 1.0

    @property
    def ok_block(self):
        return self.block_rms <= self.rms_limit

    @property
    def ok(self):
        return self.ok_elem and self.ok_block

    def line(self):
        return (f"[bound] {self.name}: worst err/tol={self.worst:.3f} at {self.worst_at}; worst 64x64 block RMS={self.block_rms:.3f} (limit {self.rms_limit}) "
                f"at block {self.block_at}, tile {self.block_tile}{' (edge tile)' if self.block_edge else ''}; {self.n} outputs")


def check(name, out, want, e, rounds=1, tile=(256, 256), rows=None, verbose=True):
    """out: the kernel's bf16 output [R, C]; want / e: fp64 [R, C] (the epilogue functions above); rounds: 2 for twice-rounded epilogues (one extra ulp, block
    limit 0.8).  rows: the logical row numbers of out's rows (row-sampled checks), for the location report.  Returns a Report; assert_bound() raises on it."""
    o = out.to(F64)
    assert o.shape == want.shape, (name, tuple(o.shape), tuple(want.shape))
    err = (o - want).abs()
    ulp = ulp_bf16(want.abs() + e)
    tol = (0.5 + (rounds - 1)) * ulp + e
    ratio = torch.where(torch.isfinite(o), err / tol, torch.full_like(err, math.inf))
    flat = int(torch.argmax(ratio))
    worst = float(ratio.view(-1)[flat])
    R, Cn = o.shape
    wr, wc = divmod(flat, Cn)
    u = torch.where(torch.isfinite(o), err / ulp_bf16(want), torch.full_like(err, 4.0)).clamp(max=4.0)
    rb, cb = (R + BLOCK - 1) // BLOCK, (Cn + BLOCK - 1) // BLOCK
    up = torch.zeros(rb * BLOCK, cb * BLOCK, dtype=F64, device=u.device)
    cnt = torch.zeros_like(up)
    up[:R, :Cn] = u * u
    cnt[:R, :Cn] = 1
    ms = up.view(rb, BLOCK, cb, BLOCK).sum((1, 3)) / cnt.view(rb, BLOCK, cb, BLOCK).sum((1, 3))
    bflat = int(torch.argmax(ms))
    brms = math.sqrt(float(ms.view(-1)[bflat]))
    br, bc = divmod(bflat, cb)
    row0 = int(rows[br * BLOCK]) if rows is not None else br * BLOCK
    Mlog = (int(rows[-1]) + 1) if rows is not None else R
    tr, tc = row0 // tile[0], (bc * BLOCK) // tile[1]
    edge = (Mlog % tile[0] != 0 and tr == Mlog // tile[0]) or (Cn % tile[1] != 0 and tc == Cn // tile[1])
    wrow = int(rows[wr]) if rows is not None else wr
    rep = Report(name, worst, (wrow, wc), brms, (row0 // BLOCK, bc), (tr, tc), edge, RMS_LIMIT if rounds == 1 else RMS_LIMIT_TWICE, R * Cn)
    if verbose:
        print(rep.line())
    return rep


def assert_bound(rep: Report):
    assert rep.ok_elem, rep.line()
    assert rep.ok_block, rep.line()


def rel_l2(out, ref):
    """the suite's existing global check"""
    o, r = out.to(F64), ref.to(F64)
    return float((o - r).norm() / r.norm().clamp_min(1e-300))

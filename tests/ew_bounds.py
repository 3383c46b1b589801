"""Element-wise error bounds for the kernels called BETWEEN the large families: the activations and the add (elementwise.hip k_unary_binary<0..3>), scale_cols,
the stand-alone GEGLU (k_geglu<false | true>), the row softmax and its backward (k_softmax_rows<1..32>, k_softmax_rows_bwd), the timestep projection, the TREAD
row gather / scatter, the bf16 transpose (reduce.hip) and the fp8 quantisers (fp8.hip), against an fp64 reference of the SAME stored inputs.

The rules (the project's, restated).
  * The reference is fp64 of the same stored bf16 / fp32 inputs (exact in fp64).  A scalar is the fp32 value that crosses the C ABI (SB.f32).
  * The kernels compute in fp32, u = 2^-24 per rounding.  The library is built with -ffp-contract=fast: a fused multiply-add rounds once where the bound counts
    two roundings, so a kernel never rounds more often than the count.
  * A sum along a tree whose longest chain has L additions is off by at most L u sum|terms|; L is read off the kernel's actual tree.
  * A bf16 output gets tol = 1/2 ulp_bf16(|ref| + e) + e (GB.check) and keeps the 64 x 64 block statistic RMS(min(err / ulp, 4)) <= 0.5.
  * No number below is fitted to a kernel's output.
  * Transcendental accuracies are the ones the project already uses: __expf 2^-21 (2 + |z|) relative (norm_bounds); sqrtf and a division 4 u (step_bounds);
    v_rcp_f32 1 ulp = 2 u (common.h).
  * v_exp_f32 (__builtin_amdgcn_exp2f: sigmoid2u, gelu_erf_parts) and the libm-grade expf / sinf / cosf of k_timestep_proj: the ROCm installation this was
    written against ships NO ISA or HIP-math accuracy table (its documentation directories hold licences and changelogs only), so NONE of the four figures is
    taken from documentation: all four use the fall-back the GEMM family's epilogues use, an ABSOLUTE allowance 2^-20 (1 + |f| + opmag) on the value f that
    the transcendental feeds, opmag being the fp32 operand its error multiplies (A20 below).  The error of an exponential's ARGUMENT is counted separately and
    becomes a relative error of the exponential (d exp(z) = exp(z) dz).

silu (OP 0):  f / (1 + __expf(-f)).  -f is exact.  E = exp(-f) carries 2^-21 (2 + |f|) relative; d = 1 + E carries E / d of it (= sigmoid(-f)) plus u; the
  division 4 u:      rel = r_d / (1 - r_d) + 4 u,   r_d = sigmoid(-f) 2^-21 (2 + |f|) + u,      e = rel |ref|.
  The bound is RELATIVE and holds for |f| <= 80, where exp(80) = 5.5e34 is finite in fp32.  Past |f| = 88.7 the sum 1 + exp(-f) overflows fp32 to infinity and
  the kernel returns -0 for a true value near -89 / 4.5e38 = -2e-37: an absolute error of 2e-37 that no relative bound covers.  The main bound is NOT widened
  for it; the edge vector (+-0, +-2^-126, +-80, +-89, +-1e4, +-3e38) asserts only what the expression guarantees there: a finite output of the right sign whose
  magnitude does not exceed the correctly rounded |ref| (the kernel underflows towards zero or saturates to the identity, it never overshoots) — and, on the
  saturating side x >= 80, where exp(-x) vanishes beside 1 and the expression returns x (dy for the backward) exactly, bit equality with the rounded
  reference (edge_exact): a zero there is an error.
silu_bwd (OP 2):  dy sg (1 + f (1 - sg)),  sg = 1 / (1 + __expf(-f)).  e_sg = sg rel (as above, 1.f / d being the division).  a = 1 - sg cancels for large f:
  its error is ABSOLUTE, e_a = e_sg + u a; b = f a: e_b = |f| e_a + u |b|; c = 1 + b: e_c = e_b + u |c|; p = dy sg: e_p = |dy| e_sg + u |p|;
      e = |p| e_c + |c| e_p + e_p e_c + u |ref|.
gelu_tanh (OP 3):  x sigmoid2u(x, x^2) = x rcp(1 + exp2(w)),  w = -x (c0 + c1 x^2).  c0, c1 are fp32 roundings of their constants (u each), x^2 one rounding,
  c1 x^2, the add and the product by x one each: e_w = 5 u |w|, i.e. 5 u |2u(x)| relative on the exponential (ln 2 |w| = |2u|).  d = 1 + E: r_d =
  sigmoid(-2u) 5 u |2u| + u;  rcp 2 u;  the product u:    e = |ref| (r_d / (1 - r_d) + 3 u) + A20(ref, |x|).
add (OP 1):  one fp32 rounding of an exact sum:  e = u |ref|.
scale_cols:  a product of two bf16 values is exact in fp32; the output is ONE RNE of it: bit-compared with GB.to_bf16_rne(x * gate).

GEGLU (k_geglu, gelu_erf_parts).  Phi(g) = 0.5 (1 + erf(g / sqrt 2)) by Abramowitz & Stegun 7.1.26, stated |error| <= 1.5e-7 on erf, 0.75e-7 on Phi (evaluated
  in fp64 over g in [-14, 14] the polynomial's own maximum is 6.97e-8).  That error is ABSOLUTE by construction: Phi(-5) = 2.9e-7, so below g = -5 the stored
  gelu(g) = g Phi(g) is off by more than half a bf16 ulp of itself (by tens of ulps at g = -6) — the tail is NOT relatively accurate.  That is accepted: the
  values there are |g Phi(g)| < 1.5e-6 beside activations of order 1 in the same row, F.gelu's consumers (a GEMM) sum them with fp32 weights, and an absolute
  1e-7 is below the bf16 resolution of every output that matters; libm's erff cost ~60 instructions per element (common.h).  The fp32 roundings on top:
      ax = |g| / sqrt 2              2 u (constant, product)
      t = rcp(1 + 0.3275911 ax)      6 u relative (constant, ax, fma: 4 u; rcp 2 u)
      poly(t), 5 fused steps         absolute: 6 u t sum k |a_k| + 10 u sum |a_k| (t's error through poly'; five roundings and five rounded constants at
                                     magnitudes <= sum |a_k| = 4.475; sum k |a_k| = 16.21)  <= 144 u t
      gauss = exp2(-ax^2 log2 e)     argument 7 u relative (ax twice, the square, the constant, the product) -> 3.5 u g^2 relative on gauss
      h = 0.5 poly gauss             2 u
      e_h = 0.5 gauss 144 u t + h (3.5 u g^2 + 2 u),      e_phi = 0.75e-7 + e_h + u Phi
  forward  v (g phi):    e = |v g| e_phi + 2 u |ref| + A20(ref, |v|)
  backward dv = d (g phi):   e = |d g| e_phi + 2 u |ref| + A20(ref, |d|)
           dg = d v grad,  grad = fma(g / sqrt(2 pi), gauss, phi):  e_grad = e_phi + |g| 0.3989 gauss (3.5 u g^2 + 3 u) + u |grad|   (the Gaussian term has no
           polynomial: the A&S error enters grad once, through phi);     e = |d v| e_grad + 2 u |ref| + A20(ref, |d v|)
  Block statistic of the GEGLU outputs: RMS(min(err / ulp, 4)) <= 0.5 measures RELATIVE accuracy, which the tail below g = -5 does not have by the account
  above: a correct fp32 emulation of the kernel's expression gives 0.57 - 0.58 at 2050 x 2056 with gates at three sigma (4.8 % of them below -5), 0.32 over the
  elements with g >= -5 (the CPU checker test asserts both figures' sides of 0.5).  So the statistic is taken over the elements with g >= -5 (check_geglu:
  the others are left out of a block's sum AND of its count; both halves of the backward's output); the element bound covers every element, the tail included.

softmax_rows (in place).  With M the kernel's own fp32 row maximum, softmax is exp(x s - M) / sum exp(x s - M) EXACTLY for any M, so only the differences count.
      v = x scale                   u |v|
      z = v - M                     u |z| more: e_z = u (|v| + |z|)      (|z| taken as |v - max v| + u |max v|: M is within u |max v| of the true maximum)
      E = __expf(z)                 relative r_E = expm1(e_z) + 2^-21 (2 + |z|)
      S = sum E                     chain L = 8 nch + 6 + 3 (8 nch values per thread, nch = cdiv(n, 2048), padding lanes add exact zeros; wave_sum 6; the four
                                    wave partials in order 3):  e_S = sum E r_E + L u S
      inv = 1 / S                   r_S / (1 - r_S) + 4 u,  r_S = e_S / S
      p = E inv                     u
      e = p (r_E + r_S / (1 - r_S) + 5 u)        (+ 2^-126 in the underflow rows: an exponential below the smallest normal may be flushed to zero)
  The launcher picks MAXC in {1, 2, 4, 8, 16, 32} as the first >= nch (softmax_maxc): the GPU test asserts that all six were launched.
softmax_rows_bwd (in place on dp):  ds = scale p (dp - dot), dot = sum p dp, a sum of EXACT products along L = 8 cdiv(n, 2048) + 9:  e_dot = L u sum |p dp|.
  The output cancels (dp - dot); its rounding terms (the difference, scale p, the product) are scaled by |scale p| (|dp| + |dot|), not by |ds|:
      e = |scale p| (e_dot + 3 u (|dp| + |dot|)).          p is a stored bf16 softmax output.

timestep_proj:  f = expf(c k / half), a = t scale f, out = [cos a | sin a]; c = fp32(-ln 1e4).  The reference is the fp64 value of that expression from the fp32
  t, scale and c.  The argument c k / half: one product, one division: 5 u |arg|, relative on f; expf itself A20(f, 0) = 2^-20 (1 + f) absolute:
      e_f = 5 u |arg| f + 2^-20 (1 + f);      e_a = |t scale| e_f + 2 u |a|  (t scale, then f);      e = e_a + A20(out, 0)      (|d cos|, |d sin| <= |da|)
  At t scale = 1000 e_a is ~1e-3, a quarter of a bf16 ulp of an output near 1: this bound is not just half an ulp, and says so.

gather_rows / scatter_rows / transpose_bf16 are copies: bit-compared with torch indexing, every byte outside the owned region keeping its prior bits.
fp8 quantisers: bit-compared (bytes and scales) with oracle.train_math.fp8_quantize_weight / fp8_quantize_act on the CPU, which tests/golden/fp8_vectors.pt pins to
the reference module bit for bit.  act_scale_f32() restates k_fp8_quant_act's scale lines in numpy fp32 for the CPU test."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests import step_bounds as SB

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
U = 2.0 ** -24
U20 = 2.0 ** -20
U_DIV = 4 * U
U_RCP = 2 * U
AS_PHI = 0.75e-7              # Abramowitz & Stegun 7.1.26: 1.5e-7 on erf
AS_SUM_A = 4.475              # sum |a_k|
AS_SUM_KA = 16.21             # sum k |a_k|
FLUSH = 2.0 ** -126
SOFTMAX_MAXC = (1, 2, 4, 8, 16, 32)

cdiv = NB.cdiv
f32 = SB.f32
as2d = SB.as2d
bits = SB.bits


def expf_rel(z):
    """__expf: 2^-21 (2 + |z|) relative (norm_bounds)"""
    return 2.0 ** -21 * (2 + z.abs())


def A20(f, opmag=0.0):
    """the epilogue allowance for a transcendental without a documented accuracy: 2^-20 (1 + |f| + opmag), absolute"""
    return U20 * (1 + f.abs() + opmag)


# ---- activations and add --------------------------------------------------------------------------------------------------------------------------------
def _sigmoid_rel(x):
    """sg = 1 / (1 + __expf(-x)): (sg, 1 - sg, relative error of sg), all stable at both ends"""
    sg, nsg = torch.sigmoid(x), torch.sigmoid(-x)
    r_d = nsg * expf_rel(x) + U
    return sg, nsg, r_d / (1 - r_d) + U_DIV


def silu(x):
    x = x.to(F64)
    sg, _, rel = _sigmoid_rel(x)
    want = x * sg
    return want, rel * want.abs()


def silu_bwd(x, dy):
    x, dy = x.to(F64), dy.to(F64)
    sg, a, rel = _sigmoid_rel(x)
    e_sg = sg * rel
    e_a = e_sg + U * a
    b = x * a
    e_b = x.abs() * e_a + U * b.abs()
    c = 1 + b
    e_c = e_b + U * c.abs()
    p = dy * sg
    e_p = dy.abs() * e_sg + U * p.abs()
    want = p * c
    return want, p.abs() * e_c + c.abs() * e_p + e_p * e_c + U * want.abs()


def gelu_tanh(x):
    x = x.to(F64)
    two_u = 2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    sg, nsg = torch.sigmoid(two_u), torch.sigmoid(-two_u)
    r_d = (nsg * 5 * U * two_u.abs()).clamp(max=0.5) + U
    want = x * sg
    return want, want.abs() * (r_d / (1 - r_d) + U_RCP + U) + A20(want, x.abs())


def add(a, b):
    want = a.to(F64) + b.to(F64)
    return want, U * want.abs()


def edge_vector(device=None):
    """+-0, +-2^-126, +-80, +-89, +-1e4, +-3e38 as bf16 (the nearest bf16 of each); no infinities, no NaN"""
    v = [0.0, 2.0 ** -126, 80.0, 89.0, 1e4, 3e38]
    return torch.tensor(v + [-t for t in v], dtype=F64, device=device).to(F32).to(BF16)


def edge_ok(out, want):
    """what the expressions guarantee on the edge vector: finite, the right sign (a zero of either sign where the value underflows), |out| <= RNE |ref|"""
    o, w = out.to(F64), GB.to_bf16_rne(want).to(F64)
    finite = torch.isfinite(o)
    sign = (o == 0) | (torch.signbit(o) == torch.signbit(w))
    small = o.abs() <= w.abs()
    return finite & sign & small


def edge_exact(x, out, want):
    """the saturating side of the edge vector, x >= 80: 1 + exp(-x) is exactly 1 in fp32 (exp(-80) = 1.8e-35 < 2^-24), so silu and gelu_tanh return x, silu_bwd
    dy and add one RNE of an exact sum: the output's bits are those of the rounded reference.  Returns the mask of elements that hold"""
    sat = x.to(F64) >= 80
    return ~sat | (bits(out) == bits(GB.to_bf16_rne(want)))


# ---- GEGLU -------------------------------------------------------------------------------------------------------------------------------------------------
def _phi_parts(g):
    """Phi(g), exp(-g^2 / 2) and the bound e_phi on the kernel's phi (module docstring)"""
    phi = 0.5 * torch.erfc(-g / math.sqrt(2.0))
    gauss = torch.exp(-0.5 * g * g)
    ax = g.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + 0.3275911 * ax)
    h = 0.5 * torch.erfc(ax)
    e_poly = (6 * AS_SUM_KA + 10 * AS_SUM_A) * U * t
    assert 6 * AS_SUM_KA + 10 * AS_SUM_A <= 144
    e_h = 0.5 * gauss * e_poly + h * (3.5 * U * g * g + 2 * U)
    return phi, gauss, AS_PHI + e_h + U * phi


def geglu_fwd(h, F_):
    """h [M, >= 2F] (value | gate), the logical columns: want [M, F], e"""
    v, g = h[:, :F_].to(F64), h[:, F_:2 * F_].to(F64)
    phi, _, e_phi = _phi_parts(g)
    want = v * g * phi
    return want, (v * g).abs() * e_phi + 2 * U * want.abs() + A20(want, v.abs())


def geglu_bwd(h, dout, F_):
    """want [M, 2F] = [d value | d gate], e"""
    v, g, d = h[:, :F_].to(F64), h[:, F_:2 * F_].to(F64), dout.to(F64)
    phi, gauss, e_phi = _phi_parts(g)
    dv = d * g * phi
    e_dv = (d * g).abs() * e_phi + 2 * U * dv.abs() + A20(dv, d.abs())
    k = 1.0 / math.sqrt(2.0 * math.pi)
    grad = phi + g * k * gauss
    e_grad = e_phi + g.abs() * k * gauss * (3.5 * U * g * g + 3 * U) + U * grad.abs()
    dg = d * v * grad
    e_dg = (d * v).abs() * e_grad + 2 * U * dg.abs() + A20(dg, (d * v).abs())
    return torch.cat([dv, dg], 1), torch.cat([e_dv, e_dg], 1)


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------------------
def softmax_nch(n):
    return cdiv(n, 2048)


def softmax_maxc(n):
    """the launcher's rule: the first MAXC >= nch"""
    nch = softmax_nch(n)
    return next(m for m in SOFTMAX_MAXC if nch <= m)


def L_softmax(n):
    return 8 * softmax_nch(n) + 6 + 3


def softmax_rows(x, scale, flush=False):
    """x [rows, n] (the logical columns), scale as given to the ABI: want, e"""
    s = f32(scale)
    v = x.to(F64) * s
    m = v.amax(1, keepdim=True)
    z = v - m
    zmag = z.abs() + U * m.abs()
    e_z = U * (v.abs() + zmag)
    E = torch.exp(z)
    r_E = torch.expm1(e_z) + expf_rel(zmag)
    S = E.sum(1, keepdim=True)
    r_S = ((E * r_E).sum(1, keepdim=True) + L_softmax(x.shape[1]) * U * S) / S
    want = E / S
    e = want * (r_E + r_S / (1 - r_S) + U_DIV + U)
    if flush:
        e = e + FLUSH
    return want, e


def softmax_rows_bwd(p, dp, scale):
    """p (a stored softmax output), dp [rows, n]: want, e"""
    s = f32(scale)
    p, dp = p.to(F64), dp.to(F64)
    n = p.shape[1]
    dot = (p * dp).sum(1, keepdim=True)
    e_dot = (8 * cdiv(n, 2048) + 9) * U * (p * dp).abs().sum(1, keepdim=True)
    want = s * p * (dp - dot)
    return want, (s * p).abs() * (e_dot + 3 * U * (dp.abs() + dot.abs()))


# ---- timestep projection -------------------------------------------------------------------------------------------------------------------------------------------
TS_C = float(np.float32(-9.210340371976184))


def timestep_proj(t, dim, scale):
    """t [B] fp32: want [B, dim] = [cos | sin], e"""
    half = dim // 2
    k = torch.arange(half, dtype=F64, device=t.device)
    arg = TS_C * k / half
    f = torch.exp(arg)
    e_f = 5 * U * arg.abs() * f + A20(f)
    ts = t.to(F64)[:, None] * f32(scale)
    a = ts * f
    e_a = ts.abs() * e_f + 2 * U * a.abs()
    want = torch.cat([torch.cos(a), torch.sin(a)], 1)
    return want, torch.cat([e_a, e_a], 1) + A20(want)


# ---- checks ------------------------------------------------------------------------------------------------------------------------------------------------------
def check_bf16(name, out, want, e, flat=False, verbose=True):
    return SB.check_bf16(name, out, want, e, flat=flat, verbose=verbose)


def check_elem(name, out, want, e, verbose=True):
    """element bound only (short rows, constant rows: no population for a block statistic)"""
    rep = GB.check(name, as2d(out), as2d(want.to(F64)), as2d(e.to(F64)), verbose=False)
    rep.block_rms = 0.0
    if verbose:
        print(f"[bound] {name}: worst err/tol={rep.worst:.3f} at {rep.worst_at}; {rep.n} outputs")
    return rep


GEGLU_TAIL = -5.0


def block_stat(out, want, keep=None):
    """max over 64 x 64 blocks of RMS(min(err / ulp_bf16(want), 4)) (GB.check's statistic) over the elements of `keep` (all if None): the elements left out
    count neither in a block's sum nor in its count"""
    o, w = out.to(F64), want.to(F64)
    u = torch.where(torch.isfinite(o), (o - w).abs() / GB.ulp_bf16(w), torch.full_like(w, 4.0)).clamp(max=4.0)
    k = torch.ones_like(w) if keep is None else keep.to(F64)
    R, Cn = w.shape
    rb, cb = cdiv(R, GB.BLOCK), cdiv(Cn, GB.BLOCK)
    sq = torch.zeros(rb * GB.BLOCK, cb * GB.BLOCK, dtype=F64, device=w.device)
    cnt = torch.zeros_like(sq)
    sq[:R, :Cn] = u * u * k
    cnt[:R, :Cn] = k
    B = GB.BLOCK
    ms = sq.view(rb, B, cb, B).sum((1, 3)) / cnt.view(rb, B, cb, B).sum((1, 3)).clamp_min(1)
    return math.sqrt(float(ms.max()))


def check_geglu(name, out, want, e, gate, verbose=True):
    """GEGLU: the element bound on every element; the block statistic over the elements whose gate is >= -5 (module docstring).  gate [M, F] is repeated
    over the column blocks of out ([M, F] forward, [M, 2F] backward)"""
    want, e = want.to(F64), e.to(F64)
    rep = GB.check(name, out, want, e, verbose=False)
    keep = (gate.to(F64) >= GEGLU_TAIL).repeat(1, out.shape[1] // gate.shape[1])
    rep.block_rms = block_stat(out, want, keep)
    if verbose:
        print(rep.line())
    return rep


# ---- fp8 -----------------------------------------------------------------------------------------------------------------------------------------------------------
def bf16_patterns(A, subnormal=False):
    """every finite bf16 bit pattern with |x| <= A, both signs (+-0 included): the normal ones (subnormal=False) or only the bf16 subnormals (subnormal=True)"""
    mag = torch.arange(0, 0x7F80, dtype=torch.int32)
    is_sub = (mag > 0) & (mag < 0x80)
    mag = mag[is_sub] if subnormal else mag[~is_sub]
    both = torch.cat([mag, mag | 0x8000]).to(torch.int16)          # wraps to the negative int16 of the same bits
    v = both.view(BF16)
    return v[v.float().abs() <= A]


def pad_to(v, K):
    """a flat bf16 vector zero-padded to [M, K]"""
    M = cdiv(v.numel(), K)
    out = torch.zeros(M * K, dtype=v.dtype, device=v.device)
    out[:v.numel()] = v
    return out.view(M, K)


def _bf_np(x):
    """RNE of a numpy fp32 array to bf16, returned as fp32 (integer arithmetic; finite inputs and infinities)"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def act_scale_f32(amax):
    """k_fp8_quant_act's scale lines in numpy fp32: amax (fp32 array of bf16 values) -> (input_scale, scale_a)"""
    one, top = np.float32(1.0), np.float32(57344.0)
    amax = _bf_np(amax)
    amin = _bf_np(np.float32(1e-12))
    with np.errstate(over="ignore", divide="ignore"):
        rcp = _bf_np(one / np.maximum(amax, amin))
        isc = np.minimum(_bf_np(rcp * top), top)
        return isc, _bf_np(one / isc)

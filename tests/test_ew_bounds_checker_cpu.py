"""The checker of tests/ew_bounds.py bites: fp32 emulations of the kernels' expressions (and, for the softmax sums, of their reduction trees), written in torch on
the CPU, pass every check — the worst ratios are printed: the reference alone stays inside the bound — and each planted defect is reported by the check named
beside it.  The cases are those of tests/test_ew_bounds_gpu.py that a CPU affords."""
import math

import numpy as np
import pytest
import torch

from tests import ew_bounds as EB
from tests import gemm_bounds as GB

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
SENT = 73728.0
WORST = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(x):
    return x.float().to(BF16)


def _trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (the planted conversion defect)"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def _lane_tree(v):
    """wave_sum: xor-shuffle tree over the last axis (64 lanes), offsets 32 ... 1"""
    o = v.shape[-1] // 2
    while o >= 1:
        v = v + v[..., torch.arange(v.shape[-1]) ^ o]
        o //= 2
    return v[..., 0]


def _passes(family, rep):
    w = WORST.setdefault(family, {"err/tol": 0.0, "block": 0.0})
    w["err/tol"] = max(w["err/tol"], rep.worst)
    w["block"] = max(w["block"], rep.block_rms)
    assert rep.ok, f"a correct emulation fails the check: {rep.line()}"


def _caught(rep, what, by):
    """by: 'element' (the element bound must fail), 'block' (the block statistic must fail) or 'both'"""
    print(f"[defect] {what}: element bound {'pass' if rep.ok_elem else 'FAIL'} ({rep.worst:.2f}), block statistic {'pass' if rep.ok_block else 'FAIL'} "
          f"({rep.block_rms:.2f})")
    if by in ("element", "both"):
        assert not rep.ok_elem, f"{what}: the element bound misses it"
    if by in ("block", "both"):
        assert not rep.ok_block, f"{what}: the block statistic misses it"


# ---- emulations ------------------------------------------------------------------------------------------------------------------------------------------------
def _sig(f):
    return 1.0 / (1.0 + torch.exp(-f))


def emu_unary(op, a, b=None, rnd=_bf, tail_left=0, defect=None):
    f = a.float()
    if op == "silu":
        y = f / (1.0 + torch.exp(-f))
    elif op == "gelu_tanh":
        c0, c1 = torch.tensor(2.302208198, dtype=F32), torch.tensor(0.1029432397, dtype=F32)
        y = f * (1.0 / (1.0 + torch.exp2(-f * (c0 + c1 * (f * f)))))
    elif op == "add":
        y = f + b.float()
    else:
        sg = _sig(f)
        y = b.float() * sg if defect == "no_x_term" else b.float() * sg * (1.0 + f * (1.0 - sg))
    out = rnd(y)
    if tail_left:
        out[-tail_left:] = SENT
    return out


def _act_inputs(seed, n):
    """randn * 3 with every eighth element uniform in [-80, 80]"""
    g = _gen(seed)
    x = torch.randn(n, generator=g) * 3
    x[::8] = (torch.rand(x[::8].shape, generator=g) * 160 - 80)
    return _bf(x), _bf(torch.randn(n, generator=g))


ACT_REF = {"silu": lambda a, b: EB.silu(a), "gelu_tanh": lambda a, b: EB.gelu_tanh(a), "add": lambda a, b: EB.add(a, b), "silu_bwd": lambda a, b: EB.silu_bwd(a, b)}


@pytest.mark.parametrize("op", ["silu", "silu_bwd", "gelu_tanh", "add"])
@pytest.mark.parametrize("n", [3, 8 * 1000 + 5, 262144 + 8 * 300 + 5])
def test_activation_emulations_pass(op, n):
    a, b = _act_inputs(n, n)
    want, e = ACT_REF[op](a, b)
    chk = EB.check_elem if n == 3 else (lambda *k: EB.check_bf16(*k, flat=True))
    _passes(op, chk(f"emu {op} n={n}", emu_unary(op, a, b), want, e))


def test_activation_edge_vector():
    a = EB.edge_vector()
    b = _bf(-0.5 * a.float())
    for op in ("silu", "gelu_tanh", "add", "silu_bwd"):
        bb = b if op == "add" else torch.full_like(a, 0.75)
        want, _ = ACT_REF[op](a, bb)
        out = emu_unary(op, a, bb)
        ok = EB.edge_ok(out, want)
        assert bool(ok.all()), (op, a[~ok].tolist())
        assert bool(EB.edge_exact(a, out, want).all()), op
        zeroed = out.clone()
        zeroed[a.float() >= 80] = 0.0                                        # passes edge_ok (a zero, never larger): edge_exact makes the check two-sided
        assert bool(EB.edge_ok(zeroed, want).all()) and not bool(EB.edge_exact(a, zeroed, want).all()), op
    assert not bool(EB.edge_ok(_bf(torch.tensor([1.5, -1.0, math.inf])), torch.tensor([1.0, 1.0, 1.0], dtype=F64)).any())          # larger, wrong sign, infinite


def test_activation_defects():
    n = 8 * 1000 + 5
    a, b = _act_inputs(n, n)
    want, e = EB.silu(a)
    _caught(EB.check_bf16("silu", emu_unary("silu", a, rnd=_trunc), want, e, flat=True, verbose=False), "truncation to bf16 instead of RNE (silu)", "both")
    _caught(EB.check_bf16("silu", emu_unary("silu", a, tail_left=5), want, e, flat=True, verbose=False), "a tail of 5 elements left at the sentinel (silu)", "element")
    want, e = EB.silu_bwd(a, b)
    _caught(EB.check_bf16("silu_bwd", emu_unary("silu_bwd", a, b, defect="no_x_term"), want, e, flat=True, verbose=False), "silu_bwd without x (1 - sg)", "both")
    want, e = EB.add(a, b)
    _caught(EB.check_bf16("add", emu_unary("add", a, b, rnd=_trunc), want, e, flat=True, verbose=False), "truncation to bf16 instead of RNE (add)", "element")          # many sums of two bf16 values need no rounding: the block statistic stays below 0.5


# ---- scale_cols ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale_cols_product_is_exact_in_fp32():
    """why the GPU test may compare bits: an 8-bit x 8-bit significand product has 16 bits, exact in fp32, so fp32 and fp64 products round to the same bf16"""
    g = _gen(5)
    x, gate = _bf(torch.randn(192, 520, generator=g) * 3), _bf(torch.randn(192, 520, generator=g))
    p32 = x.float() * gate.float()
    assert torch.equal(p32.double(), x.double() * gate.double())
    assert torch.equal(EB.bits(GB.to_bf16_rne(p32)), EB.bits(GB.to_bf16_rne(x.double() * gate.double())))
    assert not torch.equal(EB.bits(_trunc(p32)), EB.bits(GB.to_bf16_rne(p32)))


# ---- GEGLU ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _erf_parts(g):
    ax = g.abs() * torch.tensor(0.70710678118654752, dtype=F32)
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
    gauss = torch.exp2(-ax * ax * torch.tensor(1.4426950408889634, dtype=F32))
    h = 0.5 * poly * gauss
    return torch.where(g >= 0, 1.0 - h, h), gauss


def emu_geglu_fwd(h, F_, tanh=False, rnd=_bf):
    v, g = h[:, :F_].float(), h[:, F_:2 * F_].float()
    if tanh:
        return _bf(v * GB.gelu_tanh(g))
    return rnd(v * (g * _erf_parts(g)[0]))


def emu_geglu_bwd(h, d, F_):
    v, g, d = h[:, :F_].float(), h[:, F_:2 * F_].float(), d.float()
    phi, gauss = _erf_parts(g)
    grad = g * torch.tensor(0.39894228040143268, dtype=F32) * gauss + phi
    return torch.cat([_bf(d * (g * phi)), _bf(d * v * grad)], 1)


def _geglu_inputs(seed, M, F_, ldh):
    g = _gen(seed)
    h = _bf(torch.randn(M, ldh, generator=g))
    h[:, F_:2 * F_] = _bf(torch.randn(M, F_, generator=g) * 3)
    return h, _bf(torch.randn(M, F_, generator=g))


@pytest.mark.parametrize("M,F_", [(70, 40), (520, 1024)])
def test_geglu_emulations_pass_and_tanh_form_is_caught(M, F_):
    h, d = _geglu_inputs(M, M, F_, 2 * F_ + 16)
    want, e = EB.geglu_fwd(h, F_)
    gate = h[:, F_:2 * F_]
    _passes("geglu_fwd", EB.check_geglu(f"emu geglu_fwd M={M} F={F_}", emu_geglu_fwd(h, F_), want, e, gate))
    wb, eb = EB.geglu_bwd(h, d, F_)
    _passes("geglu_bwd", EB.check_geglu(f"emu geglu_bwd M={M} F={F_}", emu_geglu_bwd(h, d, F_), wb, eb, gate))
    _caught(EB.check_geglu("geglu", emu_geglu_fwd(h, F_, tanh=True), want, e, gate, verbose=False), "GEGLU with the tanh GELU in place of the erf one", "both")
    _caught(EB.check_geglu("geglu", emu_geglu_fwd(h, F_, rnd=_trunc), want, e, gate, verbose=False),
            "truncation to bf16 instead of RNE (GEGLU: the statistic over g >= -5 still counts roundings)", "both")
    plain = GB.check("geglu", emu_geglu_fwd(h, F_), want, e, verbose=False)
    print(f"[geglu] the statistic over ALL elements, the tail below g = -5 included, of the correct emulation: {plain.block_rms:.3f}")


def test_geglu_tail_is_why_the_statistic_leaves_it_out():
    """at 2050 x 2056 with gates at three sigma a CORRECT fp32 emulation exceeds 0.5 over all elements and stays below it over the gates >= -5: the all-element
    statistic measures the accepted absolute error of the erf polynomial, not a defect.  The left-out elements do not dilute a block: they leave its count too"""
    M, F_ = 2050, 2056
    h, _ = _geglu_inputs(M, M, F_, 2 * F_)
    want, e = EB.geglu_fwd(h, F_)
    out, gate = emu_geglu_fwd(h, F_), h[:, F_:2 * F_]
    every, kept = EB.block_stat(out, want), EB.check_geglu("emu geglu_fwd 2050 x 2056", out, want, e, gate)
    print(f"[geglu] correct emulation at {M} x {F_}: block statistic over all elements {every:.3f}, over gates >= -5 {kept.block_rms:.3f}")
    assert abs(every - GB.check("geglu", out, want, e, verbose=False).block_rms) < 1e-12          # block_stat without a mask is GB.check's statistic
    assert every > 0.5 and kept.ok
    o = torch.tensor([[1.0, 1.0 + 2.0 ** -5, 1.0, 1.0]], dtype=F64)                              # one element 4 ulps off among four
    w = torch.ones(1, 4, dtype=F64)
    assert abs(EB.block_stat(o, w) - 2.0) < 1e-12
    assert abs(EB.block_stat(o, w, torch.tensor([[True, True, False, False]])) - math.sqrt(8.0)) < 1e-12


def test_polynomial_stays_inside_the_stated_figure():
    """A&S 7.1.26 in fp64 over g in [-14, 14]: |Phi error| inside 0.75e-7; and the tail below g = -5 is off by more than half a bf16 ulp of gelu(g) (docstring)"""
    g = torch.linspace(-14, 14, 280001, dtype=F64)
    ax = g.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
    hh = 0.5 * poly * torch.exp(-ax * ax)
    phi = torch.where(g >= 0, 1 - hh, hh)
    err = (phi - 0.5 * torch.erfc(-g / math.sqrt(2.0))).abs()
    print(f"[poly] max |Phi error| = {float(err.max()):.3e}")
    assert float(err.max()) <= EB.AS_PHI
    tail = (g < -5) & (g > -8)
    ulps = (g.abs() * err / GB.ulp_bf16(g * phi))[tail]
    assert float(ulps.max()) > 0.5


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _thread_sums(t):
    """t [rows, n] fp32 terms (n a multiple of 8): every thread's running sum over its chunks in the kernel's order -> [rows, 256]"""
    rows, n = t.shape
    nch = EB.cdiv(n, 2048)
    pad = torch.zeros(rows, nch * 2048, dtype=F32)
    pad[:, :n] = t
    pad = pad.view(rows, nch, 256, 8)
    s = torch.zeros(rows, 256, dtype=F32)
    for c in range(nch):
        for j in range(8):
            s = s + pad[:, c, :, j]
    return s


def _block_sum(s, skip_wave=None):
    w = _lane_tree(s.view(-1, 4, 64))
    if skip_wave is not None:
        w = w.clone()
        w[:, skip_wave] = 0
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def emu_softmax(x, scale, defect=None):
    v = x.float() * torch.tensor(scale, dtype=F32)
    m = v.amax(1, keepdim=True)
    E = torch.exp(v - m)
    S = _block_sum(_thread_sums(E), skip_wave=2 if defect == "wave_missing" else None)
    y = E * (1.0 / S)[:, None]
    if defect == "row_scaled":
        y = y * (1 + 2.0 ** -8)
    return (_trunc if defect == "trunc" else _bf)(y)


def emu_softmax_bwd(p, dp, scale, defect=None):
    t = p.float() * dp.float()
    if defect == "dot_first_chunk":
        t = t.clone()
        t[:, 2048:] = 0
    dot = _block_sum(_thread_sums(t))[:, None]
    return _bf(torch.tensor(scale, dtype=F32) * p.float() * (dp.float() - dot))


def _scores(seed, rows, n):
    return _bf(torch.randn(rows, n, generator=_gen(seed)) * 3)


SM_CASES = [(8, 67), (2040, 67), (2056, 67), (4104, 67), (8200, 3), (16392, 3), (32776, 3), (65536, 3)]


@pytest.mark.parametrize("n,rows", SM_CASES)
def test_softmax_emulation_passes(n, rows):
    x = _scores(n, rows, n)
    want, e = EB.softmax_rows(x, 0.7)
    assert float((x.double() * EB.f32(0.7)).sub((x.double() * EB.f32(0.7)).amax(1, keepdim=True)).min()) >= -80
    _passes("softmax_rows", EB.check_bf16(f"emu softmax n={n}", emu_softmax(x, 0.7), want, e))


def test_softmax_maxc_rule_covers_all_six():
    assert {EB.softmax_maxc(n) for n, _ in SM_CASES} == set(EB.SOFTMAX_MAXC)
    assert [EB.softmax_maxc(n) for n, _ in SM_CASES] == [1, 1, 2, 4, 8, 16, 32, 32]


def test_softmax_small_rows():
    n = 264
    eq = _bf(torch.full((2, n), 1.375))
    want, e = EB.softmax_rows(eq, 0.7)
    out = emu_softmax(eq, 0.7)
    _passes("softmax_rows small", EB.check_elem("emu softmax all-equal", out, want, e))
    assert torch.equal(out, _bf(torch.full((2, n), 1.0 / n)))
    for scale, flush in ((1.0, False), (1.5, True)):
        one = _bf(torch.zeros(2, n))
        one[0, 5] = 60.0
        one[1, n - 1] = 60.0
        want, e = EB.softmax_rows(one, scale, flush=flush)
        _passes("softmax_rows small", EB.check_elem(f"emu softmax one element 60 above, scale {scale}", emu_softmax(one, scale), want, e))
    vae = _bf(torch.randn(3, 4104, generator=_gen(9)) * 40)
    s = 1.0 / math.sqrt(512.0)
    want, e = EB.softmax_rows(vae, s)
    _passes("softmax_rows small", EB.check_elem("emu softmax VAE form", emu_softmax(vae, s), want, e))


def test_softmax_defects():
    x = _scores(1, 67, 4104)
    want, e = EB.softmax_rows(x, 0.7)
    _caught(EB.check_bf16("softmax", emu_softmax(x, 0.7, "wave_missing"), want, e, verbose=False), "one of the four wave partials missing from the denominator", "both")
    _caught(EB.check_bf16("softmax", emu_softmax(x, 0.7, "row_scaled"), want, e, verbose=False), "softmax rows scaled by 1 + 2^-8", "both")
    _caught(EB.check_bf16("softmax", emu_softmax(x, 0.7, "trunc"), want, e, verbose=False), "truncation to bf16 instead of RNE (softmax)", "both")


SMB_CASES = [(8, 67), (2040, 67), (2056, 67), (16384, 3), (20488, 3)]


def _bwd_inputs(n, rows):
    p = emu_softmax(_scores(100 + n, rows, n), 0.7)
    return p, _bf(torch.randn(rows, n, generator=_gen(200 + n)))


@pytest.mark.parametrize("n,rows", SMB_CASES)
def test_softmax_bwd_emulation_passes(n, rows):
    p, dp = _bwd_inputs(n, rows)
    want, e = EB.softmax_rows_bwd(p, dp, 0.125)
    _passes("softmax_rows_bwd", EB.check_bf16(f"emu softmax_bwd n={n}", emu_softmax_bwd(p, dp, 0.125), want, e))


def test_softmax_bwd_defect():
    p, dp = _bwd_inputs(16384, 3)
    want, e = EB.softmax_rows_bwd(p, dp, 0.125)
    _caught(EB.check_bf16("softmax_bwd", emu_softmax_bwd(p, dp, 0.125, "dot_first_chunk"), want, e, verbose=False),
            "dot over the first 2048 columns only", "both")


# ---- timestep projection ------------------------------------------------------------------------------------------------------------------------------------------------
def emu_timestep(t, dim, scale, defect=None, rnd=_bf):
    half = dim // 2
    k = torch.arange(half, dtype=F32)
    den = torch.tensor(float(half - 1 if defect == "half_minus_1" else half), dtype=F32)
    f = torch.exp(torch.tensor(-9.210340371976184, dtype=F32) * k / den)
    a = t.float()[:, None] * torch.tensor(scale, dtype=F32) * f
    return rnd(torch.cat([torch.cos(a), torch.sin(a)], 1))


TS_CASES = [(torch.tensor([0.0, 1e-4, 0.1234, 0.5, 1.0]), 1000.0), (torch.tensor([0.0, 1.0, 37.0, 500.5, 999.0, 1000.0]), 1.0)]


@pytest.mark.parametrize("dim", [256, 320])
def test_timestep_emulation_passes_and_wrong_denominator_is_caught(dim):
    for t, scale in TS_CASES:
        want, e = EB.timestep_proj(t, dim, scale)
        _passes("timestep_proj", EB.check_bf16(f"emu timestep dim={dim} scale={scale}", emu_timestep(t, dim, scale), want, e))
    t, scale = TS_CASES[0]
    want, e = EB.timestep_proj(t, dim, scale)
    _caught(EB.check_bf16("timestep", emu_timestep(t, dim, scale, "half_minus_1"), want, e, verbose=False), "frequencies with half - 1 in the denominator", "both")
    _caught(EB.check_bf16("timestep", emu_timestep(t, dim, scale, rnd=_trunc), want, e, verbose=False), "truncation to bf16 instead of RNE (timestep_proj)", "both")


# ---- fp8 --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_act_scale_restatement_equals_the_oracle_for_every_amax():
    """every positive finite bf16 amax: the numpy fp32 restatement of k_fp8_quant_act's scale lines gives the oracle's input_scale and its reciprocal"""
    from oracle import train_math as TM

    amax = torch.arange(1, 0x7F80, dtype=torch.int32).to(torch.int16).view(BF16)
    isc, sa = EB.act_scale_f32(amax.float().numpy())
    o_is = (TM.FP8_E5M2_MAX / amax.clamp(min=1e-12)).clamp(max=TM.FP8_E5M2_MAX)          # the oracle's line on a vector: element-wise, the same arithmetic
    o_sa = o_is.reciprocal().to(F32)
    assert o_is.dtype == BF16
    assert np.array_equal(isc.view(np.uint32), o_is.float().numpy().view(np.uint32))
    assert np.array_equal(sa.view(np.uint32), o_sa.numpy().view(np.uint32))
    for i in range(0, amax.numel(), 97):                                                  # and the oracle function itself on a sample
        x = torch.zeros(1, 8, dtype=BF16)
        x[0, 3] = amax[i]
        q, s = TM.fp8_quantize_act(x)
        assert float(s) == float(sa[i]), (i, float(amax[i]))
    assert float(EB.act_scale_f32(np.float32(7.5))[0]) == 7680.0                           # two bf16 roundings, not one (7648)


def test_bf16_patterns():
    v = EB.bf16_patterns(3.4e38)
    assert v.numel() == 2 * (0x7F80 - 0x7F) and bool(torch.isfinite(v.float()).all())
    s = EB.bf16_patterns(3.4e38, subnormal=True)
    assert s.numel() == 2 * 0x7F and float(s.float().abs().max()) < 2.0 ** -126 and float(s.float().abs().min()) > 0
    assert float(EB.bf16_patterns(7.5).float().abs().max()) == 7.5
    assert EB.pad_to(EB.bf16_patterns(1.0), 264).shape[1] == 264


def test_worst_ratios_report():
    print("\n| family (CPU emulation) | worst err/tol | worst block statistic |\n|---|---|---|")
    for fam, w in sorted(WORST.items()):
        print(f"| {fam} | {w['err/tol']:.3f} | {w['block']:.3f} |")

"""Every kernel between the model's output and the next step's weights, element-wise against an fp64 reference of the same stored inputs (tests/step_bounds.py):
noise mix, loss and d loss / d pred, the rank-space LoRA gradients (skinny.hip), gradient norm / clip / clamp, AdamW, EMA and the LoRA operand packer.

Each case runs twice and must be bit-identical (the reductions are fixed-order), prefills every output buffer with a sentinel (or a non-zero prior) and asserts that
everything outside the region the call owns is untouched.  Where the ops wrapper allocates its outputs itself (noise mix, losses, grad_norm) the case calls the C ABI
directly with guarded buffers of its own.  The skinny cases assert the chunk the launcher chose (ops.skinny_plan ->
st355_skinny_plan) and the last tests assert that the cases reached all 18 routes {mfma<32>, mfma<64>, multi<128>} x mc {256, 512, 1024} x {plain, segmented}
and print the worst ratios per family: run the module as a whole.  The first-generation k_skinny_tn is reachable only through the ST355_SKINNY environment
variable, which the library reads once per process: it is not part of the enumeration."""
import os

import numpy as np
import pytest
import torch

from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests import step_bounds as SB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
HIT = set()
WORST = {}
ALL_ROUTES = {f"{k}|mc{mc}|{s}" for k in ("mfma<32>", "mfma<64>", "multi<128>") for mc in (256, 512, 1024) for s in ("plain", "seg")}
SENT = 73728.0           # sentinel (2^16 + 2^13: exact in bf16 and fp32), far from every value the kernels produce
PAD = 32                 # guard elements on both sides of a flat arena (keeps 16-byte alignment for fp32 and bf16)


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    assert os.environ.get("ST355_SKINNY", "") != "1", "the enumeration is of the MFMA skinny kernels (the library's default)"
    return o


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _randn(g, *shape, scale=1.0, shift=0.0, dtype=BF16):
    return (torch.randn(*shape, device=dev(), generator=g) * scale + shift).to(dtype)


def _note(family, rep):
    w = WORST.setdefault(family, {"err/tol": 0.0, "block": 0.0})
    w["err/tol"] = max(w["err/tol"], rep.worst)
    w["block"] = max(w["block"], rep.block_rms)
    if isinstance(rep, NB.SumReport):
        assert rep.ok, rep.line()
    else:
        GB.assert_bound(rep)


def _same(a, b, what):
    assert torch.equal(SB.bits(a), SB.bits(b)), f"{what}: two runs differ (the reduction order must be fixed)"


def _guarded(t, pad=PAD):
    """a copy of the flat tensor t inside a buffer with `pad` sentinel elements on both sides: (buffer, the view the library gets)"""
    n = t.numel()
    buf = torch.full((n + 2 * pad,), SENT, dtype=t.dtype, device=t.device)
    buf[pad:pad + n] = t.reshape(-1)
    return buf, buf[pad:pad + n]


def _guards_ok(buf, what, pad=PAD):
    s = torch.tensor(SENT, dtype=buf.dtype, device=buf.device)
    assert bool((buf[:pad] == s).all()) and bool((buf[-pad:] == s).all()), f"{what}: wrote outside its arena"


# ------------------------------------------------------------------------------------------------
# skinny
# ------------------------------------------------------------------------------------------------
def _operand(g, M, cols, c_lo, width, seg, s_extra, lo, shift=0.0):
    """a [M, width] operand as columns [c_lo, c_lo + width) of a wider buffer full of non-zero data; seg = (rows, B): rows [lo, lo + rows) of every sample of a
    joint [B, rows + s_extra, cols] buffer.  Returns (the view the library gets, the logical rows gathered [M, width])"""
    if seg is None:
        buf = _randn(g, M, cols, shift=shift)
        v = buf[:, c_lo:c_lo + width]
        return v, v
    rows, B = seg
    assert rows * B == M
    buf = _randn(g, B, rows + s_extra, cols, shift=shift)
    v = buf[:, lo:lo + rows, c_lo:c_lo + width]
    return v, v.reshape(M, width)


def _out_buffer(g, P, r_used, layout, accumulate):
    """both engine layouts: 'B' = (so_p, so_r) = (rank, 1) into gB[:, s0:] of a rank-128 adapter, s0 = 64; 'A' = (1, K) into gA[s0:, k0:], s0 = 64, k0 = 24.
    Returns (buffer, the view handed to the library, so_p, so_r, a function that extracts the owned [P, r_used] block, the owned mask)"""
    if layout == "B":
        shape, so_p, so_r = (P, 128), 128, 1
    else:
        K = P + 48
        shape, so_p, so_r = (128, K), 1, K
    buf = torch.randn(*shape, device=dev(), generator=g) if accumulate else torch.full(shape, SENT, device=dev())
    own = torch.zeros(shape, dtype=torch.bool, device=dev())
    if layout == "B":
        own[:, 64:64 + r_used] = True
        return buf, buf[:, 64:], so_p, so_r, (lambda b: b[:, 64:64 + r_used]), own
    own[64:64 + r_used, 24:24 + P] = True
    return buf, buf[64:, 24:], so_p, so_r, (lambda b: b[64:64 + r_used, 24:24 + P].t()), own


def _skinny(ops, M, P, Rn, r_used, seg=None, seg_mode="both", layout="B", alpha=0.37, accumulate=False, expect_mc=None, seed=0):
    g = _gen(1000 + seed)
    name = f"skinny M={M} P={P} Rn={Rn} r_used={r_used} seg={seg}/{seg_mode} out={layout} acc={accumulate}"
    segL = seg if seg is not None and seg_mode in ("both", "L") else None
    segR = seg if seg is not None and seg_mode in ("both", "R") else None
    Lv, Ll = _operand(g, M, 2 * P, 72, P, segL, 96, 64)
    Rv, Rl = _operand(g, M, 3 * Rn, Rn, Rn, segR, 32, 32, shift=0.25)
    plan = ops.skinny_plan(M, P, seg[0] if seg else 0)
    if expect_mc is not None:
        assert plan["mc"] == expect_mc, (name, plan)
    assert plan["nchunks"] == SB.cdiv(M, plan["mc"])
    HIT.add(f"mfma<{Rn}>|mc{plan['mc']}|{'seg' if seg else 'plain'}")
    buf, view, so_p, so_r, owned, own = _out_buffer(g, P, r_used, layout, accumulate)
    prior = buf.clone()
    ops.skinny_tn(Lv, Rv, view, so_p, so_r, r_used, alpha=alpha, accumulate=accumulate)
    first = buf.clone()
    buf.copy_(prior)
    ops.skinny_tn(Lv, Rv, view, so_p, so_r, r_used, alpha=alpha, accumulate=accumulate)
    _same(buf, first, name)
    assert torch.equal(SB.bits(buf)[~own], SB.bits(prior)[~own]), f"{name}: wrote outside [P, r_used]"
    want, e = SB.skinny(Ll, Rl[:, :r_used], alpha, plan["mc"], plan["nchunks"], prior=owned(prior) if accumulate else None)
    _note("skinny", SB.check_sum(name, owned(buf).contiguous(), want, e))


@pytest.mark.parametrize("Rn,r_used", [(32, 16), (64, 48)])
@pytest.mark.parametrize("P", [136, 320, 1152, 3072])
def test_skinny_operand_layouts(ops, P, Rn, r_used):
    """L a column block of a buffer twice as wide, R a column block of a wider T with r_used < Rn; 136 and 320 end inside a 128-column tile"""
    _skinny(ops, 300, P, Rn, r_used, layout="B", alpha=0.37, accumulate=False, expect_mc=256, seed=P + Rn)
    _skinny(ops, 300, P, Rn, r_used, layout="A", alpha=-1.7, accumulate=True, expect_mc=256, seed=P + Rn + 1)


@pytest.mark.parametrize("Rn,r_used", [(32, 16), (32, 32), (64, 48), (64, 64)])
@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_skinny_r_used_output_layouts_alpha_accumulate(ops, Rn, r_used, layout, accumulate):
    _skinny(ops, 577, 320, Rn, r_used, layout=layout, alpha=0.37 if accumulate else 1.0 / 3.0, accumulate=accumulate, expect_mc=256, seed=r_used)


@pytest.mark.parametrize("Rn", [32, 64])
@pytest.mark.parametrize("tail", [1, 63, 64, 65, 255])
def test_skinny_ragged_rows(ops, tail, Rn):
    _skinny(ops, 512 + tail, 136, Rn, Rn // 2, layout="A", accumulate=True, expect_mc=256, seed=tail)


@pytest.mark.parametrize("Rn", [32, 64])
@pytest.mark.parametrize("M,P,mc", [(3600, 8192, 512), (7200, 8192, 1024), (3600, 8200, 512), (7200, 8200, 1024)])
def test_skinny_large_chunks_with_ragged_tails(ops, M, P, mc, Rn):
    """the 512- and 1024-row chunks, each with a last chunk shorter than one 64-row sub-tile (16 / 32 rows), and a ragged P at a large chunk"""
    _skinny(ops, M, P, Rn, Rn - 16, layout="B" if Rn == 32 else "A", accumulate=(mc == 512), expect_mc=mc, seed=M + P)


@pytest.mark.parametrize("Rn", [32, 64])
@pytest.mark.parametrize("seg_mode", ["both", "L", "R"])
@pytest.mark.parametrize("rows,B,P,mc", [(256, 3, 320, 256), (768, 2, 136, 256), (512, 8, 8192, 512), (1024, 8, 8192, 1024)])
def test_skinny_segmented(ops, rows, B, P, mc, seg_mode, Rn):
    """[B, rows, C] views of joint buffers with non-zero rows outside; L segmented with R compact and the reverse (seg_l != seg_r, seg_r = 0)"""
    _skinny(ops, rows * B, P, Rn, Rn - 16, seg=(rows, B), seg_mode=seg_mode, layout="A" if seg_mode == "both" else "B", accumulate=(seg_mode == "L"),
            expect_mc=mc, seed=rows + Rn)


def _skinny_multi(ops, M, P, nout, r_used, wide, seg=None, expect_mc=None, accumulate=False, alpha=0.37, seed=0):
    g = _gen(2000 + seed)
    name = f"skinny_multi M={M} P={P} nout={nout} r_used={r_used} wide={wide} seg={seg} acc={accumulate}"
    Lv, Ll = _operand(g, M, 2 * P, 72, P, seg, 96, 64)
    Rv, Rl = _operand(g, M, 224, 32, 160, seg, 32, 32, shift=0.25) if wide else _operand(g, M, 128, 0, 128, seg, 32, 32, shift=0.25)
    plan = ops.skinny_plan(M, P, seg[0] if seg else 0)
    if expect_mc is not None:
        assert plan["mc"] == expect_mc, (name, plan)
    HIT.add(f"multi<128>|mc{plan['mc']}|{'seg' if seg else 'plain'}")
    outs = [_out_buffer(g, P, r_used, "A", accumulate) for _ in range(4)]          # four adapters' buffers; the first nout are handed over
    priors = [o[0].clone() for o in outs]
    so_p, so_r = outs[0][2], outs[0][3]
    ops.skinny_tn_multi(Lv, Rv, [o[1] for o in outs[:nout]], so_p, so_r, r_used, alpha=alpha, accumulate=accumulate)
    first = [o[0].clone() for o in outs]
    for o, p in zip(outs, priors):
        o[0].copy_(p)
    ops.skinny_tn_multi(Lv, Rv, [o[1] for o in outs[:nout]], so_p, so_r, r_used, alpha=alpha, accumulate=accumulate)
    for gi, (o, p, f) in enumerate(zip(outs, priors, first)):
        buf, _, _, _, owned, own = o
        _same(buf, f, name)
        if gi >= nout:
            assert torch.equal(SB.bits(buf), SB.bits(p)), f"{name}: output {gi} beyond nout was written"
            continue
        assert torch.equal(SB.bits(buf)[~own], SB.bits(p)[~own]), f"{name}: output {gi} written outside [P, r_used]"
        want, e = SB.skinny(Ll, Rl[:, 32 * gi:32 * gi + r_used], alpha, plan["mc"], plan["nchunks"], prior=owned(p) if accumulate else None)
        _note("skinny multi", SB.check_sum(f"{name} out {gi}", owned(buf).contiguous(), want, e))


@pytest.mark.parametrize("nout", [1, 2, 3, 4])
@pytest.mark.parametrize("r_used", [16, 32])
@pytest.mark.parametrize("wide", [False, True])
def test_skinny_multi(ops, nout, r_used, wide):
    """R with exactly 128 columns and with more, plain and segmented; the outputs beyond nout stay untouched"""
    _skinny_multi(ops, 577, 320, nout, r_used, wide, expect_mc=256, accumulate=(nout % 2 == 0), seed=nout)
    _skinny_multi(ops, 768, 136, nout, r_used, wide, seg=(256, 3), expect_mc=256, accumulate=(nout % 2 == 1), seed=nout + 10)


@pytest.mark.parametrize("M,P,seg,mc", [(3600, 8192, None, 512), (7200, 8200, None, 1024), (4096, 8192, (512, 8), 512), (8192, 8192, (1024, 8), 1024)])
def test_skinny_multi_large_chunks(ops, M, P, seg, mc):
    _skinny_multi(ops, M, P, 3, 16 if mc == 512 else 32, wide=(mc == 1024), seg=seg, expect_mc=mc, accumulate=(seg is not None), seed=M)


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
def _loss_inputs(seed, B, n):
    """residuals at three scales in one tensor (|d| ~ 1, ~ c, ~ 1e-3 c), the target at the residual's scale so that bf16 can hold the small ones"""
    g = _gen(3000 + seed)
    c = (0.01 + 0.99 * torch.rand(B, device=dev(), generator=g)).float()
    sc = torch.stack([torch.ones_like(c), c, 1e-3 * c], 1)[:, torch.arange(n, device=dev()) % 3]
    target = (3.0 * sc * torch.randn(B, n, device=dev(), generator=g)).to(BF16)
    pred = (target.float() + sc * torch.randn(B, n, device=dev(), generator=g)).to(BF16)
    w = (0.5 + torch.rand(B, device=dev(), generator=g)).float()
    return pred, target, c, w, g


def _mask(g, B, period):
    em = torch.rand(B, period, device=dev(), generator=g).float()
    em[:, ::5] = 0.0
    em[:, 1::7] = 2.5
    return em


def _loss_case(ops, loss_type, pred, target, c, w, em, grad_scale, want_grad=True):
    B, n = pred.shape
    name = f"{loss_type} B={B} n={n} w={w is not None} c={'vec' if torch.is_tensor(c) else c} mask={None if em is None else em.shape[1]} gs={grad_scale}"
    kw = dict(loss_type=loss_type, huber_c=c, weight=w, want_grad=want_grad, grad_scale=grad_scale, emask=em)
    lo, per, dp = ops.cond_loss(pred, target, **kw)
    lo2, per2, dp2 = ops.cond_loss(pred, target, **kw)
    _same(lo, lo2, name); _same(per, per2, name)
    cv = c if torch.is_tensor(c) else torch.full((B,), SB.f32(c), device=dev())
    ref = SB.loss(pred, target, loss_type, huber_c=cv, weight=w, emask=em, grad_scale=grad_scale)
    _note("loss per-sample", SB.check_sum(f"{name} per-sample", per.reshape(1, -1), ref["per_sample"][0].reshape(1, -1), ref["per_sample"][1].reshape(1, -1)))
    _note("loss batch", SB.check_sum(f"{name} loss", lo.reshape(1, 1), ref["loss"][0].reshape(1, 1), ref["loss"][1].reshape(1, 1)))
    if not want_grad:
        assert dp is None
        return lo, per
    _same(dp, dp2, name)
    _note("dpred", SB.check_bf16(f"{name} dpred", dp, *ref["dpred"]))
    return lo, per


PER_SAMPLE = [(8, 8), (8 * 1024 - 8, 8 * 1024 - 8), (8 * 1024 + 8, 8 * 1024 + 8), (4 * 64 * 64, 64 * 64), (16 * 48 * 40, 48 * 40)]      # (per_sample, H * W)


@pytest.mark.parametrize("loss_type", ["l2", "huber", "smooth_l1"])
@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("n,hw", PER_SAMPLE)
def test_loss_and_dpred(ops, loss_type, B, n, hw):
    pred, target, c, w, g = _loss_inputs(B * 7 + n, B, n)
    lo, per = _loss_case(ops, loss_type, pred, target, 0.1, None, None, 1.0)
    if loss_type == "l2":          # st355_mse_loss is the same kernel behind its own entry point
        lo_m, per_m, dp_m = ops.mse_loss(pred, target)
        _same(lo, lo_m, "mse_loss vs cond_loss l2"); _same(per, per_m, "mse_loss vs cond_loss l2")
    _loss_case(ops, loss_type, pred, target, c, w, None, 0.7)
    _loss_case(ops, loss_type, pred, target, c, w, _mask(g, B, hw), 0.7)               # mask_period = H * W (< per_sample where C > 1): repeats over the channels
    if hw != n:
        _loss_case(ops, loss_type, pred, target, 0.1, None, _mask(g, B, n), 1.3)       # mask_period == per_sample
    lo_n, per_n = _loss_case(ops, loss_type, pred, target, c, w, None, 0.7, want_grad=False)


@pytest.mark.parametrize("loss_type", ["l2", "huber", "smooth_l1"])
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("n,hw", PER_SAMPLE + [(4 * 32 * 40, 32 * 40)])
def test_loss_writes_only_its_outputs(ops, loss_type, want_grad, n, hw):
    """through the C ABI with guarded, sentinel-filled buffers at every size of PER_SAMPLE (the ragged 8 x 1024 +- 8 and per_sample = 8 among them), masked, with
    and without dpred: dpred, the per-sample losses and the loss are all the call may write, it writes all of them, and they are what ops.cond_loss returns"""
    from simpletuner_amd import lib as _l

    B = 3
    pred, target, c, w, g = _loss_inputs(99 + n, B, n)
    em = _mask(g, B, hw)
    dbuf, dp = _guarded(torch.full((B * n,), SENT, dtype=BF16, device=dev()))
    pbuf, per = _guarded(torch.full((B,), SENT, dtype=F32, device=dev()))
    lbuf, lo = _guarded(torch.full((1,), SENT, dtype=F32, device=dev()))
    ins = [t.clone() for t in (pred, target, w, c, em)]
    st = torch.cuda.current_stream().cuda_stream
    _l.check(_l.load().st355_cond_loss_masked(st, pred.data_ptr(), target.data_ptr(), w.data_ptr(), c.data_ptr(), ops.LOSS_TYPES[loss_type], em.data_ptr(), hw,
                                              lo.data_ptr(), per.data_ptr(), dp.data_ptr() if want_grad else None, B, n, 0.7), "cond_loss")
    torch.cuda.synchronize()
    for b_, what in ((dbuf, "dpred"), (pbuf, "per-sample"), (lbuf, "loss")):
        _guards_ok(b_, f"{loss_type} {what}")
    for t, t0 in zip((pred, target, w, c, em), ins):
        assert torch.equal(t, t0), f"{loss_type}: an input was written"
    lo2, per2, dp2 = ops.cond_loss(pred, target, loss_type=loss_type, huber_c=c, weight=w, grad_scale=0.7, emask=em, want_grad=want_grad)
    _same(per, per2, "guarded per-sample"); _same(lo, lo2, "guarded loss")
    if want_grad:
        _same(dp, dp2.reshape(-1), "guarded dpred")
    else:
        assert dp2 is None and bool((dp == SENT).all()), f"{loss_type}: dpred written although none was asked for"


# ------------------------------------------------------------------------------------------------
# noise mix
# ------------------------------------------------------------------------------------------------
SIGMA = [0.0, 1.0, 0.3, 0.77, 0.5]
MIX_PER = [8, 4 * 64 * 64, 8 * 104864]           # B = 5: the last is 4 194 560 elements, past 8 x 524 288: a second grid-stride pass


def _mix_out(numel, wanted=True):
    """a guarded, sentinel-filled bf16 output of numel elements: (buffer, view); (None, None) for an output the call does not ask for"""
    return _guarded(torch.full((numel,), SENT, dtype=BF16, device=dev())) if wanted else (None, None)


def _mix_done(name, ins, outs):
    """after the call: the inputs are unchanged, no guard is touched, every output that was handed over is written throughout (the kernels never produce SENT)"""
    torch.cuda.synchronize()
    for t, t0 in ins:
        assert torch.equal(SB.bits(t), SB.bits(t0)), f"{name}: an input was written"
    for what, (buf, view) in outs.items():
        if buf is None:
            continue
        _guards_ok(buf, f"{name} {what}")
        assert not bool((view == SENT).any()), f"{name} {what}: elements left unwritten"


def _flow_mix(ops, x, sig, noise=None, want_target=True, seed=0, offset=0):
    """st355_flow_noise_mix through the C ABI (ops.flow_noise_mix allocates its outputs itself).  Returns (x_t, target | None, the noise used) as [B, per]"""
    from simpletuner_amd import lib as _l

    B, per = x.shape
    name = f"flow_noise_mix per={per} noise={'given' if noise is not None else 'generated'} target={want_target}"
    outs = {"x_t": _mix_out(B * per), "target": _mix_out(B * per, want_target), "noise_out": _mix_out(B * per, noise is None)}
    ins = [(t, t.clone()) for t in (x, sig) + ((noise,) if noise is not None else ())]
    _l.check(_l.load().st355_flow_noise_mix(torch.cuda.current_stream().cuda_stream, x.data_ptr(), ops._ptr(noise), sig.data_ptr(), outs["x_t"][1].data_ptr(),
                                            ops._ptr(outs["target"][1]), ops._ptr(outs["noise_out"][1]), B, per, seed, offset), "flow_noise_mix")
    _mix_done(name, ins, outs)
    v = lambda k: None if outs[k][1] is None else outs[k][1].view(B, per)
    return v("x_t"), v("target"), (noise if noise is not None else v("noise_out"))


def _ddpm_mix(ops, x, n, a, s, want_v=True):
    from simpletuner_amd import lib as _l

    B, per = x.shape
    name = f"ddpm_noise_mix per={per} v={want_v}"
    outs = {"x_t": _mix_out(B * per), "v": _mix_out(B * per, want_v)}
    ins = [(t, t.clone()) for t in (x, n, a, s)]
    _l.check(_l.load().st355_ddpm_noise_mix(torch.cuda.current_stream().cuda_stream, x.data_ptr(), n.data_ptr(), a.data_ptr(), s.data_ptr(),
                                            outs["x_t"][1].data_ptr(), ops._ptr(outs["v"][1]), B, per), "ddpm_noise_mix")
    _mix_done(name, ins, outs)
    return outs["x_t"][1].view(B, per), (outs["v"][1].view(B, per) if want_v else None)


@pytest.mark.parametrize("per", MIX_PER)
def test_flow_noise_mix_given_noise(ops, per):
    g = _gen(4000 + per)
    x, n = _randn(g, 5, per, scale=1.5), _randn(g, 5, per)
    sig = torch.tensor(SIGMA, device=dev())
    xt, tg, n_out = _flow_mix(ops, x, sig, noise=n)
    xt2, tg2, _ = _flow_mix(ops, x, sig, noise=n)
    _same(xt, xt2, "flow x_t"); _same(tg, tg2, "flow target")
    (w1, e1), (w2, e2) = SB.flow_mix(x, n, sig)
    _note("noise mix", SB.check_bf16(f"flow x_t per={per}", xt, w1, e1, flat=True))
    _note("noise mix", SB.check_bf16(f"flow target per={per}", tg, w2, e2, flat=True))
    assert torch.equal(SB.bits(xt[0]), SB.bits(x[0])) and torch.equal(SB.bits(xt[1]), SB.bits(n[1]))          # sigma = 0 and sigma = 1
    xt3, tg3, _ = _flow_mix(ops, x, sig, noise=n, want_target=False)          # no target buffer: x_t the same, nothing else written (the guards of _flow_mix)
    _same(xt3, xt, "flow x_t without the target")
    xt4, tg4, n4 = ops.flow_noise_mix(x, sig, noise=n)                         # the wrapper hands over the same call
    _same(xt4, xt, "ops.flow_noise_mix x_t"); _same(tg4, tg, "ops.flow_noise_mix target")
    assert ops.flow_noise_mix(x, sig, noise=n, want_target=False)[1] is None


@pytest.mark.parametrize("per", MIX_PER)
def test_flow_noise_mix_generated_noise(ops, per):
    g = _gen(4100 + per)
    x = _randn(g, 5, per, scale=1.5)
    sig = torch.tensor(SIGMA, device=dev())
    xt, tg, n = _flow_mix(ops, x, sig, noise=None, seed=77, offset=1 << 20)
    xt2, tg2, n2 = _flow_mix(ops, x, sig, noise=None, seed=77, offset=1 << 20)
    _same(n, n2, "generated noise (same seed and offset)"); _same(xt, xt2, "flow x_t"); _same(tg, tg2, "flow target")
    assert bool(torch.isfinite(n.float()).all())
    (w1, e1), (w2, e2) = SB.flow_mix(x, n, sig)           # chained on the kernel's own stored noise
    _note("noise mix", SB.check_bf16(f"flow (generated) x_t per={per}", xt, w1, e1, flat=True))
    _note("noise mix", SB.check_bf16(f"flow (generated) target per={per}", tg, w2, e2, flat=True))
    xt3, tg3, n3 = _flow_mix(ops, x, sig, noise=None, want_target=False, seed=77, offset=1 << 20)
    _same(xt3, xt, "flow (generated) x_t without the target"); _same(n3, n, "generated noise without the target")
    xt4, tg4, n4 = ops.flow_noise_mix(x, sig, noise=None, seed=77, offset=1 << 20)
    _same(xt4, xt, "ops.flow_noise_mix x_t"); _same(tg4, tg, "ops.flow_noise_mix target"); _same(n4, n, "ops.flow_noise_mix noise")
    if per > 8:
        _, _, n5 = _flow_mix(ops, x, sig, noise=None, seed=78, offset=1 << 20)
        assert not torch.equal(n, n5)
        nf = n.float()
        assert abs(nf.mean().item()) < 2e-2 and abs(nf.std().item() - 1.0) < 2e-2          # a coarse screen; the moment test of test_kernels_gpu.py stays the bar


@pytest.mark.parametrize("per", MIX_PER)
def test_ddpm_noise_mix(ops, per):
    g = _gen(4200 + per)
    x, n = _randn(g, 5, per, scale=1.5), _randn(g, 5, per)
    acp = torch.tensor([1.0, 0.0, 0.9, 0.2, 0.5], device=dev())
    a, s = acp.sqrt(), (1 - acp).sqrt()
    xt, v = _ddpm_mix(ops, x, n, a, s)
    xt2, v2 = _ddpm_mix(ops, x, n, a, s)
    _same(xt, xt2, "ddpm x_t"); _same(v, v2, "ddpm v")
    (w1, e1), (w2, e2) = SB.ddpm_mix(x, n, a, s)
    _note("noise mix", SB.check_bf16(f"ddpm x_t per={per}", xt, w1, e1, flat=True))
    _note("noise mix", SB.check_bf16(f"ddpm v per={per}", v, w2, e2, flat=True))
    xt3, _ = _ddpm_mix(ops, x, n, a, s, want_v=False)
    _same(xt3, xt, "ddpm x_t without v")
    xt4, v4 = ops.ddpm_noise_mix(x, n, a, s)
    _same(xt4, xt, "ops.ddpm_noise_mix x_t"); _same(v4, v, "ops.ddpm_noise_mix v")
    assert ops.ddpm_noise_mix(x, n, a, s, want_v=False)[1] is None


# ------------------------------------------------------------------------------------------------
# gradient norm / clip / clamp
# ------------------------------------------------------------------------------------------------
def _grad_norm(ops, g):
    """st355_grad_norm_ws through the C ABI (ops.grad_norm allocates the two statistics itself): the [2] output and the 2 x 1024 scratch are guarded and
    sentinel-filled, the gradient is unchanged"""
    from simpletuner_amd import lib as _l

    obuf, out = _guarded(torch.full((2,), SENT, dtype=F32, device=dev()))
    wbuf, ws = _guarded(torch.full((2 * 1024,), SENT, dtype=F32, device=dev()))
    g0 = g.clone()
    _l.check(_l.load().st355_grad_norm_ws(torch.cuda.current_stream().cuda_stream, g.data_ptr(), g.numel(), g.element_size(), out.data_ptr(), ws.data_ptr()),
             "grad_norm")
    torch.cuda.synchronize()
    _guards_ok(obuf, "grad_norm stats"); _guards_ok(wbuf, "grad_norm scratch")
    assert torch.equal(SB.bits(g), SB.bits(g0)), "grad_norm: the gradient was written"
    assert not bool((out == SENT).any()), "grad_norm: a statistic left unwritten"
    return out.clone()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n", [1, 255, 257, 262145, 3000001])
def test_grad_norm(ops, n, dtype):
    g = _randn(_gen(5000 + n), n, scale=0.02, dtype=dtype)
    for last_is_max in (False, True):
        if last_is_max:
            g[-1] = 0.5                                        # the largest |g| in the last element
        st = _grad_norm(ops, g)
        st2 = _grad_norm(ops, g)
        _same(st, st2, f"grad_norm n={n}")
        _same(st, ops.grad_norm(g), f"ops.grad_norm n={n}")
        want, e, mx = SB.grad_norm(g)
        _note("grad_norm", SB.check_sum(f"grad_norm n={n} {dtype}", st[0:1].reshape(1, 1), want, e))
        assert float(st[1]) == float(mx), f"grad_norm n={n}: max |g| {float(st[1])} != {float(mx)}"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("max_norm,clips", [(1.0, True), (100.0, False)])
def test_grad_clip_norm(ops, dtype, max_norm, clips):
    n, pre = 600001, 0.5
    g0 = _randn(_gen(5100), n, scale=0.02, dtype=dtype)       # norm ~ 15.5, ~ 7.7 after pre_scale
    buf, g = _guarded(g0)
    st = ops.grad_norm(g)
    ops.grad_clip_norm_(g, st, max_norm, pre_scale=pre)
    first = g.clone()
    g.copy_(g0)
    ops.grad_clip_norm_(g, st, max_norm, pre_scale=pre)
    _same(g, first, "grad_clip_norm")
    _guards_ok(buf, "grad_clip_norm")
    coef = SB.clip_coef(float(st[0]), max_norm, pre)
    assert (coef < 1.0) == clips
    if not clips:
        assert torch.equal(SB.bits(g), SB.bits(g0)), "grad_clip_norm: coef >= 1 must leave every element's bits alone"
        return
    want, e = SB.grad_clip(g0, coef)
    _note("grad_clip", SB.check_f32(f"grad_clip_norm {dtype}", g, want, e) if dtype == F32 else SB.check_bf16(f"grad_clip_norm {dtype}", g, want, e, flat=True))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_grad_clamp(ops, dtype):
    n, c = 600001, 0.013
    g0 = _randn(_gen(5200), n, scale=0.02, dtype=dtype)
    buf, g = _guarded(g0)
    ops.grad_clamp_(g, c)
    _guards_ok(buf, "grad_clamp")
    want = g0.float().clamp(-SB.f32(c), SB.f32(c)).to(dtype)          # exact: a comparison, then (bf16) one RNE of the fp32 bound
    assert torch.equal(SB.bits(g), SB.bits(want))


# ------------------------------------------------------------------------------------------------
# AdamW / EMA
# ------------------------------------------------------------------------------------------------
def _adam_state(seed, n, dtype):
    g_ = _gen(6000 + seed)
    p = _randn(g_, n, scale=0.05, dtype=dtype)
    g = _randn(g_, n, scale=1e-3, dtype=dtype)
    m = _randn(g_, n, scale=1e-3, dtype=F32)
    v = _randn(g_, n, scale=1e-3, dtype=F32) ** 2
    m[::22] = 0
    v[::11] = 0
    g[::11] = 0                                                # v = 0 and g = 0: the denominator is eps; m = 0 on half of them, on the others the update is
                                                               # step_size m' / eps, so that a wrong denominator there moves p
    ema = (p.float() + 1e-3 * torch.randn(n, device=dev(), generator=g_)).to(dtype)
    return p, g, m, v, ema


def _adam_case(ops, n, dtype, step, wd, with_ema, with_pb, seed):
    name = f"adamw {dtype} n={n} step={step} wd={wd} ema={with_ema} p_bf16={with_pb}"
    p0, g, m0, v0, e0 = _adam_state(seed, n, dtype)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, grad_scale=0.5, ema_decay=0.99)
    c = SB.adam_consts(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, step, hp["grad_scale"], hp["ema_decay"])
    bufs = [_guarded(t) for t in (p0, m0, v0, e0)]
    (pb_, p), (mb_, m), (vb_, v), (eb_, ema) = bufs
    gb_, gv = _guarded(g)
    hb_, pbf = _guarded(torch.full((n,), SENT, dtype=BF16, device=dev()))
    kw = dict(ema=ema if with_ema else None, p_bf16=pbf if with_pb else None) if dtype == F32 else dict(ema=ema if with_ema else None)
    ops.adamw_ema_step(p, gv, m, v, step, **hp, **kw)
    first = [t.clone() for t in (p, m, v, ema, pbf)]
    for t, t0 in ((p, p0), (m, m0), (v, v0), (ema, e0)):
        t.copy_(t0)
    pbf.fill_(SENT)
    ops.adamw_ema_step(p, gv, m, v, step, **hp, **kw)
    for t, f in zip((p, m, v, ema, pbf), first):
        _same(t, f, name)
    for b_ in (pb_, mb_, vb_, eb_, gb_, hb_):
        _guards_ok(b_, name)
    assert torch.equal(SB.bits(gv), SB.bits(g)), f"{name}: the gradient was written"
    ref = SB.adamw(p0, g, m0, v0, c)
    _note("adamw", SB.check_f32(f"{name} m", m, *ref["m"]))
    _note("adamw", SB.check_f32(f"{name} v", v, *ref["v"]))
    if dtype == F32:
        _note("adamw", SB.check_f32(f"{name} p", p, *ref["p"]))
    else:
        _note("adamw", SB.check_bf16(f"{name} p", p, *ref["p"], flat=True))
    if with_ema:                                               # chained on the stored new parameter
        if dtype == F32:
            _note("ema", SB.check_f32(f"{name} ema", ema, *SB.ema_f32(e0, p, c["omd"])))
        else:
            _note("ema", SB.check_bf16(f"{name} ema", ema, *SB.ema_bf16(e0, p, c["omd"]), flat=True))
    else:
        assert torch.equal(SB.bits(ema), SB.bits(e0))
    if dtype == F32 and with_pb:
        assert torch.equal(SB.bits(pbf), SB.bits(GB.to_bf16_rne(p))), f"{name}: p_bf16 is not one RNE of the stored parameter"
    else:
        assert bool((pbf == SENT).all())


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [3, 100003, 2097152 + 7])
def test_adamw_fp32(ops, n, step):
    """the n % 4 tail and (n > 2 097 152) a second grid-stride pass; with and without ema / p_bf16; weight decay 0 and 1e-2; grad_scale 0.5"""
    _adam_case(ops, n, F32, step, 1e-2, True, True, seed=n + step)
    _adam_case(ops, n, F32, step, 0.0, False, False, seed=n + step + 1)


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [8 * 4099, 4194304 + 8])
def test_adamw_bf16_parameters(ops, n, step):
    _adam_case(ops, n, BF16, step, 1e-2, True, False, seed=n + step)
    _adam_case(ops, n, BF16, step, 0.0, False, False, seed=n + step + 1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ema_update(ops, dtype):
    n, decay = 600001, 0.999
    g_ = _gen(6500)
    p = _randn(g_, n, scale=0.05, dtype=dtype)
    s0 = (p.float() + 1e-2 * torch.randn(n, device=dev(), generator=g_)).to(dtype)
    buf, s = _guarded(s0)
    ops.ema_update(s, p, decay)
    first = s.clone()
    s.copy_(s0)
    ops.ema_update(s, p, decay)
    _same(s, first, "ema_update")
    _guards_ok(buf, "ema_update")
    omd = float(np.float32(1.0) - np.float32(decay))
    if dtype == F32:
        _note("ema", SB.check_f32("ema_update fp32", s, *SB.ema_f32(s0, p, omd)))
    else:
        _note("ema", SB.check_bf16("ema_update bf16", s, *SB.ema_bf16(s0, p, omd), flat=True))


def test_adamw_bf16_sr_large_arena(ops):
    """one arena of 4 194 304 + 13 elements (a second grid-stride pass, an n % 8 tail) in three tensors whose boundaries fall inside a 16-byte group, injected
    draws: bit-equal to the oracle (fp32-alpha mode), tensor by tensor"""
    from oracle import train_math as TM

    n = 4194304 + 13
    ends = [1000003, 2500005, n]
    decs = [0.0, 7e-3, 3e-3]
    g_ = _gen(6600)
    mk = lambda s: _randn(g_, n, scale=s)
    p0, g, m0, v0, s0 = mk(0.5), mk(0.2), mk(0.05), (mk(0.05).float() ** 2).to(BF16), mk(1e-3)
    rb = torch.randint(0, 65536, (4, n), device=dev(), dtype=torch.int32, generator=g_)
    seg_end = torch.tensor(ends, dtype=torch.int64, device=dev())
    seg_decay = torch.tensor(decs, dtype=F32, device=dev())
    bufs = [_guarded(t) for t in (p0, m0, v0, s0)]
    views = [b[1] for b in bufs]
    ops.adamw_bf16_sr_step(views[0], g, views[1], views[2], views[3], 3, 1e-2, 0.9, 0.999, 1e-8, seg_end=seg_end, seg_decay=seg_decay, rand_bits=rb)
    first = [t.clone() for t in views]
    for t, t0 in zip(views, (p0, m0, v0, s0)):
        t.copy_(t0)
    ops.adamw_bf16_sr_step(views[0], g, views[1], views[2], views[3], 3, 1e-2, 0.9, 0.999, 1e-8, seg_end=seg_end, seg_decay=seg_decay, rand_bits=rb)
    for t, f in zip(views, first):
        _same(t, f, "adamw_bf16_sr_step")
    for b_ in bufs:
        _guards_ok(b_[0], "adamw_bf16_sr_step")
    got = [t.cpu() for t in views]
    cpu = [t.cpu() for t in (p0, g, m0, v0, s0)]
    rbc = rb.cpu()
    lo = 0
    for hi, dec in zip(ends, decs):
        o = TM.adamw_bf16_step(*[t[lo:hi] for t in cpu], 3, 1e-2, 0.9, 0.999, 1e-8, dec, [rbc[k, lo:hi] for k in range(4)])
        for x, y, what in zip(got, o, ("p", "exp_avg", "exp_avg_sq", "shift")):
            assert torch.equal(SB.bits(x[lo:hi]), SB.bits(y)), f"adamw_bf16_sr_step: {what} of the tensor [{lo}, {hi}) differs from the oracle"
        lo = hi


# ------------------------------------------------------------------------------------------------
# LoRA operand packer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [16, 128])
def test_lora_pack(ops, r):
    """r = 128: r (K + N) = 786 432 items, past the grid cap of 2048 x 256.  k2_off / n_off non-zero; all four packed operands bit-checked"""
    K = N = 3072
    K2, k2_off, N_total, n_off, scale = 256, 64 if r == 16 else 128, 3072 + 1024, 512, 0.37
    g = _gen(7000 + r)
    A = _randn(g, r, K, dtype=F32)
    Bm = _randn(g, N, r, dtype=F32)
    packed = [_randn(g, *shape, scale=3.0, shift=9.0) for shape in ((K2, K), (K, K2), (N_total, K2), (K2, N_total))]          # non-zero sentinels
    prior = [t.clone() for t in packed]
    ops.lora_pack(A, Bm, scale, *packed, k2_off=k2_off, n_off=n_off)
    first = [t.clone() for t in packed]
    ops.lora_pack(A, Bm, scale, *packed, k2_off=k2_off, n_off=n_off)
    for t, f in zip(packed, first):
        _same(t, f, "lora_pack")
    a_bf = GB.to_bf16_rne(A)
    b_bf = GB.to_bf16_rne(torch.tensor(scale, dtype=F32, device=dev()) * Bm)          # one RNE of the fp32 product
    want = [t.clone() for t in prior]
    want[0][k2_off:k2_off + r, :] = a_bf
    want[1][:, k2_off:k2_off + r] = a_bf.t()
    want[2][n_off:n_off + N, k2_off:k2_off + r] = b_bf
    want[3][k2_off:k2_off + r, n_off:n_off + N] = b_bf.t()
    for t, w, what in zip(packed, want, ("A_cat", "A_cat_T", "B_blk", "B_blk_T")):
        assert torch.equal(SB.bits(t), SB.bits(w)), f"lora_pack r={r}: {what} (the block, or an element outside it)"


# ------------------------------------------------------------------------------------------------
def test_every_skinny_route_was_hit():
    missing = ALL_ROUTES - HIT
    assert not missing, f"skinny routes never run by this module: {sorted(missing)}"
    assert HIT <= ALL_ROUTES, sorted(HIT - ALL_ROUTES)


def test_worst_ratios_report():
    print("\n| family | worst err/tol | worst block statistic |\n|---|---|---|")
    for fam, w in sorted(WORST.items()):
        print(f"| {fam} | {w['err/tol']:.3f} | {w['block']:.3f} |")

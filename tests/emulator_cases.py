"""One table of cases that holds BOTH sides of the CPU / GPU boundary to the kernels' own fp64 bounds: tests/ops_emulator.py on the CPU
(tests/test_ops_emulator_bounds_cpu.py) and simpletuner_amd.ops on the MI355X (tests/test_ops_emulator_bounds_gpu.py).

A case names a wrapper and builds, from a seeded CPU generator,
  * its operands, as views inside larger backing buffers (a padded leading dimension, an offset into the buffer and a guard tail after the last row), so the
    device and the emulator see identical stored bits, strides and offsets (`Twin` re-creates a view on a device copy of its backing buffer with as_strided);
  * `call(mod, T)`: the call itself on module `mod` (the emulator or ops), every tensor passed through T (identity on the CPU, the device twin on the GPU);
  * `outs`: label -> the view the call OWNS (everything else in every backing buffer must keep its bits), `ret(r)`: label -> tensors the call returns fresh,
    `same`: the label of the view the call must hand back as the very object it was given;
  * `ref(o)`: per stored output (label, want, e, kind[, extra]) from the family's fp64 functions (tests/{gemm,attn,norm,conv,step,ew}_bounds.py) with the route
    parameters the device takes at that shape.  `o` holds the outputs as stored, for the chained references (an output the kernel computes from another stored
    output is judged against fp64 of that stored value, as the family tests do).

Kinds: "bf16" one RNE of an fp32 value, |out - want| <= 1/2 ulp_bf16(|want| + e) + e (on the GPU with the family's 64 x 64 block RMS); "bf16e" the same without
a block statistic (short vectors, lattice outputs, edge vectors); "bf16x2" a twice-rounded output (one more ulp); "f32s" an fp32 sum, |out - want| <= e + u |want|
(on the GPU with the 64-column block statistic); "f32" the same, element-wise only; "lse2"; "attn" (extra: the model variance, the map to [B, H, S, d]); "geglu"
(extra: the gate, for ew_bounds.check_geglu's block statistic); "edge" (ew_bounds' edge vector: extra x); "exact": bit equality with `want`; "zero": a grid's
border and tail rows, zero of either sign.

References this module adds for wrappers without a family function follow the same rules: fp64 of the stored inputs, u = 2^-24 per fp32 rounding counted from
the kernel's source, half a bf16 ulp per store.  No figure is fitted to an output.  Shapes are the smallest that reach each argument form."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import attn_bounds as AB
from tests import conv_bounds as CB
from tests import ew_bounds as EB
from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests import step_bounds as SB

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
OFF = 64           # elements before the first row of every view (128 / 256 bytes: keeps the 16-byte alignment the C entries require)
GUARD = 192        # elements after the last row


# ---- backing buffers and their twins --------------------------------------------------------------------------------------------------------------------
class Gen:
    """seeded operand factory; remembers every backing buffer it made (the guard check walks them)"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.backs = []

    def _back(self, n, dtype, scale, shift):
        if dtype == I32:
            b = torch.randint(-7, 7, (n,), generator=self.g, dtype=I32)
        else:
            b = (torch.randn(n, generator=self.g) * scale + shift).to(dtype)
        self.backs.append(b)
        return b

    def mat(self, rows, cols, dtype=BF16, pad=24, scale=1.0, shift=0.0):
        """[rows, cols] with leading dimension cols + pad inside a guarded buffer"""
        ld = cols + pad
        b = self._back(OFF + rows * ld + GUARD, dtype, scale, shift)
        return torch.as_strided(b, (rows, cols), (ld, 1), OFF)

    def blk(self, *shape, dtype=BF16, scale=1.0, shift=0.0):
        """a contiguous tensor of `shape` inside a guarded buffer"""
        n = int(np.prod(shape))
        b = self._back(OFF + n + GUARD, dtype, scale, shift)
        return b[OFF:OFF + n].view(*shape)

    def seg(self, segs, rows, cols, gap_rows, dtype=BF16, pad=24, scale=1.0):
        """[segs, rows, cols] row blocks `gap_rows` apart (the segmented operand form)"""
        ld = cols + pad
        b = self._back(OFF + segs * (rows + gap_rows) * ld + GUARD, dtype, scale, 0.0)
        return torch.as_strided(b, (segs, rows, cols), ((rows + gap_rows) * ld, ld, 1), OFF)


class Twin:
    """host view -> the same view (shape, strides, offset) of a device copy of its backing buffer; identity on the CPU"""

    def __init__(self, device=None):
        self.device = device
        self.backs = {}          # host storage pointer -> device flat buffer
        self.memo = {}           # id(host view) -> device view (the SAME object for the same host view: `same` is an identity check)

    def back(self, t):
        key = (t.untyped_storage().data_ptr(), t.dtype)
        if key not in self.backs:
            flat = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
            self.backs[key] = flat.to(self.device)
        return self.backs[key]

    def __call__(self, t):
        if t is None or self.device is None or not torch.is_tensor(t):
            return t
        if id(t) not in self.memo:
            self.memo[id(t)] = (t, torch.as_strided(self.back(t), tuple(t.shape), t.stride(), t.storage_offset()))
        return self.memo[id(t)][1]


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@dataclass
class Built:
    call: object
    ref: object
    gen: Gen
    outs: dict = field(default_factory=dict)
    ret: object = None
    same: str = None
    steps: int = 1            # > 1: `call(mod, T, step)` runs that often (the optimizer cases)


@dataclass
class Case:
    name: str
    wrapper: str
    family: str
    build: object
    opts: frozenset            # the optional arguments this case passes (the coverage gate needs each of a wrapper's at least once)


@dataclass
class Ran:
    out: dict                  # label -> stored output on the CPU
    guard_ok: bool
    guard_msg: str
    same_ok: bool


def _owned_masks(b: Built):
    """per backing buffer: True where some owned view lives"""
    masks = {}
    for back in b.gen.backs:
        masks[(back.untyped_storage().data_ptr(), back.dtype)] = torch.zeros(back.numel(), dtype=torch.bool)
    for v in b.outs.values():
        key = (v.untyped_storage().data_ptr(), v.dtype)
        assert key in masks, "an owned view must live in one of the case's backing buffers"
        idx = torch.as_strided(torch.arange(masks[key].numel()), tuple(v.shape), v.stride(), v.storage_offset())
        masks[key][idx.reshape(-1)] = True
    return masks


def run(case: Case, mod, device=None):
    """build the case afresh, run it on `mod`: (the stored outputs and the guard / identity verdicts, the Built whose ref judges them)"""
    b = case.build()
    T = Twin(device)
    for back in b.gen.backs:                   # every buffer travels, used or not: the guard check covers the inputs too
        T.back(back) if device is not None else None
    before = {k: (T.backs[k].clone() if device is not None else None) for k in T.backs}
    host_before = [x.clone() for x in b.gen.backs] if device is None else None
    r = None
    for step in range(1, b.steps + 1):
        r = b.call(mod, T, step) if b.steps > 1 else b.call(mod, T)
    if device is not None:
        torch.cuda.synchronize()
    masks = _owned_masks(b)
    ok, msg = True, ""
    for i, back in enumerate(b.gen.backs):
        key = (back.untyped_storage().data_ptr(), back.dtype)
        now = T.backs[key].cpu() if device is not None else back
        was = before[key].cpu() if device is not None else host_before[i]
        bad = (bits(now) != bits(was)) & ~masks[key]
        if bool(bad.any()):
            ok = False
            msg += f"buffer {i}: {int(bad.sum())} elements outside the owned region changed, first at flat index {int(bad.nonzero()[0])}; "
    out = {k: T(v).detach().cpu().clone() for k, v in b.outs.items()}
    if b.ret is not None:
        out.update({k: v.detach().cpu().clone() for k, v in b.ret(r).items() if v is not None})
    same_ok = True
    if b.same is not None:
        same_ok = r is T(b.outs[b.same]) if not isinstance(b.same, tuple) else all(x is T(b.outs[s]) for x, s in zip(r, b.same) if s is not None)
    return Ran(out, ok, msg, same_ok), b


# ---- the element rule every family shares -------------------------------------------------------------------------------------------------------------------
def elem_tol(out, want, e, kind, extra=None):
    """the element tolerance of one stored output under its kind's rule (fp64, out's shape); the families' checkers reduce to this per element"""
    w, ee = want.to(F64).reshape(out.shape), e.to(F64).reshape(out.shape)
    if kind in ("bf16", "bf16e", "bf16x2", "attn", "geglu", "edge"):
        assert out.dtype == BF16 or (extra and "out" in extra), out.dtype          # extra["out"]: a derived quantity (O + O_res), not a stored tensor
        fr = w if not (extra and "final" in extra) else extra["final"].to(F64).reshape(out.shape)
        return (1.5 if kind == "bf16x2" else 0.5) * GB.ulp_bf16(fr.abs() + ee) + ee
    assert kind in ("f32", "f32s", "lse2") and out.dtype == F32, (kind, out.dtype)
    return ee + U * w.abs() + 1e-300


def elem_ratio(out, want, e, kind, extra=None):
    """worst |err| / tol of one stored output under its kind's element rule; the exact kinds give 0.0 or inf"""
    if kind == "exact":
        assert out.dtype == want.dtype and out.shape == want.shape, (out.dtype, want.dtype, tuple(out.shape), tuple(want.shape))
        return 0.0 if torch.equal(bits(out), bits(want)) else math.inf
    if kind == "zero":            # a grid's border and tail rows: zero of either sign (conv_bounds.check_grid_sum)
        return 0.0 if not bool((bits(out) & 0x7FFF).any()) else math.inf
    o = out.to(F64)
    ratio = (o - want.to(F64).reshape(out.shape)).abs() / elem_tol(out, want, e, kind, extra)
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, math.inf))
    if kind == "edge":            # ew_bounds' edge vector: finite, right sign, never above the rounded reference; x >= 80 the reference's bits; |x| <= 80 the main bound
        x = extra["x"]
        if not (bool(EB.edge_ok(out, want).all()) and bool(EB.edge_exact(x, out, want).all())):
            return math.inf
        return float(ratio[x.float().abs() <= 80].max())
    return float(ratio.max())


CASES = []


def case(wrapper, family, name=None, opts=()):
    def deco(fn):
        CASES.append(Case(name or fn.__name__.lstrip("_"), wrapper, family, fn, frozenset(opts)))
        return fn
    return deco


# =============================================================================================================================================================
# GEMM family: M 320 (one full 256-row tile and a ragged one), N 136, K 192
# =============================================================================================================================================================
def _lib():
    from simpletuner_amd import lib
    return lib


GM, GN, GK = 320, 136, 192


def _batch_rows(t, M, rpb):
    return t[torch.arange(M) // rpb]


def _gemm(seed, epi, N=GN, aux_out=False, rpb=0, seg2=False, bias=True, plain_out=False):
    """one NT GEMM case: `out=` a strided view unless plain_out (the wrapper allocates); seg2: the second K segment, 16 adapter columns in a 64-column granule"""
    def build():
        L = _lib()
        g = Gen(seed)
        a, w = g.mat(GM, GK), g.mat(N, GK, scale=0.06)
        kw = dict(epilogue=getattr(L, epi))
        if bias:
            kw["bias"] = g.blk(N, scale=0.1)
        A2 = B2 = None
        if seg2:
            A2, B2 = g.mat(GM, 64, pad=8), g.mat(N, 64, pad=40, scale=0.1)
            A2[:, 16:] = 0                      # K2_real = 16: the rest of the granule is zero padding (st355.h)
            B2[:, 16:] = 0
            kw.update(a2=A2, b2=B2, k2_real=16)
        n_out = N // 2 if epi == "EPI_GEGLU" else 2 * N if epi == "EPI_GEGLU_GRAD" else N
        outs = {}
        if not plain_out:
            kw["out"] = outs["out"] = g.mat(GM, n_out, pad=40)
        if epi in ("EPI_ADD", "EPI_MUL_GELU_GRAD", "EPI_GATE_RESIDUAL"):
            kw["aux_in"] = g.mat(GM, N, pad=16)
        if epi == "EPI_GEGLU_GRAD":
            kw["aux_in"] = g.mat(GM, 2 * N, pad=16)
        if epi == "EPI_GATE_RESIDUAL":
            kw["gate"] = g.mat(GM // rpb, N, pad=6 * N - N, scale=0.5)          # a column block of a [B, 6 N] modulation table
            kw["rows_per_batch"] = rpb
        if aux_out:
            kw["aux_out"] = outs["aux_out"] = g.mat(GM, N, pad=8)

        def call(mod, T):
            return mod.gemm(T(a), T(w), **{k: T(v) for k, v in kw.items()})

        def ref(o):
            acc = GB.gemm_ref(a, w, A2, B2, kw.get("bias"))
            res = []
            if aux_out:
                res.append(("aux_out", *GB.epi_none(acc), "bf16"))
            if epi == "EPI_NONE":
                res.append(("out", *GB.epi_none(acc), "bf16"))
            elif epi == "EPI_ADD":
                res.append(("out", *GB.epi_add(acc, kw["aux_in"]), "bf16"))
            elif epi == "EPI_GELU":
                res.append(("out", *(GB.epi_gelu_of_stored(o["aux_out"]) if aux_out else GB.epi_gelu(acc)), "bf16"))
            elif epi == "EPI_MUL_GELU_GRAD":
                res.append(("out", *GB.epi_mul_gelu_grad(acc, kw["aux_in"]), "bf16"))
            elif epi == "EPI_GATE_RESIDUAL":
                res.append(("out", *GB.epi_gate_residual(acc, kw["aux_in"], _batch_rows(kw["gate"], GM, rpb)), "bf16"))
            elif epi == "EPI_GEGLU":
                res.append(("out", *GB.epi_geglu_of_stored(o["aux_out"]), "bf16"))
            elif epi == "EPI_GEGLU_GRAD":
                res.append(("out", *GB.epi_geglu_grad(acc, kw["aux_in"]), "bf16x2"))
            return res

        return Built(call, ref, g, outs, ret=(lambda r: {"out": r}) if plain_out else None, same=None if plain_out else "out")
    return build


for _i, (_nm, _kw, _opts) in enumerate([
        ("gemm_none", dict(epi="EPI_NONE"), ("bias", "out", "epilogue")),
        ("gemm_none_alloc", dict(epi="EPI_NONE", plain_out=True, bias=False), ("epilogue",)),
        ("gemm_none_k2", dict(epi="EPI_NONE", seg2=True), ("a2", "b2", "k2_real")),
        ("gemm_add", dict(epi="EPI_ADD"), ("aux_in",)),
        ("gemm_gelu", dict(epi="EPI_GELU"), ()),
        ("gemm_gelu_aux", dict(epi="EPI_GELU", aux_out=True), ("aux_out",)),
        ("gemm_mul_gelu_grad", dict(epi="EPI_MUL_GELU_GRAD", bias=False), ()),
        ("gemm_gate_residual_rpb160", dict(epi="EPI_GATE_RESIDUAL", rpb=160, aux_out=True, seg2=True), ("gate", "rows_per_batch")),
        ("gemm_gate_residual_rpb1", dict(epi="EPI_GATE_RESIDUAL", rpb=1), ("gate", "rows_per_batch")),
        # the GEGLU epilogues require N % 64 == 0 (gemm.hip: "the GEGLU epilogues take a plain problem with N %% 64 == 0"): N 128 here, not 136
        ("gemm_geglu", dict(epi="EPI_GEGLU", N=128, aux_out=True), ("aux_out",)),
        ("gemm_geglu_grad", dict(epi="EPI_GEGLU_GRAD", N=64, bias=False), ("aux_in",))]):
    CASES.append(Case(_nm, "gemm", "gemm", _gemm(1000 + _i, **_kw), frozenset(_opts)))


@case("gemm", "gemm", opts=("heads",))
def _gemm_heads():
    """EPI_HEADS: q | k | v parts of H = 2 heads of 64 columns; rows_per_batch 160 at pos0 32 of S = 192 (the epilogue's preconditions fix N = 384)"""
    L = _lib()
    g = Gen(1100)
    B, H, S, R, p0 = 2, 2, 192, 160, 32
    a, w, bias = g.mat(GM, GK), g.mat(3 * H * 64, GK, scale=0.06), g.blk(3 * H * 64, scale=0.1)
    Q, K, Vt = g.blk(B, H, S, 64), g.blk(B, H, S, 64), g.blk(B, H, 64, S)
    out = g.mat(GM, H * 64, pad=8)
    outs = {"Q": Q[:, :, p0:p0 + R], "K": K[:, :, p0:p0 + R], "Vt": Vt[..., p0:p0 + R], "out": out}

    def call(mod, T):
        return mod.gemm(T(a), T(w), bias=T(bias), out=T(out), epilogue=L.EPI_HEADS, rows_per_batch=R, heads=mod.heads(T(Q), T(K), T(Vt), H, S, p0, H * 64, H * 64))

    def ref(o):
        acc = GB.gemm_ref(a, w, None, None, bias)
        hm = lambda t, j: t[:, j * H * 64:(j + 1) * H * 64].reshape(B, R, H, 64)
        res = []
        for j, nm in ((0, "Q"), (1, "K")):
            res.append((nm, hm(acc.ref, j).permute(0, 2, 1, 3), hm(acc.s, j).permute(0, 2, 1, 3), "bf16"))
        res.append(("Vt", hm(acc.ref, 2).permute(0, 2, 3, 1), hm(acc.s, 2).permute(0, 2, 3, 1), "bf16"))
        res.append(("out", acc.ref[:, 2 * H * 64:], acc.s[:, 2 * H * 64:], "bf16"))
        return res

    return Built(call, ref, g, outs, same="out")


@case("heads", "gemm")
def _heads_struct():
    """ops.heads alone builds the epilogue's destination struct; what it does is pinned through gemm_heads (same name on both sides, one call)"""
    return _gemm_heads()


@case("gemm_grouped", "gemm")
def _gemm_grouped():
    """two problems of one epilogue kind (gemm.hip: "all problems must share one epilogue kind") and different shapes in one launch"""
    L = _lib()
    g = Gen(1200)
    a1, w1, b1, o1 = g.mat(GM, GK), g.mat(GN, GK, scale=0.06), g.blk(GN, scale=0.1), g.mat(GM, GN, pad=8)
    a2, w2, x2, o2 = g.mat(96, 64), g.mat(72, 64, scale=0.1), g.mat(96, 72, pad=8), g.mat(96, 72, pad=16)
    r1, r2 = g.mat(GM, GN, pad=8), None

    def call(mod, T):
        return mod.gemm_grouped([dict(a=T(a1), w=T(w1), bias=T(b1), out=T(o1), epilogue=L.EPI_ADD, aux_in=T(r1)),
                                 dict(a=T(a2), w=T(w2), out=T(o2), epilogue=L.EPI_ADD, aux_in=T(x2))])

    def ref(o):
        return [("o1", *GB.epi_add(GB.gemm_ref(a1, w1, None, None, b1), r1), "bf16"), ("o2", *GB.epi_add(GB.gemm_ref(a2, w2), x2), "bf16")]

    return Built(call, ref, g, {"o1": o1, "o2": o2}, same=("o1", "o2"))


TN_M, TN_P, TN_Q = 256, 136, 72


def _gemm_tn(seed, accumulate=False, segmented=False, alloc=False):
    def build():
        g = Gen(seed)
        if segmented:                                   # 2 segments of 128 rows, 24 rows of other data between them
            Lm, R = g.seg(2, 128, TN_P, 24), g.seg(2, 128, TN_Q, 24, pad=8, scale=1 / 16)
        else:
            Lm, R = g.mat(TN_M, TN_P), g.mat(TN_M, TN_Q, pad=8, scale=1 / 16)
        out = None if alloc else g.mat(TN_P, TN_Q, pad=8)
        prior = None if alloc else out.clone()

        def call(mod, T):
            return mod.gemm_tn(T(Lm), T(R)) if alloc else mod.gemm_tn(T(Lm), T(R), out=T(out), accumulate=accumulate)

        def ref(o):
            acc = GB.gemm_ref(Lm.reshape(-1, TN_P).t(), R.reshape(-1, TN_Q).t())
            return [("out", *(GB.epi_add(acc, prior) if accumulate else GB.epi_none(acc)), "bf16")]

        return Built(call, ref, g, {} if alloc else {"out": out}, ret=(lambda r: {"out": r}) if alloc else None, same=None if alloc else "out")
    return build


CASES.append(Case("gemm_tn_alloc", "gemm_tn", "gemm", _gemm_tn(1300, alloc=True), frozenset()))
CASES.append(Case("gemm_tn_accumulate", "gemm_tn", "gemm", _gemm_tn(1301, accumulate=True), frozenset(("out", "accumulate"))))
CASES.append(Case("gemm_tn_segmented", "gemm_tn", "gemm", _gemm_tn(1302, segmented=True), frozenset(("out",))))


@case("transpose", "gemm", opts=("out",))
def _transpose():
    g = Gen(1400)
    src, out = g.mat(72, 136), g.mat(136, 72, pad=8)
    return Built(lambda mod, T: mod.transpose(T(src), out=T(out)), lambda o: [("out", src.t().contiguous(), None, "exact")], g, {"out": out}, same="out")


@case("transpose", "gemm", name="transpose_alloc")
def _transpose_alloc():
    g = Gen(1401)
    src = g.mat(72, 136)
    return Built(lambda mod, T: mod.transpose(T(src)), lambda o: [("out", src.t().contiguous(), None, "exact")], g, ret=lambda r: {"out": r})


def _scale_cols(seed, rpb, alloc=False):
    """a bf16 x bf16 product is exact in fp32, so the single store rounding makes the output a bit-exact function of the operands"""
    def build():
        g = Gen(seed)
        M, N = 72, 136
        x, gate = g.mat(M, N), g.mat(M // rpb, N, pad=5 * N, scale=0.5)
        out = None if alloc else g.mat(M, N, pad=8)
        want = (x.double() * _batch_rows(gate, M, rpb).double()).float().to(BF16)
        call = (lambda mod, T: mod.scale_cols(T(x), T(gate), rpb)) if alloc else (lambda mod, T: mod.scale_cols(T(x), T(gate), rpb, out=T(out)))
        return Built(call, lambda o: [("out", want, None, "exact")], g, {} if alloc else {"out": out}, ret=(lambda r: {"out": r}) if alloc else None,
                     same=None if alloc else "out")
    return build


CASES.append(Case("scale_cols_rpb36", "scale_cols", "gemm", _scale_cols(1500, 36), frozenset(("out",))))
CASES.append(Case("scale_cols_rpb1_alloc", "scale_cols", "gemm", _scale_cols(1501, 1, alloc=True), frozenset()))


# =============================================================================================================================================================
# elementwise: 72 x 136 strided views; the activations also on ew_bounds' edge vector
# =============================================================================================================================================================
EW_M, EW_N = 72, 136
_ACT_REF = {"silu": lambda a, b: EB.silu(a), "gelu_tanh": lambda a, b: EB.gelu_tanh(a), "silu_bwd": EB.silu_bwd, "add": EB.add}


def _act(seed, op, edge=False):
    def build():
        g = Gen(seed)
        if edge:                               # ew_bounds.edge_vector inside a guarded buffer; the second operand as tests/test_ew_bounds_gpu.py takes it
            a = g.blk(12)
            a.copy_(EB.edge_vector())
            b = g.blk(12)
            b.copy_((-0.5 * a.float()).to(BF16) if op == "add" else torch.full_like(a, 0.75))
        else:
            a, b = g.mat(EW_M, EW_N, scale=2.0), g.mat(EW_M, EW_N, pad=8)
        two = op in ("silu_bwd", "add")
        call = (lambda mod, T: getattr(mod, op)(T(a), T(b))) if two else (lambda mod, T: getattr(mod, op)(T(a)))

        def ref(o):
            want, e = _ACT_REF[op](a, b)
            return [("y", want, e, "edge", {"x": a})] if edge else [("y", want, e, "bf16")]

        return Built(call, ref, g, ret=lambda r: {"y": r})
    return build


for _i, _op in enumerate(("silu", "silu_bwd", "gelu_tanh", "add")):
    CASES.append(Case(_op, _op, "elementwise", _act(2000 + _i, _op), frozenset()))
    CASES.append(Case(_op + "_edges", _op, "elementwise", _act(2010 + _i, _op, edge=True), frozenset()))


def _geglu(seed, bwd):
    def build():
        g = Gen(seed)
        F_ = EW_N // 2 + 60                  # 128 features: h [72, 256] strided
        h, dout = g.mat(EW_M, 2 * F_, scale=1.5), g.mat(EW_M, F_, pad=8)
        if bwd:
            return Built(lambda mod, T: mod.geglu_bwd(T(h), T(dout)), lambda o: [("dh", *EB.geglu_bwd(h, dout, F_), "geglu", {"gate": h[:, F_:]})], g, ret=lambda r: {"dh": r})
        return Built(lambda mod, T: mod.geglu_fwd(T(h)), lambda o: [("y", *EB.geglu_fwd(h, F_), "geglu", {"gate": h[:, F_:]})], g, ret=lambda r: {"y": r})
    return build


CASES.append(Case("geglu_fwd", "geglu_fwd", "elementwise", _geglu(2020, False), frozenset()))
CASES.append(Case("geglu_bwd", "geglu_bwd", "elementwise", _geglu(2021, True), frozenset()))


def _softmax(seed, n, bwd=False, scale=0.7):
    """n 264: one 2048-column chunk; n 2056: two (k_softmax_rows<2>)"""
    def build():
        g = Gen(seed)
        rows = 5
        x = g.mat(rows, n, pad=64, scale=3.0)
        if not bwd:
            x0 = x.clone()
            return Built(lambda mod, T: mod.softmax_rows_(T(x), scale=scale), lambda o: [("x", *EB.softmax_rows(x0, scale), "bf16")], g, {"x": x}, same="x")
        p, dp = g.mat(rows, n, pad=64), x
        p.copy_(torch.softmax(p.float() * 3.0 * 0.7, 1).to(BF16))          # a real softmax output as stored in bf16
        dp0 = dp.clone()
        return Built(lambda mod, T: mod.softmax_rows_bwd_(T(p), T(dp), scale=0.125), lambda o: [("dp", *EB.softmax_rows_bwd(p, dp0, 0.125), "bf16")], g, {"dp": dp},
                     same="dp")
    return build


for _n in (264, 2056):
    CASES.append(Case(f"softmax_rows_n{_n}", "softmax_rows_", "elementwise", _softmax(2030 + _n, _n), frozenset(("scale",))))
    CASES.append(Case(f"softmax_rows_bwd_n{_n}", "softmax_rows_bwd_", "elementwise", _softmax(2040 + _n, _n, bwd=True), frozenset(("scale",))))


def _timestep(seed, dim, ts, scale):
    def build():
        g = Gen(seed)
        t = g.blk(len(ts), dtype=F32)
        t.copy_(torch.tensor(ts, dtype=F32))
        return Built(lambda mod, T: mod.timestep_proj(T(t), dim, scale=scale), lambda o: [("y", *EB.timestep_proj(t, dim, scale), "bf16")], g, ret=lambda r: {"y": r})
    return build


CASES.append(Case("timestep_proj_256", "timestep_proj", "elementwise", _timestep(2050, 256, [0.0, 1e-4, 0.1234, 0.5, 1.0], 1000.0), frozenset(("scale",))))
CASES.append(Case("timestep_proj_320", "timestep_proj", "elementwise", _timestep(2051, 320, [0.0, 1.0, 37.0, 500.5, 999.0, 1000.0], 1.0), frozenset()))


# =============================================================================================================================================================
# copies and layout passes: bit equality with an expectation indexed independently of the emulator
# =============================================================================================================================================================
def _patch_expect(x, order):
    B, C, H, W = x.shape
    out = torch.zeros(B, (H // 2) * (W // 2), 4 * C, dtype=x.dtype)
    v = out.view(B, H // 2, W // 2, C, 2, 2) if order == 0 else out.view(B, H // 2, W // 2, 2, 2, C)
    for dh in range(2):
        for dw in range(2):
            src = x[:, :, dh::2, dw::2].permute(0, 2, 3, 1)
            if order == 0:
                v[..., dh, dw] = src
            else:
                v[:, :, :, dh, dw, :] = src
    return out


def _patch(seed, op, order):
    def build():
        g = Gen(seed)
        B, C, H, W = 2, 16, 6, 10
        x = g.blk(B, C, H, W)
        packed = g.blk(B, (H // 2) * (W // 2), 4 * C)
        ex = lambda want: (lambda o: [("y", want, None, "exact")])
        kw = {} if op.startswith("flux") else {"order": order}
        if op in ("patchify", "flux_pack"):
            return Built(lambda mod, T: getattr(mod, op)(T(x), **kw), ex(_patch_expect(x, order)), g, ret=lambda r: {"y": r})
        want = torch.zeros(B, C, H, W, dtype=BF16)
        # the inverse: the expectation is the tensor whose patchify is `packed`
        idx = _patch_expect(torch.arange(B * C * H * W, dtype=torch.float32).view(B, C, H, W), order).long().reshape(-1)
        want.view(-1)[idx] = packed.reshape(-1)
        return Built(lambda mod, T: getattr(mod, op)(T(packed), C, H, W, **kw), ex(want), g, ret=lambda r: {"y": r})
    return build


for _i, (_op, _order) in enumerate((("patchify", 0), ("patchify", 1), ("unpatchify", 0), ("unpatchify", 1), ("flux_pack", 0), ("flux_unpack", 0))):
    CASES.append(Case(f"{_op}_order{_order}", _op, "copies", _patch(2100 + _i, _op, _order), frozenset(("order",)) if _op.endswith("patchify") else frozenset()))


def _route_idx(g, B, S, K):
    idx = g.blk(B, K, dtype=I32)
    for b in range(B):
        idx[b] = torch.randperm(S, generator=g.g)[:K].to(I32)
    return idx


@case("gather_rows", "copies", opts=("out",))
def _gather_rows():
    g = Gen(2200)
    B, S, K, D = 2, 40, 17, 136
    x = torch.as_strided(g.mat(B * S, D), (B, S, D), (S * (D + 24), D + 24, 1), OFF)
    idx = _route_idx(g, B, S, K)
    ob = g.mat(B * K, D, pad=8)
    out = torch.as_strided(ob, (B, K, D), (K * (D + 8), D + 8, 1), OFF)
    want = torch.stack([x[b][idx[b].long()] for b in range(B)])
    return Built(lambda mod, T: mod.gather_rows(T(x), T(idx), out=T(out)), lambda o: [("out", want, None, "exact")], g, {"out": out}, same="out")


@case("gather_rows", "copies", name="gather_rows_alloc")
def _gather_rows_alloc():
    g = Gen(2201)
    B, S, K, D = 2, 40, 17, 136
    x = torch.as_strided(g.mat(B * S, D), (B, S, D), (S * (D + 24), D + 24, 1), OFF)
    idx = _route_idx(g, B, S, K)
    want = torch.stack([x[b][idx[b].long()] for b in range(B)])
    return Built(lambda mod, T: mod.gather_rows(T(x), T(idx)), lambda o: [("out", want, None, "exact")], g, ret=lambda r: {"out": r})


@case("scatter_rows", "copies")
def _scatter_rows():
    """dst rows named by idx are owned; every other row of dst keeps its bits"""
    g = Gen(2210)
    B, S, K, D = 2, 40, 17, 136
    src = torch.as_strided(g.mat(B * K, D, pad=8), (B, K, D), (K * (D + 8), D + 8, 1), OFF)
    dst = torch.as_strided(g.mat(B * S, D), (B, S, D), (S * (D + 24), D + 24, 1), OFF)
    idx = _route_idx(g, B, S, K)
    want = dst.clone()
    for b in range(B):
        want[b][idx[b].long()] = src[b]
    outs = {f"row{b}_{j}": dst[b, int(idx[b, j])] for b in range(B) for j in range(K)}

    def ref(o):
        return [(f"row{b}_{j}", src[b, j], None, "exact") for b in range(B) for j in range(K)]

    return Built(lambda mod, T: mod.scatter_rows(T(src), T(idx), T(dst)), ref, g, outs)


def _head_split(seed, d, d_src, want_x=True, want_xt=True):
    def build():
        g = Gen(seed)
        B, H, S = 2, 2, 77
        ds = d if d_src is None else d_src
        src = g.mat(B * S, H * ds, pad=40)
        Sp = (S + 63) // 64 * 64
        X = torch.zeros(B, H, S, d, dtype=BF16)
        X[..., :ds] = torch.stack([src[b * S:(b + 1) * S].view(S, H, ds).transpose(0, 1) for b in range(B)])
        Xt = torch.zeros(B, H, d, Sp, dtype=BF16)
        Xt[..., :S] = X.transpose(-1, -2)

        def ref(o):
            return ([("X", X, None, "exact")] if want_x else []) + ([("Xt", Xt, None, "exact")] if want_xt else [])

        def ret(r):
            assert r[2] == Sp and (r[0] is None) == (not want_x) and (r[1] is None) == (not want_xt)
            return {"X": r[0], "Xt": r[1]}

        return Built(lambda mod, T: mod.head_split(T(src), B, H, d, S, want_x=want_x, want_xt=want_xt, d_src=d_src), ref, g, ret=ret)
    return build


CASES.append(Case("head_split_d64", "head_split", "copies", _head_split(2300, 64, None), frozenset()))
CASES.append(Case("head_split_d128_src72", "head_split", "copies", _head_split(2301, 128, 72), frozenset(("d_src",))))
CASES.append(Case("head_split_x_only", "head_split", "copies", _head_split(2302, 64, None, want_xt=False), frozenset(("want_xt",))))
CASES.append(Case("head_split_xt_only", "head_split", "copies", _head_split(2303, 64, None, want_x=False), frozenset(("want_x",))))


def _head_merge(seed, d, d_src):
    def build():
        g = Gen(seed)
        B, H, S = 2, 2, 77
        ds = d if d_src is None else d_src
        dX = g.blk(B, H, S, d)
        buf = g.mat(B * S, H * ds + 16, pad=24)
        dst = buf[:, 8:8 + H * ds]                  # a column block of a wider buffer: the columns beside it keep their bits
        want = dX[..., :ds].permute(0, 2, 1, 3).reshape(B * S, H * ds).contiguous()
        return Built(lambda mod, T: mod.head_merge(T(dX), T(dst), B, H, d, S, d_src=d_src), lambda o: [("dst", want, None, "exact")], g, {"dst": dst}, same="dst")
    return build


CASES.append(Case("head_merge_d64", "head_merge", "copies", _head_merge(2310, 64, None), frozenset()))
CASES.append(Case("head_merge_d128_src72", "head_merge", "copies", _head_merge(2311, 128, 72), frozenset(("d_src",))))


# =============================================================================================================================================================
# LayerNorm (+ modulation) and the token-axis sums: D 264 (rows 96, 48 per batch) and D 3072, the _stats limit (rows 8, 1 per batch)
# =============================================================================================================================================================
def ln_nc(D):            # norm_route.h ln_route_nc
    return 1 if D <= 512 else 2 if D <= 1024 else 3 if D <= 1536 else 4 if D <= 2048 else 6 if D <= 3072 else 8


def ln_stats_nc(D):      # norm_route.h ln_stats_route_nc
    return 1 if D <= 512 else 2 if D <= 1024 else 3 if D <= 1536 else 4 if D <= 2048 else 6


def lnp_nc(D):           # norm_route.h lnp_route_nc
    return 1 if D <= 512 else 2 if D <= 1024 else 3 if D <= 1536 else 4


LN_SHAPES = ((264, 96, 48), (3072, 8, 1))


def _mod(g, nb, D, k, scale=0.3):
    """column block k of a [nb, 6 D] modulation table"""
    return g.mat(nb, 6 * D, pad=8, scale=scale)[:, k * D:(k + 1) * D]


def _ln_fwd(seed, D, rows, rpb, alloc=False, xhat=False):
    def build():
        g = Gen(seed)
        nb = rows // rpb
        x = g.mat(rows, D, scale=1.3, shift=0.4)
        scale, shift = _mod(g, nb, D, 1), _mod(g, nb, D, 0)
        out = None if alloc else g.mat(rows, D, pad=40)
        kw = {} if alloc else {"out": out}
        if xhat:
            call = lambda mod, T: mod.layer_norm_xhat(T(x), eps=1e-6, **{k: T(v) for k, v in kw.items()})
        else:
            call = lambda mod, T: mod.ln_modulate_fwd(T(x), T(scale), T(shift), rpb, eps=1e-6, **{k: T(v) for k, v in kw.items()})

        def ref(o):
            xd = x.double()
            st = NB.ln_stats(xd, 1e-6, NB.L_ln(ln_nc(D)))
            b = torch.arange(rows) // rpb
            a, bb = (torch.ones_like(xd), torch.zeros_like(xd)) if xhat else (1 + scale.double()[b], shift.double()[b])
            want, e, _, _ = NB.norm_fwd(xd, st, a, bb)
            return [("y", want, e, "bf16")]

        return Built(call, ref, g, {} if alloc else {"y": out}, ret=(lambda r: {"y": r}) if alloc else None, same=None if alloc else "y")
    return build


for _i, (_D, _rows, _rpb) in enumerate(LN_SHAPES):
    CASES.append(Case(f"ln_modulate_fwd_D{_D}", "ln_modulate_fwd", "norm", _ln_fwd(3000 + _i, _D, _rows, _rpb), frozenset(("out", "eps"))))
    CASES.append(Case(f"layer_norm_xhat_D{_D}", "layer_norm_xhat", "norm", _ln_fwd(3010 + _i, _D, _rows, _rpb, xhat=True), frozenset(("out", "eps"))))
CASES.append(Case("ln_modulate_fwd_alloc", "ln_modulate_fwd", "norm", _ln_fwd(3020, 264, 96, 48, alloc=True), frozenset()))
CASES.append(Case("layer_norm_xhat_alloc", "layer_norm_xhat", "norm", _ln_fwd(3021, 264, 96, 48, alloc=True, xhat=True), frozenset()))


def _ln_bwd(seed, D, rows, rpb, dres, gated, out, stats=None):
    """ln_modulate_bwd, or ln_modulate_bwd_stats with stats = the set of sums asked for out of {"shift", "scale", "gate", "bias32", "bias16"}"""
    def build():
        g = Gen(seed)
        nb = rows // rpb
        x, dy = g.mat(rows, D, scale=1.2, shift=0.5), g.mat(rows, D, pad=8, scale=0.7, shift=0.1)
        scale, gate = _mod(g, nb, D, 1), _mod(g, nb, D, 2)
        dr = g.mat(rows, D, pad=16, scale=0.05) if dres else None
        o_dx = g.mat(rows, D, pad=40) if out else None
        outs = {"dx": o_dx} if out else {}
        kw = dict(dres=dr, gate=gate if gated else None, eps=1e-6, want_gated=gated, out=o_dx)
        if stats is None:
            call = lambda mod, T: mod.ln_modulate_bwd(T(dy), T(x), T(scale), rpb, **{k: T(v) for k, v in kw.items()})
        else:
            yb = g.mat(rows, D, pad=8) if "gate" in stats else None
            ds = {k: g.mat(nb, D, dtype=F32, pad=8) for k in ("shift", "scale", "gate") if k in stats}
            if "bias32" in stats or "bias16" in stats:
                ds["bias"] = g.blk(D, dtype=F32 if "bias32" in stats else BF16)
            outs.update({"d_" + k: v for k, v in ds.items()})
            kw.update(y_branch=yb, d_gate=ds.get("gate"), d_bias=ds.get("bias"))
            call = lambda mod, T: mod.ln_modulate_bwd_stats(T(dy), T(x), T(scale), rpb, T(ds.get("shift")), T(ds.get("scale")), **{k: T(v) for k, v in kw.items()})

        def ref(o):
            xd, dyd = x.double(), dy.double()
            L = NB.L_ln(ln_nc(D) if stats is None else ln_stats_nc(D))
            st = NB.ln_stats(xd, 1e-6, L)
            b = torch.arange(rows) // rpb
            want, e = NB.ln_bwd(dyd, xd, 1 + scale.double()[b], st, L, dres=dr.double() if dres else None)
            res = [("dx", want, e, "bf16")]
            if gated:
                res.append(("dxg", *NB.mul_stored(o["dx"].double(), gate.double()[b]), "bf16"))
            if stats:
                chunks = NB.cdiv(rpb, 64)
                Ls = NB.L_stats(chunks)
                xh = (xd - st.mu[:, None]) * st.r[:, None]
                e_xh = st.r[:, None] * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * NB.U)
                v = lambda t: t.view(nb, rpb, D)
                if "shift" in stats:
                    res.append(("d_shift", *NB.colsum(v(dyd), Ls), "f32s"))
                if "scale" in stats:
                    t = dyd * xh
                    res.append(("d_scale", *NB.colsum(v(t), Ls, v(dyd.abs() * e_xh + NB.U * t.abs())), "f32s"))
                if "gate" in stats:
                    t = o["dx"].double() * yb.double()
                    res.append(("d_gate", *NB.colsum(v(t), Ls, v(NB.U * t.abs())), "f32s"))
                if "d_bias" in outs:
                    w5, e5 = NB.colsum(o["dxg"].double(), NB.L_stats(nb * chunks))
                    res.append(("d_bias", w5, e5, "f32s" if "bias32" in stats else "bf16"))
            return res

        def ret(r):
            assert (r[1] is None) == (not gated), "dxg is returned exactly when want_gated"
            return {"dxg": r[1]} if out else {"dx": r[0], "dxg": r[1]}

        return Built(call, ref, g, outs, ret=ret, same=("dx", None) if out else None)
    return build


_i = 0
for _D, _rows, _rpb in LN_SHAPES:
    for _dres, _gated, _out in ((False, False, True), (True, True, False), (True, False, True)):
        _i += 1
        CASES.append(Case(f"ln_modulate_bwd_D{_D}_dres{int(_dres)}_gated{int(_gated)}_out{int(_out)}", "ln_modulate_bwd", "norm",
                          _ln_bwd(3100 + _i, _D, _rows, _rpb, _dres, _gated, _out),
                          frozenset(k for k, on in (("dres", _dres), ("gate", _gated), ("want_gated", _gated), ("out", _out), ("eps", True)) if on)))
    for _dres, _gated, _out, _st in ((True, True, True, ("shift", "scale", "gate", "bias32")), (False, True, False, ("shift", "scale", "bias16")),
                                     (True, False, True, ("shift", "scale")), (False, False, False, ())):
        _i += 1
        CASES.append(Case(f"ln_modulate_bwd_stats_D{_D}_{'_'.join(_st) or 'nosums'}", "ln_modulate_bwd_stats", "norm", _ln_bwd(3100 + _i, _D, _rows, _rpb, _dres, _gated, _out, stats=_st),
                          frozenset(k for k, on in (("dres", _dres), ("gate", _gated), ("want_gated", _gated), ("out", _out), ("eps", True), ("y_branch", "gate" in _st),
                                                    ("d_gate", "gate" in _st), ("d_bias", "bias32" in _st or "bias16" in _st)) if on)))


def _scale_cols_stats(seed, rpb, with_gate, bias, out):
    def build():
        g = Gen(seed)
        M, N = 96, 264
        nb = M // rpb
        x, yb = g.mat(M, N, shift=0.1), g.mat(M, N, pad=8)
        gate = _mod(g, nb, N, 1, scale=0.5)
        o_out = g.mat(M, N, pad=40) if out else None
        d_gate = g.mat(nb, N, dtype=F32, pad=8) if with_gate else None
        d_bias = g.blk(N, dtype=F32 if bias == 32 else BF16) if bias else None
        outs = {k: v for k, v in (("out", o_out), ("d_gate", d_gate), ("d_bias", d_bias)) if v is not None}
        call = lambda mod, T: mod.scale_cols_stats(T(x), T(gate), rpb, y_branch=T(yb) if with_gate else None, d_gate=T(d_gate), d_bias=T(d_bias), out=T(o_out))

        def ref(o):
            b = torch.arange(M) // rpb
            res = [("out", (x.double() * gate.double()[b]).float().to(BF16), None, "exact")]
            Ls = NB.L_stats(NB.cdiv(rpb, 64))
            if with_gate:
                t = (x.double() * yb.double()).view(nb, rpb, N)
                res.append(("d_gate", *NB.colsum(t, Ls, NB.U * t.abs()), "f32s"))
            if bias:
                res.append(("d_bias", *NB.colsum(o["out"].double(), NB.L_stats(nb * NB.cdiv(rpb, 64))), "f32s" if bias == 32 else "bf16"))
            return res

        return Built(call, ref, g, outs, ret=None if out else (lambda r: {"out": r}), same="out" if out else None)
    return build


CASES.append(Case("scale_cols_stats_all", "scale_cols_stats", "norm", _scale_cols_stats(3200, 48, True, 32, True), frozenset(("y_branch", "d_gate", "d_bias", "out"))))
CASES.append(Case("scale_cols_stats_bias16_rpb1", "scale_cols_stats", "norm", _scale_cols_stats(3201, 1, False, 16, False), frozenset(("d_bias",))))
CASES.append(Case("scale_cols_stats_none", "scale_cols_stats", "norm", _scale_cols_stats(3202, 48, False, 0, True), frozenset(("out",))))


def _colsum_rows(seed, per_batch, dtype, accumulate):
    """3 blocks of 48 rows, 60 rows apart"""
    def build():
        g = Gen(seed)
        rpb, stride, nb, N = 48, 60, 3, 264
        a = g.mat(nb * stride, N, shift=0.3)
        out = g.mat(nb, N, dtype=F32, pad=8) if per_batch else g.blk(N, dtype=dtype)
        prior = out.clone()
        rows = torch.stack([a[i * stride:i * stride + rpb] for i in range(nb)]).double()

        def ref(o):
            chunks = NB.cdiv(rpb, 64)
            if per_batch:
                w, e = NB.colsum(rows, NB.L_stats(chunks) + (1 if accumulate else 0))
            else:
                w, e = NB.colsum(rows.reshape(-1, N), NB.L_stats(nb * chunks) + (1 if accumulate else 0))
            if accumulate:
                w = w + prior.double()
                e = e + NB.U * w.abs()
            return [("out", w, e, "f32s" if out.dtype == F32 else "bf16")]

        return Built(lambda mod, T: mod.colsum_rows(T(a), rpb, stride, nb, T(out), per_batch=per_batch, accumulate=accumulate), ref, g, {"out": out}, same="out")
    return build


CASES.append(Case("colsum_rows_per_batch", "colsum_rows", "norm", _colsum_rows(3300, True, F32, False), frozenset(("per_batch",))))
CASES.append(Case("colsum_rows_reduced_bf16_accumulate", "colsum_rows", "norm", _colsum_rows(3301, False, BF16, True), frozenset(("accumulate",))))
CASES.append(Case("colsum_rows_reduced_f32", "colsum_rows", "norm", _colsum_rows(3302, False, F32, False), frozenset()))


def _colsum_prod(seed, with_b, mode, accumulate, rpb):
    def build():
        g = Gen(seed)
        rows, D = 96, 264
        r = rows if rpb is None else rpb
        nb = rows // r
        a, b = g.mat(rows, D, scale=0.5, shift=0.05), g.mat(rows, D, pad=8, scale=1.2)
        out = g.mat(nb, D, dtype=F32, pad=8)
        prior = out.clone()
        shift, scale = _mod(g, nb, D, 0), _mod(g, nb, D, 1)
        prev = g.mat(nb, D, dtype=F32, pad=16)
        kw = dict(b=b if with_b else None, rows_per_batch=rpb, mode=mode, accumulate=accumulate)
        if mode == 1:
            kw.update(prev=prev, shift=shift, scale=scale)

        def ref(o):
            Ls = NB.L_stats(NB.cdiv(r, 64))
            t = (a.double() * b.double() if with_b else a.double()).view(nb, r, D)
            w, e = NB.colsum(t, Ls, NB.U * t.abs() if with_b else None)
            if mode == 1:                       # d scale = (sum a b - shift prev) / (1 + scale)   (tests/test_norm_bounds_gpu.py test_colsum_prod)
                sp = shift.double() * prev.double()
                den = 1 + scale.double()
                w1 = (w - sp) / den
                e = (e + 2 * NB.U * (w.abs() + sp.abs())) / den.abs() + 2 * NB.U * w1.abs()
                w = w1
            if accumulate:
                w = w + prior.double()
                e = e + NB.U * w.abs()
            return [("out", w, e, "f32s")]

        return Built(lambda mod, T: mod.colsum_prod(T(a), T(out), **{k: T(v) for k, v in kw.items()}), ref, g, {"out": out}, same="out")
    return build


CASES.append(Case("colsum_prod_plain", "colsum_prod", "norm", _colsum_prod(3400, False, 0, False, None), frozenset()))
CASES.append(Case("colsum_prod_mode0_b_accumulate", "colsum_prod", "norm", _colsum_prod(3401, True, 0, True, 48), frozenset(("b", "rows_per_batch", "accumulate"))))
CASES.append(Case("colsum_prod_mode1", "colsum_prod", "norm", _colsum_prod(3402, True, 1, False, 48), frozenset(("b", "rows_per_batch", "mode", "prev", "shift", "scale"))))


def _layernorm(seed, op, flag):
    """affine LayerNorm: forward (flag: out= given), backward (flag: dres given), parameter gradients (flag: accumulate)"""
    def build():
        g = Gen(seed)
        rows, D = 96, 264
        x, dy = g.mat(rows, D, scale=2.0, shift=-0.7), g.mat(rows, D, pad=8)
        w, bias = g.blk(D, scale=0.3, shift=1.0), g.blk(D, scale=0.2)
        L = NB.L_ln(ln_nc(D))
        xd = x.double()
        a, bb = w.double()[None].expand(rows, D), bias.double()[None].expand(rows, D)
        if op == "fwd":
            out = g.mat(rows, D, pad=40) if flag else None

            def ref(o):
                want, e, _, _ = NB.norm_fwd(xd, NB.ln_stats(xd, 1e-5, L), a, bb)
                return [("y", want, e, "bf16")]
            return Built(lambda mod, T: mod.layernorm_fwd(T(x), T(w), T(bias), eps=1e-5, out=T(out)), ref, g, {"y": out} if flag else {},
                         ret=None if flag else (lambda r: {"y": r}), same="y" if flag else None)
        if op == "bwd":
            dres = g.mat(rows, D, pad=16, scale=0.1) if flag else None
            ref = lambda o: [("dx", *NB.ln_bwd(dy.double(), xd, a, NB.ln_stats(xd, 1e-5, L), L, dres=dres.double() if flag else None), "bf16")]
            return Built(lambda mod, T: mod.layernorm_bwd(T(dy), T(x), T(w), dres=T(dres), eps=1e-5), ref, g, ret=lambda r: {"dx": r})
        dw, db = g.blk(D, dtype=F32), g.blk(D, dtype=F32)
        p_w, p_b = dw.clone(), db.clone()

        def ref(o):
            st = NB.ln_stats(xd, 1e-5, NB.L_ln(lnp_nc(D)))
            xh = (xd - st.mu[:, None]) * st.r[:, None]
            e_xh = st.r[:, None] * st.e_mu[:, None] + xh.abs() * (st.e_r[:, None] + 2 * NB.U)
            Lp = NB.L_ln_params(rows) + (1 if flag else 0)
            t = dy.double() * xh
            ww, ew = NB.colsum(t, Lp, dy.double().abs() * e_xh + NB.U * t.abs())
            wb, eb = NB.colsum(dy.double(), Lp)
            if flag:
                ww, wb = ww + p_w.double(), wb + p_b.double()
            return [("dweight", ww, ew, "f32s"), ("dbias", wb, eb, "f32s")]

        return Built(lambda mod, T: mod.layernorm_param_grads(T(dy), T(x), T(dw), T(db), eps=1e-5, accumulate=flag), ref, g, {"dweight": dw, "dbias": db})
    return build


CASES.append(Case("layernorm_fwd_out", "layernorm_fwd", "norm", _layernorm(3500, "fwd", True), frozenset(("out", "eps"))))
CASES.append(Case("layernorm_fwd_alloc", "layernorm_fwd", "norm", _layernorm(3501, "fwd", False), frozenset(("eps",))))
CASES.append(Case("layernorm_bwd_dres", "layernorm_bwd", "norm", _layernorm(3502, "bwd", True), frozenset(("dres", "eps"))))
CASES.append(Case("layernorm_bwd", "layernorm_bwd", "norm", _layernorm(3503, "bwd", False), frozenset(("eps",))))
CASES.append(Case("layernorm_param_grads", "layernorm_param_grads", "norm", _layernorm(3504, "params", False), frozenset(("eps",))))
CASES.append(Case("layernorm_param_grads_accumulate", "layernorm_param_grads", "norm", _layernorm(3505, "params", True), frozenset(("eps", "accumulate"))))


# =============================================================================================================================================================
# step family: rank-space products, adapter packing, noise mixes, losses, optimizers, gradient norm / clamp / clip
# =============================================================================================================================================================
SK_M, SK_P = 192, 72


def skinny_chunk(M, P, seg_rows=0):
    """skinny.hip skinny_chunk: (mc, nchunks)"""
    pt = NB.cdiv(P, 64)
    for mc in (1024, 512):
        if (seg_rows == 0 or seg_rows % mc == 0) and NB.cdiv(M, mc) * pt >= 512:
            return mc, NB.cdiv(M, mc)
    return 256, NB.cdiv(M, 256)


def _skinny(seed, transposed, accumulate, alpha, multi=0):
    """skinny_tn (R 32 wide, r_used 16) or skinny_tn_multi (R 128 wide, `multi` outputs); transposed: the output is stored [r, P] (so_p = 1)"""
    def build():
        g = Gen(seed)
        r_used = 16
        Lm, R = g.mat(SK_M, SK_P), g.mat(SK_M, 128 if multi else 32, pad=32, shift=0.25)
        bufs = [g.mat(r_used, SK_P, dtype=F32, pad=8) if transposed else g.mat(SK_P, r_used, dtype=F32, pad=8) for _ in range(max(multi, 1))]
        so_p, so_r = (1, SK_P + 8) if transposed else (r_used + 8, 1)
        priors = [b.clone() for b in bufs]
        mc, nch = skinny_chunk(SK_M, SK_P)
        kw = dict(alpha=alpha, accumulate=accumulate)
        if multi:
            call = lambda mod, T: mod.skinny_tn_multi(T(Lm), T(R), [T(b) for b in bufs], so_p, so_r, r_used, **kw)
        else:
            call = lambda mod, T: mod.skinny_tn(T(Lm), T(R), T(bufs[0]), so_p, so_r, r_used, **kw)

        def ref(o):
            res = []
            for i, (b, p) in enumerate(zip(bufs, priors)):
                pr = (p.t() if transposed else p) if accumulate else None
                want, e = SB.skinny(Lm, R[:, 32 * i:32 * i + r_used], alpha, mc, nch, prior=pr)
                res.append((f"out{i}", want.t() if transposed else want, e.t() if transposed else e, "f32s"))
            return res

        return Built(call, ref, g, {f"out{i}": b for i, b in enumerate(bufs)}, same=None if multi else "out0")
    return build


CASES.append(Case("skinny_tn_transposed_accumulate", "skinny_tn", "step", _skinny(4000, True, True, 0.5), frozenset(("alpha", "accumulate"))))
CASES.append(Case("skinny_tn_plain", "skinny_tn", "step", _skinny(4001, False, False, 1.0), frozenset()))
CASES.append(Case("skinny_tn_multi_4", "skinny_tn_multi", "step", _skinny(4002, False, False, 0.25, multi=4), frozenset(("alpha",))))
CASES.append(Case("skinny_tn_multi_3_transposed_accumulate", "skinny_tn_multi", "step", _skinny(4003, True, True, 1.0, multi=3), frozenset(("accumulate",))))


@case("lora_pack", "step", opts=("k2_off", "n_off"))
def _lora_pack():
    """A [16, 72], B [40, 16] into a 64-wide rank granule at k2_off 16 and rows n_off 24 of 104: bf16(A) is one RNE of an exact value (bit-exact); bf16(scale * B)
    is one fp32 product and one store (k_lora_pack, optim.hip): e = u |want|"""
    g = Gen(4100)
    r, K, N, K2, NT, k2, n0, scale = 16, 72, 40, 64, 104, 16, 24, 0.37
    A, Bm = g.blk(r, K, dtype=F32, scale=0.1), g.blk(N, r, dtype=F32, scale=0.1)
    A_cat, A_cat_T, B_blk, B_blk_T = g.blk(K2, K), g.blk(K, K2), g.blk(NT, K2), g.blk(K2, NT)
    outs = {"A_cat": A_cat[k2:k2 + r], "A_cat_T": A_cat_T[:, k2:k2 + r], "B_blk": B_blk[n0:n0 + N, k2:k2 + r], "B_blk_T": B_blk_T[k2:k2 + r, n0:n0 + N]}

    def ref(o):
        wb = SB.f32(scale) * Bm.double()
        return [("A_cat", A.to(BF16), None, "exact"), ("A_cat_T", A.t().to(BF16), None, "exact"),
                ("B_blk", wb, U * wb.abs(), "bf16e"), ("B_blk_T", wb.t(), U * wb.t().abs(), "bf16e")]

    return Built(lambda mod, T: mod.lora_pack(T(A), T(Bm), scale, T(A_cat), T(A_cat_T), T(B_blk), T(B_blk_T), k2_off=k2, n_off=n0), ref, g, outs)


def _noise_mix(seed, flow, second):
    """flow_noise_mix with noise= given / ddpm_noise_mix; second: the target / v output is asked for"""
    def build():
        g = Gen(seed)
        B, per = 6, 136
        x, noise = g.mat(B, per), g.mat(B, per, pad=8)
        s1, s2 = g.blk(B, dtype=F32), g.blk(B, dtype=F32)
        s1.copy_(torch.tensor([0.0, 1.0, 0.25, 0.7311, 0.5, 0.999]))          # sigma = 0 and 1 return x and the noise themselves
        s2.copy_((1 - s1 * s1).sqrt())
        if flow:
            call = lambda mod, T: mod.flow_noise_mix(T(x), T(s1), noise=T(noise), want_target=second)
        else:
            call = lambda mod, T: mod.ddpm_noise_mix(T(x), T(noise), T(s1), T(s2), want_v=second)

        def ref(o):
            a, b = SB.flow_mix(x, noise, s1) if flow else SB.ddpm_mix(x, noise, s1, s2)
            return [("x_t", *a, "bf16")] + ([("second", *b, "bf16")] if second else [])

        def ret(r):
            assert (r[1] is None) == (not second)
            return {"x_t": r[0], "second": r[1]}

        return Built(call, ref, g, ret=ret)
    return build


CASES.append(Case("flow_noise_mix_target", "flow_noise_mix", "step", _noise_mix(4200, True, True), frozenset(("noise", "want_target"))))
CASES.append(Case("flow_noise_mix_no_target", "flow_noise_mix", "step", _noise_mix(4201, True, False), frozenset(("noise", "want_target"))))
CASES.append(Case("ddpm_noise_mix_v", "ddpm_noise_mix", "step", _noise_mix(4202, False, True), frozenset(("want_v",))))
CASES.append(Case("ddpm_noise_mix_no_v", "ddpm_noise_mix", "step", _noise_mix(4203, False, False), frozenset(("want_v",))))


def _loss(seed, fn, loss_type, weight, emask, want_grad, huber_tensor=False, grad_scale=1.0):
    """pred / target [4, 3, 88] (per-sample 264, emask period 88)"""
    def build():
        g = Gen(seed)
        B, Cn, P = 4, 3, 88
        pred, target = g.blk(B, Cn, P), g.blk(B, Cn, P)
        w = g.blk(B, dtype=F32, scale=0.2, shift=1.0) if weight else None
        em = g.blk(B, P, dtype=F32) if emask else None
        if emask:
            em.copy_((em > 0).float())
        hc = g.blk(B, dtype=F32) if huber_tensor else 0.1
        if huber_tensor:
            hc.copy_(torch.tensor([0.05, 0.1, 0.3, 1.0]))
        if fn == "mse_loss":
            call = lambda mod, T: mod.mse_loss(T(pred), T(target), weight=T(w), want_grad=want_grad, grad_scale=grad_scale)
        else:
            call = lambda mod, T: mod.cond_loss(T(pred), T(target), loss_type=loss_type, huber_c=T(hc), weight=T(w), want_grad=want_grad, grad_scale=grad_scale, emask=T(em))

        def ref(o):
            cv = hc if torch.is_tensor(hc) else torch.full((B,), SB.f32(hc))
            r = SB.loss(pred.reshape(B, -1), target.reshape(B, -1), loss_type, huber_c=cv, weight=w, emask=em, grad_scale=grad_scale)
            res = [("per_sample", *r["per_sample"], "f32s"), ("loss", *r["loss"], "f32s")]
            if want_grad:
                res.append(("dpred", r["dpred"][0].reshape(B, Cn, P), r["dpred"][1].reshape(B, Cn, P), "bf16"))
            return res

        def ret(r):
            assert (r[2] is None) == (not want_grad)
            return {"loss": r[0], "per_sample": r[1], "dpred": r[2]}

        return Built(call, ref, g, ret=ret)
    return build


CASES.append(Case("mse_loss_weight_grad", "mse_loss", "step", _loss(4300, "mse_loss", "l2", True, False, True, grad_scale=0.5), frozenset(("weight", "want_grad", "grad_scale"))))
CASES.append(Case("mse_loss_plain_no_grad", "mse_loss", "step", _loss(4301, "mse_loss", "l2", False, False, False), frozenset(("want_grad",))))
for _i, (_lt, _w, _em, _wg, _ht) in enumerate((("l2", True, True, True, False), ("l2", False, False, False, False), ("huber", True, True, True, True),
                                               ("huber", False, False, False, False), ("smooth_l1", True, False, True, False), ("smooth_l1", False, True, False, True))):
    CASES.append(Case(f"cond_loss_{_lt}_w{int(_w)}_mask{int(_em)}_grad{int(_wg)}", "cond_loss", "step", _loss(4310 + _i, "cond_loss", _lt, _w, _em, _wg, _ht, grad_scale=2.0 if _wg else 1.0),
                      frozenset(k for k, on in (("loss_type", True), ("huber_c", _lt != "l2"), ("weight", _w), ("want_grad", True), ("grad_scale", _wg), ("emask", _em)) if on)))


ADAM_N = 4096 + 40


def _adamw(seed, dtype, with_ema, with_pb, wd):
    """three steps over 4096 + 40 elements; every step is judged from the state stored before it (the snapshots the call keeps), as the family test chains"""
    def build():
        g = Gen(seed)
        n = ADAM_N
        p, gr = g.blk(n, dtype=dtype, scale=0.05), g.blk(n, dtype=dtype, scale=1e-3)
        m, v = g.blk(n, dtype=F32, scale=1e-3), g.blk(n, dtype=F32, scale=1e-3)
        v.copy_(v * v)
        m[::22] = 0
        v[::11] = 0
        gr[::11] = 0                       # v = 0 and g = 0: the denominator is eps (tests/test_step_bounds_gpu.py _adam_state)
        ema = g.blk(n, dtype=dtype, scale=0.05)
        pbf = g.blk(n)
        hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, grad_scale=0.5, ema_decay=0.99)
        kw = dict(ema=ema if with_ema else None)
        if dtype == F32:
            kw["p_bf16"] = pbf if with_pb else None
        state = {"p": p, "m": m, "v": v, "ema": ema, "pbf": pbf}
        snaps = []

        def call(mod, T, step):
            if step == 1:
                snaps.append({k: T(t).detach().cpu().clone() for k, t in state.items()})
            mod.adamw_ema_step(T(p), T(gr), T(m), T(v), step, **hp, **{k: T(t) for k, t in kw.items()})
            snaps.append({k: T(t).detach().cpu().clone() for k, t in state.items()})

        def ret(r):
            return {f"{k}{s}": t for s in (1, 2, 3) for k, t in snaps[s].items()}

        def ref(o):
            res = []
            for s in (1, 2, 3):
                c = SB.adam_consts(hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, s, hp["grad_scale"], hp["ema_decay"])
                a, b = snaps[s - 1], snaps[s]
                r = SB.adamw(a["p"], gr, a["m"], a["v"], c)
                res += [(f"m{s}", *r["m"], "f32"), (f"v{s}", *r["v"], "f32"), (f"p{s}", *r["p"], "f32" if dtype == F32 else "bf16")]
                if with_ema:
                    res.append((f"ema{s}", *(SB.ema_f32 if dtype == F32 else SB.ema_bf16)(a["ema"], b["p"], c["omd"]), "f32" if dtype == F32 else "bf16"))
                else:
                    res.append((f"ema{s}", a["ema"], None, "exact"))
                res.append((f"pbf{s}", GB.to_bf16_rne(b["p"]) if (dtype == F32 and with_pb) else a["pbf"], None, "exact"))
            return res

        outs = {"p": p, "m": m, "v": v}
        if with_ema:
            outs["ema"] = ema
        if dtype == F32 and with_pb:
            outs["pbf"] = pbf
        return Built(call, ref, g, outs, ret=ret, steps=3)
    return build


CASES.append(Case("adamw_ema_step_f32_ema_pbf16", "adamw_ema_step", "step", _adamw(4400, F32, True, True, 1e-2),
                  frozenset(("beta1", "beta2", "eps", "weight_decay", "grad_scale", "ema", "ema_decay", "p_bf16"))))
CASES.append(Case("adamw_ema_step_f32_plain", "adamw_ema_step", "step", _adamw(4401, F32, False, False, 0.0), frozenset(("beta1", "beta2", "eps", "weight_decay", "grad_scale"))))
CASES.append(Case("adamw_ema_step_bf16_ema", "adamw_ema_step", "step", _adamw(4402, BF16, True, False, 1e-2), frozenset(("ema", "ema_decay"))))


@case("adamw_bf16_sr_step", "step", opts=("seg_end", "seg_decay", "rand_bits", "grad_scale"))
def _adamw_bf16_sr():
    """a two-tensor arena (1000 + 40 elements, decay released for the second) with the stochastic-rounding draws given: the existing GPU test
    (tests/test_adamw_bf16_gpu.py) states the result bit-exactly against oracle.train_math.adamw_bf16_step; grad_scale 0.5 scales a bf16 gradient exactly"""
    from oracle import train_math as TM
    g = Gen(4500)
    n0, n = 1000, 1040
    mk = lambda s: g.blk(n, scale=s)
    p, gr, m, v, sh = mk(0.5), mk(0.2), mk(0.05), mk(0.05), mk(1e-3)
    v.copy_((v.float() ** 2).to(BF16))
    rb = g.blk(4, n, dtype=I32)
    rb.copy_(torch.randint(0, 65536, (4, n), generator=g.g, dtype=I32))
    seg_end, seg_decay = g.blk(2, dtype=torch.int64), g.blk(2, dtype=F32)
    seg_end.copy_(torch.tensor([n0, n]))
    seg_decay.copy_(torch.tensor([0.0, 7e-3]))
    init = [t.clone() for t in (p, gr, m, v, sh)]

    def ref(o):
        res = {k: torch.empty(n, dtype=BF16) for k in ("p", "m", "v", "shift")}
        for lo, hi, dec in ((0, n0, 0.0), (n0, n, 7e-3)):
            c = [t[lo:hi] for t in init]
            out = TM.adamw_bf16_step(c[0], (c[1].float() * 0.5).to(BF16), c[2], c[3], c[4], 3, 1e-2, 0.9, 0.999, 1e-8, dec, [rb[k, lo:hi] for k in range(4)])
            for k, t in zip(("p", "m", "v", "shift"), out):
                res[k][lo:hi] = t
        return [(k, t, None, "exact") for k, t in res.items()]

    call = lambda mod, T: mod.adamw_bf16_sr_step(T(p), T(gr), T(m), T(v), T(sh), 3, 1e-2, 0.9, 0.999, 1e-8, seg_end=T(seg_end), seg_decay=T(seg_decay), rand_bits=T(rb),
                                                 grad_scale=0.5)
    return Built(call, ref, g, {"p": p, "m": m, "v": v, "shift": sh})


def _ema_update(seed, dtype):
    def build():
        g = Gen(seed)
        n, decay = ADAM_N, 0.999
        p, s = g.blk(n, dtype=dtype, scale=0.05), g.blk(n, dtype=dtype, scale=0.05)
        s0 = s.clone()
        omd = float(np.float32(1.0) - np.float32(decay))
        ref = lambda o: [("s", *(SB.ema_f32 if dtype == F32 else SB.ema_bf16)(s0, p, omd), "f32" if dtype == F32 else "bf16")]
        return Built(lambda mod, T: mod.ema_update(T(s), T(p), decay), ref, g, {"s": s})
    return build


CASES.append(Case("ema_update_f32", "ema_update", "step", _ema_update(4600, F32), frozenset()))
CASES.append(Case("ema_update_bf16", "ema_update", "step", _ema_update(4601, BF16), frozenset()))


def _grad_norm(seed, dtype):
    def build():
        g = Gen(seed)
        gr = g.blk(ADAM_N + 3 if dtype == F32 else ADAM_N, dtype=dtype, scale=0.02)

        def ref(o):
            want, e, mx = SB.grad_norm(gr)
            return [("ss", want, e, "f32s"), ("max", mx.float().reshape(1), None, "exact")]

        return Built(lambda mod, T: mod.grad_norm(T(gr)), ref, g, ret=lambda r: {"ss": r[0:1].reshape(1, 1), "max": r[1:2]})
    return build


CASES.append(Case("grad_norm_f32", "grad_norm", "step", _grad_norm(4700, F32), frozenset()))
CASES.append(Case("grad_norm_bf16", "grad_norm", "step", _grad_norm(4701, BF16), frozenset()))


def _grad_clamp(seed, dtype):
    def build():
        g = Gen(seed)
        c = 0.013
        gr = g.blk(ADAM_N + 3 if dtype == F32 else ADAM_N, dtype=dtype, scale=0.02)
        want = gr.float().clamp(-SB.f32(c), SB.f32(c)).to(dtype)          # exact: a comparison, then (bf16) one RNE of the fp32 bound
        return Built(lambda mod, T: mod.grad_clamp_(T(gr), c), lambda o: [("g", want, None, "exact")], g, {"g": gr}, same="g")
    return build


CASES.append(Case("grad_clamp_f32", "grad_clamp_", "step", _grad_clamp(4800, F32), frozenset()))
CASES.append(Case("grad_clamp_bf16", "grad_clamp_", "step", _grad_clamp(4801, BF16), frozenset()))


def _grad_clip(seed, dtype, clips):
    """stats = the stored (sum of squares, max) of g; clips: max_norm below the norm, else coef >= 1 must leave every bit alone"""
    def build():
        g = Gen(seed)
        gr = g.blk(ADAM_N + 3 if dtype == F32 else ADAM_N, dtype=dtype, scale=0.02)
        g0 = gr.clone()
        stats = g.blk(2, dtype=F32)
        stats.copy_(torch.stack([(g0.double() ** 2).sum(), g0.double().abs().max()]).float())
        max_norm, pre = (0.5, 1.5) if clips else (100.0, 1.0)

        def ref(o):
            coef = SB.clip_coef(float(stats[0]), max_norm, pre)
            assert (coef < 1.0) == clips
            if not clips:
                return [("g", g0, None, "exact")]
            return [("g", *SB.grad_clip(g0, coef), "f32" if dtype == F32 else "bf16")]

        return Built(lambda mod, T: mod.grad_clip_norm_(T(gr), T(stats), max_norm, pre_scale=pre), ref, g, {"g": gr}, same="g")
    return build


CASES.append(Case("grad_clip_norm_f32_clips", "grad_clip_norm_", "step", _grad_clip(4900, F32, True), frozenset(("pre_scale",))))
CASES.append(Case("grad_clip_norm_bf16_clips", "grad_clip_norm_", "step", _grad_clip(4901, BF16, True), frozenset(("pre_scale",))))
CASES.append(Case("grad_clip_norm_bf16_keeps", "grad_clip_norm_", "step", _grad_clip(4902, BF16, False), frozenset(("pre_scale",))))


# =============================================================================================================================================================
# grid path (UNet / VAE): B 2, H 8, W 12, channels 64 -> 128
# =============================================================================================================================================================
GB_, GH, GW, GCI, GCO = 2, 8, 12, 64, 128


def _grid(g, B, H, W, C, scale=1.0, shift=0.0):
    """a contiguous grid buffer inside a guarded allocation (border and tail rows zero) and its image [B, H, W, C]"""
    t = g.blk(CB.grid_rows(B, H, W), C, scale=scale, shift=shift)
    img = t[CB.interior_rows(B, H, W)].view(B, H, W, C).clone()
    t.copy_(CB.image_to_grid(img))
    return t, img


def _split_grid(B, H, W, label="y"):
    """ret(): a returned grid as its image rows (bounded) and everything else (zero of either sign)"""
    rows = CB.interior_rows(B, H, W)

    def ret(r):
        assert r.shape[0] == CB.grid_rows(B, H, W), tuple(r.shape)
        rest = torch.ones(r.shape[0], dtype=torch.bool)
        rest[rows] = False
        return {label: r[rows.to(r.device)], label + "_rest": r[rest.to(r.device)]}
    return ret


def _whole(img):
    return lambda o: [("y", CB.image_to_grid(img), None, "exact")]


@case("grid_from_nchw", "grid")
def _grid_from_nchw():
    g = Gen(5000)
    x = g.blk(GB_, 40, GH, GW)
    img = torch.zeros(GB_, GH, GW, GCI, dtype=BF16)
    img[..., :40] = x.permute(0, 2, 3, 1)
    return Built(lambda mod, T: mod.grid_from_nchw(T(x), GCI), _whole(img), g, ret=lambda r: {"y": r})


@case("grid_to_nchw", "grid")
def _grid_to_nchw():
    g = Gen(5001)
    t, img = _grid(g, GB_, GH, GW, GCI)
    want = img[..., :40].permute(0, 3, 1, 2).contiguous()
    return Built(lambda mod, T: mod.grid_to_nchw(T(t), GB_, 40, GH, GW), lambda o: [("y", want, None, "exact")], g, ret=lambda r: {"y": r})


def _tokens_to_grid(seed, residual):
    def build():
        g = Gen(seed)
        tok = g.blk(GB_ * GH * GW, GCI)          # dense: st355_tokens_to_grid takes no row stride
        res, rimg = _grid(g, GB_, GH, GW, GCI)
        timg = tok.reshape(GB_, GH, GW, GCI)
        if not residual:
            return Built(lambda mod, T: mod.tokens_to_grid(T(tok), GB_, GH, GW), _whole(timg), g, ret=lambda r: {"y": r})
        want, e = CB.tokens_residual_expect(timg, rimg)
        ref = lambda o: [("y", want.reshape(-1, GCI), e.reshape(-1, GCI), "bf16"), ("y_rest", None, None, "zero")]
        return Built(lambda mod, T: mod.tokens_to_grid(T(tok), GB_, GH, GW, residual=T(res)), ref, g, ret=_split_grid(GB_, GH, GW))
    return build


CASES.append(Case("tokens_to_grid", "tokens_to_grid", "grid", _tokens_to_grid(5010, False), frozenset()))
CASES.append(Case("tokens_to_grid_residual", "tokens_to_grid", "grid", _tokens_to_grid(5011, True), frozenset(("residual",))))


@case("grid_to_tokens", "grid")
def _grid_to_tokens():
    g = Gen(5020)
    t, img = _grid(g, GB_, GH, GW, GCI)
    return Built(lambda mod, T: mod.grid_to_tokens(T(t), GB_, GH, GW), lambda o: [("y", img.reshape(-1, GCI), None, "exact")], g, ret=lambda r: {"y": r})


def _conv(seed, taps, bias, img_add, residual, out):
    """out= given: the rows the GEMM covers, [W + 3, positions - W - 3), are owned; the first / last W + 3 positions and the tail keep their (zero) bits"""
    def build():
        g = Gen(seed)
        x, ximg = _grid(g, GB_, GH, GW, GCI)
        w = g.blk(GCO, taps * GCI, scale=0.04)
        b = g.blk(GCO, scale=0.1) if bias else None
        ia = g.mat(GB_, GCO, pad=GCO) if img_add else None
        res, rimg = _grid(g, GB_, GH, GW, GCO) if residual else (None, None)
        o_buf = None
        outs = {}
        if out:
            o_buf = g.blk(CB.grid_rows(GB_, GH, GW), GCO)
            n, p0 = CB.grid_positions(GB_, GH, GW), GW + 3
            o_buf[:p0] = 0
            o_buf[n - p0:] = 0
            outs["whole"] = o_buf[p0:n - p0]
        def ref(o):
            want, e = CB.conv_ref(ximg, w, taps, bias=b, img_add=ia, residual_img=rimg)
            return [("y", want, e, "bf16"), ("y_rest", None, None, "zero")]

        return Built(lambda mod, T: mod.conv(T(x), T(w), GB_, GH, GW, bias=T(b), img_add=T(ia), residual=T(res), taps=taps, out=T(o_buf)), ref, g, outs,
                     ret=_split_grid(GB_, GH, GW))
    return build


CASES.append(Case("conv_taps9_bias_img_add", "conv", "grid", _conv(5100, 9, True, True, False, False), frozenset(("bias", "img_add", "taps"))))
CASES.append(Case("conv_taps9_residual_out", "conv", "grid", _conv(5101, 9, True, False, True, True), frozenset(("bias", "residual", "taps", "out"))))
CASES.append(Case("conv_taps1_residual", "conv", "grid", _conv(5102, 1, False, False, True, False), frozenset(("residual", "taps"))))
CASES.append(Case("conv_taps1_plain_out", "conv", "grid", _conv(5103, 1, False, False, False, True), frozenset(("taps", "out"))))


def _conv_wgrad(seed, taps, accumulate):
    """the bound's contraction length Mc and K-slice count come from the device's plan (ops.conv_wgrad_plan) where the module has one; the emulator has no
    route: there the grid positions rounded to the 64-row K granule in one slice"""
    def build():
        g = Gen(seed)
        x, ximg = _grid(g, GB_, GH, GW, GCI)
        dy, dimg = _grid(g, GB_, GH, GW, GCO, scale=0.1)
        dw = g.blk(GCO, taps * GCI)
        old = dw.clone()
        plan = {"Mc": NB.cdiv(CB.grid_positions(GB_, GH, GW), 64) * 64, "ks": 1}

        def call(mod, T):
            if hasattr(mod, "conv_wgrad_plan"):
                plan.update(mod.conv_wgrad_plan(GB_, GH, GW, GCI, GCO, taps=taps, accumulate=accumulate))
            return mod.conv_wgrad(T(x), T(dy), T(dw), GB_, GH, GW, taps=taps, accumulate=accumulate)

        ref = lambda o: [("dw", *CB.wgrad_ref(ximg, dimg, taps, plan["Mc"], plan["ks"], old=old if accumulate else None), "bf16")]
        return Built(call, ref, g, {"dw": dw}, same="dw")
    return build


CASES.append(Case("conv_wgrad_taps9_accumulate", "conv_wgrad", "grid", _conv_wgrad(5200, 9, True), frozenset(("taps", "accumulate"))))
CASES.append(Case("conv_wgrad_taps1", "conv_wgrad", "grid", _conv_wgrad(5201, 1, False), frozenset(("taps",))))


def _im2col(seed, stride, pad, back):
    def build():
        g = Gen(seed)
        Kpad = (9 * GCI + 63) // 64 * 64
        Ho, Wo = GH // stride, GW // stride
        if not back:
            x, ximg = _grid(g, GB_, GH, GW, GCI)
            return Built(lambda mod, T: mod.im2col3x3(T(x), GB_, GH, GW, stride=stride, pad=pad), _whole(CB.im2col_expect(ximg, stride, pad, Kpad)), g, ret=lambda r: {"y": r})
        dcol, dimg = _grid(g, GB_, Ho, Wo, Kpad, scale=0.3)
        want, e = CB.col2im_expect(dimg, GH, GW, GCI, stride, pad)
        ref = lambda o: [("y", want.reshape(-1, GCI), e.reshape(-1, GCI), "bf16"), ("y_rest", None, None, "zero")]
        return Built(lambda mod, T: mod.col2im3x3(T(dcol), GB_, GH, GW, GCI, stride=stride, pad=pad), ref, g, ret=_split_grid(GB_, GH, GW))
    return build


for _i, (_s, _p) in enumerate(((1, 1), (2, 1), (2, 0))):
    CASES.append(Case(f"im2col3x3_s{_s}_p{_p}", "im2col3x3", "grid", _im2col(5300 + _i, _s, _p, False), frozenset(("stride", "pad"))))
    CASES.append(Case(f"col2im3x3_s{_s}_p{_p}", "col2im3x3", "grid", _im2col(5310 + _i, _s, _p, True), frozenset(("stride", "pad"))))


@case("upsample2x", "grid")
def _upsample2x():
    g = Gen(5400)
    x, ximg = _grid(g, GB_, GH, GW, GCI)
    return Built(lambda mod, T: mod.upsample2x(T(x), GB_, GH, GW), _whole(CB.upsample_expect(ximg)), g, ret=lambda r: {"y": r})


@case("upsample2x_bwd", "grid")
def _upsample2x_bwd():
    g = Gen(5401)
    dy, dimg = _grid(g, GB_, 2 * GH, 2 * GW, GCI)
    want, e = CB.upsample_bwd_expect(dimg)
    ref = lambda o: [("y", want.reshape(-1, GCI), e.reshape(-1, GCI), "bf16"), ("y_rest", None, None, "zero")]
    return Built(lambda mod, T: mod.upsample2x_bwd(T(dy), GB_, GH, GW), ref, g, ret=_split_grid(GB_, GH, GW))


def gn_route(B, H, W):
    """norm_route.h gn_route_chunks: (rows_per_chunk, nch)"""
    rows_img = (H + 2) * (W + 2)
    nch = max(1, min(NB.cdiv(768, B), NB.cdiv(rows_img, 32)))
    rpc = NB.cdiv(rows_img, nch)
    return rpc, NB.cdiv(rows_img, rpc)


GN_G = 32


def _gn_groups(t, B, HW, C):
    """[B, HW, C] -> [B G, HW cg]: one row per (image, group)"""
    cg = C // GN_G
    return t.reshape(B, HW, GN_G, cg).permute(0, 2, 1, 3).reshape(B * GN_G, -1)


def _gn_ungroup(t, B, HW, C):
    cg = C // GN_G
    return t.reshape(B, GN_G, HW, cg).permute(0, 2, 1, 3).reshape(B, HW, C)


def _gn_fwd(seed, silu, out_tokens, eps):
    def build():
        g = Gen(seed)
        B, H, W, C = GB_, GH, GW, GCI
        x, ximg = _grid(g, B, H, W, C, scale=0.7, shift=0.4)
        gamma, beta = g.blk(C, scale=0.2, shift=1.0), g.blk(C, scale=0.3)
        rpc, nch = gn_route(B, H, W)
        L = NB.L_gn(rpc, NB.gn_stats_RT(C), nch, C // GN_G)

        def ref(o):
            xs = _gn_groups(ximg.double().reshape(B, H * W, C), B, H * W, C)
            st = NB.ln_stats(xs, eps, L, pivoted=True)
            ga = _gn_groups(gamma.double().expand(B, H * W, C), B, H * W, C)
            be = _gn_groups(beta.double().expand(B, H * W, C), B, H * W, C)
            want, e, _, _ = NB.norm_fwd(xs, st, ga, be, silu=silu)
            per_c = lambda v: v.view(B, GN_G, 1).expand(B, GN_G, C // GN_G).reshape(B, C)
            res = [("y", _gn_ungroup(want, B, H * W, C).reshape(-1, C), _gn_ungroup(e, B, H * W, C).reshape(-1, C), "bf16e"),
                   ("mean", per_c(st.mu), per_c(st.e_mu), "f32"), ("rstd", per_c(st.r), per_c(st.r * st.e_r), "f32")]
            return res if out_tokens else res + [("y_rest", None, None, "zero")]

        def ret(r):
            y, stats = r
            d = {"y": y} if out_tokens else _split_grid(B, H, W)(y)
            assert tuple(stats.shape) == (B, C, 2)
            d.update(mean=stats[..., 0], rstd=stats[..., 1])
            return d

        return Built(lambda mod, T: mod.groupnorm_fwd(T(x), T(gamma), T(beta), B, H, W, groups=GN_G, eps=eps, silu=silu, out_tokens=out_tokens), ref, g, ret=ret)
    return build


CASES.append(Case("groupnorm_fwd_silu_grid", "groupnorm_fwd", "grid", _gn_fwd(5500, True, False, 1e-5), frozenset(("groups", "eps", "silu", "out_tokens"))))
CASES.append(Case("groupnorm_fwd_tokens", "groupnorm_fwd", "grid", _gn_fwd(5501, False, True, 1e-6), frozenset(("groups", "eps", "silu", "out_tokens"))))


def _gn_bwd(seed, silu, dy_tokens, dadd_on, params, accumulate):
    """chained on the statistics a forward stored: here the fp32 roundings of the exact mean / rstd, handed in as the saved `stats`"""
    def build():
        g = Gen(seed)
        B, H, W, C = GB_, GH, GW, GCI
        cg, HW = C // GN_G, GH * GW
        x, ximg = _grid(g, B, H, W, C, scale=0.7, shift=0.4)
        gamma, beta = g.blk(C, scale=0.2, shift=1.0), g.blk(C, scale=0.3)
        if dy_tokens:
            dy = g.blk(B * HW, C, scale=0.5, shift=0.05)          # dense: st355_groupnorm_bwd takes no row stride
            dimg = dy.reshape(B, H, W, C)
        else:
            dy, dimg = _grid(g, B, H, W, C, scale=0.5, shift=0.05)
        dadd, aimg = _grid(g, B, H, W, C, scale=0.1) if dadd_on else (None, None)
        xs = _gn_groups(ximg.double().reshape(B, HW, C), B, HW, C)
        mu = xs.mean(1)
        rs = 1.0 / torch.sqrt(((xs - mu[:, None]) ** 2).mean(1) + 1e-5)
        per_c = lambda v: v.view(B, GN_G, 1).expand(B, GN_G, cg).reshape(B, C)
        stats = g.blk(B, C, 2, dtype=F32)
        stats.copy_(torch.stack([per_c(mu), per_c(rs)], dim=2).float())
        dgam, dbet = (g.blk(C, dtype=F32), g.blk(C, dtype=F32)) if params else (None, None)
        c0 = (dgam.clone(), dbet.clone()) if params else None
        rpc, nch = gn_route(B, H, W)
        L = NB.L_gn(rpc, NB.gn_stats_RT(C), nch, cg)

        def ref(o):          # tests/test_norm_bounds_gpu.py test_groupnorm, the backward half
            mu_f, r_f = stats[..., 0].double()[:, None, :], stats[..., 1].double()[:, None, :]
            xd, dyd = ximg.double().reshape(B, HW, C), dimg.double().reshape(B, HW, C)
            xh = (xd - mu_f) * r_f
            ga, be = gamma.double(), beta.double()
            if silu:
                z = xh * ga + be
                s = torch.sigmoid(z)
                sp = s * (1 + z * (1 - s))
                spp = s * (1 - s) * (2 + z * (1 - 2 * s))
                gg = dyd * sp
                e_g = gg.abs() * (2.0 ** -21 * (2 + z.abs()) + 6 * NB.U) + dyd.abs() * spp.abs() * (ga.abs() * 2 * NB.U * xh.abs() + NB.U * z.abs())
            else:
                gg, e_g = dyd, torch.zeros_like(dyd)
            Lb, n = L + 3, HW * cg
            grp = lambda t: t.view(B, HW, GN_G, cg).sum((1, 3))
            S1, S2 = grp(ga * gg), grp(ga * gg * xh)
            eS1 = Lb * NB.U * grp((ga * gg).abs()) + grp(ga.abs() * e_g)
            eS2 = Lb * NB.U * grp((ga * gg * xh).abs()) + grp(ga.abs() * (e_g * xh.abs() + gg.abs() * 2 * NB.U * xh.abs()))
            ex = lambda t: t.repeat_interleave(cg, 1)[:, None, :]
            c2, c3, c1 = -r_f * ex(S2) / n, -r_f * ex(S1) / n, r_f * ga
            want = c1 * gg + c2 * xh + c3
            e = r_f * (ga.abs() * e_g + xh.abs() * ex(eS2) / n + ex(eS1) / n) + 4 * NB.U * ((c1 * gg).abs() + (c2 * xh).abs() + c3.abs()) + c2.abs() * 2 * NB.U * xh.abs()
            if dadd_on:
                want = want + aimg.double().reshape(B, HW, C)
            e = e + NB.U * want.abs()
            res = [("y", want.reshape(-1, C), e.reshape(-1, C), "bf16"), ("y_rest", None, None, "zero")]
            if params:
                Lp = NB.L_gn_params(rpc, NB.gn_stats_RT(C), nch, B) + (1 if accumulate else 0)
                t = (gg * xh).view(-1, C)
                wg, eg = NB.colsum(t, Lp, (e_g * xh.abs() + gg.abs() * 2 * NB.U * xh.abs() + NB.U * (gg * xh).abs()).view(-1, C))
                wb, eb = NB.colsum(gg.view(-1, C), Lp, e_g.view(-1, C))
                if accumulate:
                    wg, wb = wg + c0[0].double(), wb + c0[1].double()
                res += [("dgamma", wg, eg, "f32s"), ("dbeta", wb, eb, "f32s")]
            return res

        call = lambda mod, T: mod.groupnorm_bwd(T(dy), T(x), T(gamma), T(beta), T(stats), B, H, W, groups=GN_G, silu=silu, dy_tokens=dy_tokens, dadd=T(dadd),
                                                dgamma=T(dgam), dbeta=T(dbet), accumulate_params=accumulate)
        return Built(call, ref, g, {"dgamma": dgam, "dbeta": dbet} if params else {}, ret=_split_grid(B, H, W))
    return build


CASES.append(Case("groupnorm_bwd_tokens_dadd_params_accumulate", "groupnorm_bwd", "grid", _gn_bwd(5600, True, True, True, True, True),
                  frozenset(("groups", "silu", "dy_tokens", "dadd", "dgamma", "dbeta", "accumulate_params"))))
CASES.append(Case("groupnorm_bwd_grid_params", "groupnorm_bwd", "grid", _gn_bwd(5601, False, False, False, True, False), frozenset(("groups", "silu", "dy_tokens", "dgamma", "dbeta"))))
CASES.append(Case("groupnorm_bwd_grid_plain", "groupnorm_bwd", "grid", _gn_bwd(5602, True, False, False, False, False), frozenset(("groups", "silu"))))


# =============================================================================================================================================================
# q / k RMSNorm + RoPE: hd 128 and 64, H 2, S 96, the 40 positions from 56 on (the second stream of a joint sequence), B 2
# =============================================================================================================================================================
QB, QH, QS, QP0, QSP, QSPAD = 2, 2, 96, 56, 40, 128


def _rope_tables(S, hd):
    freq = 10000.0 ** (-torch.arange(0, hd, 2, dtype=F64) / hd)
    ang = torch.arange(S, dtype=F64)[:, None] * freq[None, :] * 0.37
    return ang.cos().repeat_interleave(2, 1).float().contiguous(), ang.sin().repeat_interleave(2, 1).float().contiguous()


def qk_wgrad_route(B, H, S_part):
    """norm_rope.hip / norm_route.h qk_wgrad_route_slices: (ns, per)"""
    nblk = NB.cdiv(S_part, 64) * H * B
    ns = NB.cdiv(nblk, 32) if nblk < 64 * 32 else 64
    return ns, NB.cdiv(nblk, ns)


def _part_rows(t, B, S, pos0, S_part, c0, c1):
    """columns [c0, c1) of the S_part rows from pos0 of every sample of a [B * S, C] row-major view"""
    ld = t.stride(0)
    return torch.as_strided(t, (B, S_part, c1 - c0), (S * ld, ld, 1), t.storage_offset() + pos0 * ld + c0)


def _hm(rows, H, d):
    """[B, T, H d] rows -> head-major [B, H, T, d]"""
    B, T, _ = rows.shape
    return rows.reshape(B, T, H, d).permute(0, 2, 1, 3)


def _rows_of(hm):
    """head-major [B, H, T, d] -> [B, T, H d]"""
    B, H, T, d = hm.shape
    return hm.permute(0, 2, 1, 3).reshape(B, T, H * d)


def _qk_tables(g, d):
    cs, sn = _rope_tables(QS, d)
    c, s = g.blk(QS, d, dtype=F32), g.blk(QS, d, dtype=F32)
    c.copy_(cs)
    s.copy_(sn)
    return c, s


def _qk_fwd(seed, d, wts, with_t):
    def build():
        g = Gen(seed)
        B, H, S, p0, Sp_, Sp = QB, QH, QS, QP0, QSP, QSPAD
        D = H * d
        qkv = g.mat(B * S, 3 * D, pad=8, scale=1.3, shift=0.1)
        wq, wk = (g.blk(d, scale=0.2, shift=1.0), g.blk(d, scale=0.2, shift=1.0)) if wts else (None, None)
        cs, sn = _qk_tables(g, d)
        Q, K, Vt = g.blk(B, H, S, d), g.blk(B, H, S, d), g.blk(B, H, d, Sp)
        Qt, Kt = (g.blk(B, H, d, Sp), g.blk(B, H, d, Sp)) if with_t else (None, None)
        outs = {"Q": Q[:, :, p0:p0 + Sp_], "K": K[:, :, p0:p0 + Sp_], "Vt": Vt[..., p0:p0 + Sp_]}
        if with_t:
            outs.update(Qt=Qt[..., p0:p0 + Sp_], Kt=Kt[..., p0:p0 + Sp_])
        c4, s4 = cs.double()[None, None, p0:p0 + Sp_], sn.double()[None, None, p0:p0 + Sp_]

        def ref(o):
            res = []
            for j, (w, nm) in enumerate(((wq, "Q"), (wk, "K"))):
                x = _hm(_part_rows(qkv, B, S, p0, Sp_, j * D, (j + 1) * D), H, d).double()
                want, e, _ = NB.qk_fwd(x, None if w is None else w.double(), c4, s4, 1e-6)
                res.append((nm, want, e, "bf16"))
                if with_t:
                    res.append((nm + "t", o[nm].transpose(-1, -2).contiguous(), None, "exact"))
            res.append(("Vt", _hm(_part_rows(qkv, B, S, p0, Sp_, 2 * D, 3 * D), H, d).transpose(-1, -2).contiguous(), None, "exact"))
            return res

        call = lambda mod, T: mod.qk_norm_rope_fwd(T(qkv), T(wq), T(wk), T(cs), T(sn), T(Q), T(K), T(Qt), T(Kt), T(Vt), B, H, d, Sp_, p0, S, Sp, eps=1e-6)
        return Built(call, ref, g, outs)
    return build


CASES.append(Case("qk_norm_rope_fwd_d128_norm_t", "qk_norm_rope_fwd", "qk", _qk_fwd(6000, 128, True, True), frozenset(("eps",))))
CASES.append(Case("qk_norm_rope_fwd_d64_plain", "qk_norm_rope_fwd", "qk", _qk_fwd(6001, 64, False, False), frozenset(("eps",))))


def _qk_bwd(seed, d, wts, wgrad, accumulate=False):
    def build():
        g = Gen(seed)
        B, H, S, p0, Sp_ = QB, QH, QS, QP0, QSP
        D = H * d
        qkv = g.mat(B * S, 3 * D, pad=8, scale=1.3, shift=0.1)
        dqkv = g.mat(B * S, 3 * D, pad=8)
        wq, wk = (g.blk(d, scale=0.2, shift=1.0), g.blk(d, scale=0.2, shift=1.0)) if wts else (None, None)
        cs, sn = _qk_tables(g, d)
        dQ, dK = g.blk(B, H, S, d, scale=0.5, shift=0.05), g.blk(B, H, S, d, scale=0.5, shift=0.05)
        gw = [g.blk(d, scale=5.0), g.blk(d, scale=5.0)] if wgrad else [None, None]
        c0 = [t.clone() for t in gw] if wgrad else None
        outs = {"dqk": _part_rows(dqkv, B, S, p0, Sp_, 0, 2 * D)}
        if wgrad:
            outs.update(gwq=gw[0], gwk=gw[1])
        c4, s4 = cs.double()[None, None, p0:p0 + Sp_], sn.double()[None, None, p0:p0 + Sp_]

        def ref(o):
            wants, es, res = [], [], []
            for j, (w, gI, nm) in enumerate(((wq, dQ, "gwq"), (wk, dK, "gwk"))):
                x = _hm(_part_rows(qkv, B, S, p0, Sp_, j * D, (j + 1) * D), H, d).double()
                want, e, dy, e_dy, r, e_r = NB.qk_bwd(gI[:, :, p0:p0 + Sp_].double(), x, None if w is None else w.double(), c4, s4, 1e-6)
                wants.append(_rows_of(want))
                es.append(_rows_of(e))
                if wgrad:
                    ns, per = qk_wgrad_route(B, H, Sp_)
                    t = dy * x * r
                    ww, ee = NB.colsum(t.reshape(-1, d), NB.L_qk_wgrad(d, ns, per) + 1, (x.abs() * r * e_dy + t.abs() * (e_r + 2 * NB.U)).reshape(-1, d))
                    if accumulate:
                        ww = ww + c0[j].double()
                    res.append((nm, ww, ee + NB.U * ww.abs(), "bf16e"))
            return [("dqk", torch.cat(wants, -1), torch.cat(es, -1), "bf16")] + res

        if wgrad:
            call = lambda mod, T: mod.qk_norm_rope_bwd_wgrad(T(dQ), T(dK), T(qkv), T(wq), T(wk), T(cs), T(sn), T(dqkv), B, H, d, Sp_, p0, S, T(gw[0]), T(gw[1]),
                                                             accumulate=accumulate, eps=1e-6)
        else:
            call = lambda mod, T: mod.qk_norm_rope_bwd(T(dQ), T(dK), T(qkv), T(wq), T(wk), T(cs), T(sn), T(dqkv), B, H, d, Sp_, p0, S, eps=1e-6)
        return Built(call, ref, g, outs)
    return build


CASES.append(Case("qk_norm_rope_bwd_d128_norm", "qk_norm_rope_bwd", "qk", _qk_bwd(6100, 128, True, False), frozenset(("eps",))))
CASES.append(Case("qk_norm_rope_bwd_d64_plain", "qk_norm_rope_bwd", "qk", _qk_bwd(6101, 64, False, False), frozenset(("eps",))))
CASES.append(Case("qk_norm_rope_bwd_wgrad_d128_accumulate", "qk_norm_rope_bwd_wgrad", "qk", _qk_bwd(6102, 128, True, True, True), frozenset(("eps", "accumulate"))))
CASES.append(Case("qk_norm_rope_bwd_wgrad_d64", "qk_norm_rope_bwd_wgrad", "qk", _qk_bwd(6103, 64, True, True, False), frozenset(("eps",))))


def _qk_rope_norm_bwd(seed, wts):
    """from the roped head-major Q / K and the saved 1 / rms, as the fused projection epilogue leaves them (here: given operands); head_dim 128"""
    def build():
        g = Gen(seed)
        B, H, S, p0, Sp_, d = QB, QH, QS, QP0, QSP, 128
        D = H * d
        dqkv = g.mat(B * S, 3 * D, pad=8)
        wq, wk = (g.blk(d, scale=0.2, shift=1.0), g.blk(d, scale=0.2, shift=1.0)) if wts else (None, None)
        cs, sn = _qk_tables(g, d)
        Q, K = g.blk(B, H, S, d), g.blk(B, H, S, d)
        dQ, dK = g.blk(B, H, S, d, scale=0.5), g.blk(B, H, S, d, scale=0.5)
        rrms = g.blk(B * S, 2 * H, dtype=F32, scale=0.1, shift=0.9)
        c4, s4 = cs.double()[None, None, p0:p0 + Sp_], sn.double()[None, None, p0:p0 + Sp_]

        def ref(o):
            wants, es = [], []
            for part, (w, gI, z) in enumerate(((wq, dQ, Q), (wk, dK, K))):
                rr = rrms.view(B, S, 2, H)[:, p0:p0 + Sp_, part].permute(0, 2, 1).double()[..., None] if w is not None else None
                want, e = NB.qk_rope_norm_bwd(gI[:, :, p0:p0 + Sp_].double(), z[:, :, p0:p0 + Sp_].double(), rr, None if w is None else w.double(), c4, s4)
                wants.append(_rows_of(want))
                es.append(_rows_of(e))
            return [("dqk", torch.cat(wants, -1), torch.cat(es, -1), "bf16")]

        call = lambda mod, T: mod.qk_rope_norm_bwd(T(dQ), T(dK), T(Q), T(K), T(rrms), T(wq), T(wk), T(cs), T(sn), T(dqkv), B, H, d, Sp_, p0, S)
        return Built(call, ref, g, {"dqk": _part_rows(dqkv, B, S, p0, Sp_, 0, 2 * D)})
    return build


CASES.append(Case("qk_rope_norm_bwd_norm", "qk_rope_norm_bwd", "qk", _qk_rope_norm_bwd(6200, True), frozenset()))
CASES.append(Case("qk_rope_norm_bwd_plain", "qk_rope_norm_bwd", "qk", _qk_rope_norm_bwd(6201, False), frozenset()))


# =============================================================================================================================================================
# attention: self B 1, H 2, S 160 (Sp 192), d 128 and 64; cross Sq 96, Sk 77 (both padded to 128)
# =============================================================================================================================================================
def _tok(hm):
    """head-major [B, H, S, d] -> token-major [B S, H d]"""
    B, H, S, d = hm.shape
    return hm.permute(0, 2, 1, 3).reshape(B * S, H * d)


def _bhsd(B, H, S, d):
    return lambda t: t.reshape(B, S, H, d).permute(0, 2, 1, 3)


def _attn_operands(g, B, H, Sq, Sk, d, bias):
    Skp = (Sk + 63) // 64 * 64
    Q, K = g.blk(B, H, Sq, d, scale=0.5), g.blk(B, H, Sk, d, scale=0.5)
    v_rows = g.mat(B * Sk, H * d, pad=40)
    Vt = g.blk(B, H, d, Skp)
    Vt.zero_()                                  # the columns beyond Sk are the caller's to zero
    Vt[..., :Sk] = v_rows.reshape(B, Sk, H, d).permute(0, 2, 3, 1)
    kb = None
    if bias:
        kb = g.blk(B, Sk, dtype=F32)
        kb.zero_()
        kb[0, Sk - 50:] = -3.0
    return Q, K, v_rows, Vt, kb, Skp


def _attn_fwd(seed, fn, d, bias, res, Sq=160, Sk=160):
    def build():
        g = Gen(seed)
        B, H = 1, 2
        Q, K, v_rows, Vt, kb, Skp = _attn_operands(g, B, H, Sq, Sk, d, bias)
        if fn == "attn_fwd":
            Skp = 192                           # Sp 192: one more 64-column tile than S needs
            Vt = g.blk(B, H, d, Skp)
            Vt.zero_()
            Vt[..., :Sk] = v_rows.reshape(B, Sk, H, d).permute(0, 2, 3, 1)
        O, lse2 = g.mat(B * Sq, H * d, pad=32), g.blk(B, H, Sq, dtype=F32)
        O_res = g.mat(B * Sq, H * d, pad=32) if res else None
        scale = d ** -0.5
        outs = {"O": O, "lse2": lse2}
        if res:
            outs["O_res"] = O_res
        if fn == "attn_fwd":
            call = lambda mod, T: mod.attn_fwd(T(Q), T(K), T(Vt), T(O), T(lse2), B, H, Sq, Skp, d, scale, key_bias=T(kb), O_res=T(O_res))
        elif fn == "attn_cross_fwd":
            call = lambda mod, T: mod.attn_cross_fwd(T(Q), T(K), T(Vt), T(O), T(lse2), B, H, Sq, Sk, Skp, d, scale, key_bias=T(kb), O_res=T(O_res))
        else:
            call = lambda mod, T: mod.attn_fwd_vrows(T(Q), T(K), T(v_rows), T(O), T(lse2), B, H, Sq, d, scale, key_bias=T(kb))

        def ref(o):
            f = AB.attn_fwd_model(Q, K, _bhsd(B, H, Sk, d)(v_rows), scale, bias=kb)
            hm = _bhsd(B, H, Sq, d)
            res_ = [("O", _tok(f.O), _tok(f.e_O), "attn", {"var": _tok(f.var_O), "to_bhsd": hm}), ("lse2", f.lse2, f.e_lse2, "lse2")]
            if res:          # O + O_res carries the fp32 output (one fp32 rounding, u |O|); the final RNE is the residual's (tests/test_attn_bounds_gpu.py)
                Oh = o["O"].double()
                res_.append(("O_plus_res", _tok(f.O), _tok(f.e_O + AB.U24 * f.O.abs()), "attn",
                             {"var": _tok(f.var_O), "to_bhsd": hm, "out": Oh + o["O_res"].double(), "final": _tok(f.O) - Oh}))
            return res_

        return Built(call, ref, g, outs)
    return build


for _i, (_d, _b, _r) in enumerate(((128, False, False), (128, True, True), (64, True, False), (64, False, True))):
    CASES.append(Case(f"attn_fwd_d{_d}_bias{int(_b)}_res{int(_r)}", "attn_fwd", "attention", _attn_fwd(7000 + _i, "attn_fwd", _d, _b, _r),
                      frozenset(k for k, on in (("key_bias", _b), ("O_res", _r)) if on)))
CASES.append(Case("attn_cross_fwd_bias", "attn_cross_fwd", "attention", _attn_fwd(7010, "attn_cross_fwd", 64, True, False, Sq=96, Sk=77), frozenset(("key_bias",))))
CASES.append(Case("attn_cross_fwd_res", "attn_cross_fwd", "attention", _attn_fwd(7011, "attn_cross_fwd", 64, False, True, Sq=96, Sk=77), frozenset(("O_res",))))
CASES.append(Case("attn_fwd_vrows", "attn_fwd_vrows", "attention", _attn_fwd(7020, "attn_fwd_vrows", 128, False, False), frozenset()))
CASES.append(Case("attn_fwd_vrows_bias", "attn_fwd_vrows", "attention", _attn_fwd(7021, "attn_fwd_vrows", 128, True, False), frozenset(("key_bias",))))


def _attn_bwd(seed, cross, d, bias, res):
    """the backward from a forward's stored O (+ O_res) and lse2, here the roundings of the fp64 forward.  The dK / dV score chains and the dQ tail depend on the
    route: the device's plan (ops.attn_plan) says which where the module has one; the emulator has no route (the plain chain)"""
    def build():
        g = Gen(seed)
        B, H = 1, 2
        Sq, Sk = (96, 77) if cross else (160, 160)
        Q, K, v_rows, Vt, kb, Skp = _attn_operands(g, B, H, Sq, Sk, d, bias)
        Sqp = (Sq + 63) // 64 * 64
        if not cross:
            Skp = Sqp = 192
        scale = d ** -0.5
        hq, hk = _bhsd(B, H, Sq, d), _bhsd(B, H, Sk, d)
        f = AB.attn_fwd_model(Q, K, hk(v_rows), scale, bias=kb)
        O, dO = g.mat(B * Sq, H * d, pad=32), g.mat(B * Sq, H * d, pad=8)
        O.copy_(_tok(f.O).float().to(BF16))
        O_res = None
        if res:
            O_res = g.mat(B * Sq, H * d, pad=32)
            O_res.copy_((_tok(f.O) - O.double()).float().to(BF16))
        lse2 = g.blk(B, H, Sq, dtype=F32)
        lse2.copy_(f.lse2.float())
        dQ, dK, dv = g.blk(B, H, Sq, d), g.blk(B, H, Sk, d), g.mat(B * Sk, H * d, pad=40)
        route = {"lse_in_chain": False, "tail_from": None}

        def call(mod, T):
            if hasattr(mod, "attn_plan"):
                plan = mod.attn_plan(B, H, Sq, Sk, d, key_bias=bias, O_res=res)
                route.update(lse_in_chain=plan["dkv"].startswith("dkv4"), tail_from=Sk // 64 * 64 if plan["dq_tail"] else None)
            if cross:
                return mod.attn_cross_bwd(T(Q), T(K), None, None, T(v_rows), T(O), T(dO), T(lse2), T(dQ), T(dK), T(dv), B, H, Sq, Sqp, Sk, Skp, d, scale,
                                          key_bias=T(kb), O_res=T(O_res))
            return mod.attn_bwd(T(Q), T(K), None, None, T(v_rows), T(O), T(dO), T(lse2), T(dQ), T(dK), T(dv), B, H, Sq, Skp, d, scale, key_bias=T(kb), O_res=T(O_res))

        def ref(o):
            bw = AB.attn_bwd_model(Q, K, hk(v_rows), hq(dO), hq(O), lse2, scale, bias=kb, O_res=hq(O_res) if res else None, **route)
            ident = lambda t: t
            exq = {"var": bw.var_dQ, "to_bhsd": ident}
            r = [("dK", bw.dK, bw.e_dK, "attn", {"var": bw.var_dK, "to_bhsd": ident}),
                 ("dV", _tok(bw.dV), _tok(bw.e_dV), "attn", {"var": _tok(bw.var_dV), "to_bhsd": hk})]
            if bw.dQ_part is not None:          # dq64 + tail: the partial over the full key tiles is rounded once more (attn_bounds.check extra_round)
                e_q = bw.e_dQ + 0.5 * AB.ulp_bf16(bw.dQ_part.abs() + bw.e_dQ)
                exq["var"] = bw.var_dQ + AB.ulp_bf16(bw.dQ_part) ** 2 / 12
                return [("dQ", bw.dQ, e_q, "attn", exq)] + r
            return [("dQ", bw.dQ, bw.e_dQ, "attn", exq)] + r

        return Built(call, ref, g, {"dQ": dQ, "dK": dK, "dV": dv})
    return build


for _i, (_d, _b, _r) in enumerate(((128, False, False), (128, True, True), (64, True, False), (64, False, True))):
    CASES.append(Case(f"attn_bwd_d{_d}_bias{int(_b)}_res{int(_r)}", "attn_bwd", "attention", _attn_bwd(7100 + _i, False, _d, _b, _r),
                      frozenset(k for k, on in (("key_bias", _b), ("O_res", _r)) if on)))
CASES.append(Case("attn_cross_bwd_bias", "attn_cross_bwd", "attention", _attn_bwd(7110, True, 64, True, False), frozenset(("key_bias",))))
CASES.append(Case("attn_cross_bwd_res", "attn_cross_bwd", "attention", _attn_bwd(7111, True, 64, False, True), frozenset(("O_res",))))


@case("attn_bwd_rope", "attention", opts=("key_bias",))
def _attn_bwd_rope():
    """attention backward with the RoPE + RMSNorm backward in the dQ / dK epilogues: S 160, the norm weights change at joint position 56; the stored-dQ / dK bound
    is carried through the epilogue's Jacobian (attn_bounds.rope_norm_bwd_model), as tests/test_attn_bounds_gpu.py does"""
    g = Gen(7200)
    B, H, S, Sp, d, split = 1, 2, 160, 192, 128, 56
    D = H * d
    Q, K, v_rows, Vt, kb, _ = _attn_operands(g, B, H, S, S, d, True)
    scale = d ** -0.5
    hm = _bhsd(B, H, S, d)
    f = AB.attn_fwd_model(Q, K, hm(v_rows), scale, bias=kb)
    O, dO = g.mat(B * S, D, pad=32), g.mat(B * S, D, pad=8)
    O.copy_(_tok(f.O).float().to(BF16))
    lse2 = g.blk(B, H, S, dtype=F32)
    lse2.copy_(f.lse2.float())
    rrms = g.blk(B * S, 2 * H, dtype=F32)
    rrms.copy_(torch.rand(B * S, 2 * H, generator=g.g) * 1.5 + 0.5)
    w = [g.blk(d, scale=0.2, shift=1.0) for _ in range(4)]          # wq_lo, wk_lo, wq_hi, wk_hi
    ang = torch.rand(S, 64, generator=g.g) * (2 * math.pi)
    cos_p, sin_p = g.blk(S, 64, dtype=F32), g.blk(S, 64, dtype=F32)
    cos_p.copy_(torch.cos(ang))
    sin_p.copy_(torch.sin(ang))
    dqkv = g.mat(B * S, 3 * D, pad=64)
    route = {"lse_in_chain": False, "tail_from": None}

    def call(mod, T):
        if hasattr(mod, "attn_plan"):
            plan = mod.attn_plan(B, H, S, S, d, key_bias=True, rope=True)
            route.update(lse_in_chain=plan["dkv"].startswith("dkv4"), tail_from=S // 64 * 64 if plan["dq_tail"] else None)
        return mod.attn_bwd_rope(T(Q), T(K), T(v_rows), T(O), T(dO), T(lse2), T(rrms), T(w[0]), T(w[1]), T(w[2]), T(w[3]), split, T(cos_p), T(sin_p), T(dqkv),
                                 B, H, S, Sp, d, scale, key_bias=T(kb))

    def ref(o):
        bw = AB.attn_bwd_model(Q, K, hm(v_rows), hm(dO), hm(O), lse2, scale, bias=kb, **route)
        pos = torch.arange(S)[:, None] < split
        rr = rrms.view(B, S, 2, H).permute(0, 2, 3, 1)
        wants, es, vs = [], [], []
        for n, z, i in (("dQ", Q, 0), ("dK", K, 1)):
            wtok = torch.where(pos, w[i].float()[None], w[i + 2].float()[None])[None, None].expand(B, H, S, 128)
            tg, vg = AB.stored_tol_var(getattr(bw, n), getattr(bw, "e_" + n), getattr(bw, "var_" + n))
            if n == "dQ" and bw.dQ_part is not None:
                tg, vg = tg + 0.5 * AB.ulp_bf16(bw.dQ_part.abs() + bw.e_dQ), vg + AB.ulp_bf16(bw.dQ_part) ** 2 / 12
            a, b, c = AB.rope_norm_bwd_model(getattr(bw, n), tg, vg, z, rr[:, i], wtok, cos_p, sin_p)
            wants.append(_tok(a)); es.append(_tok(b)); vs.append(_tok(c))
        wants.append(_tok(bw.dV)); es.append(_tok(bw.e_dV)); vs.append(_tok(bw.var_dV))
        to = lambda t: t.reshape(B, S, 3 * H, d).permute(0, 2, 1, 3)          # the 3 H column blocks of 128 as heads
        return [("dqkv", torch.cat(wants, 1), torch.cat(es, 1), "attn", {"var": torch.cat(vs, 1), "to_bhsd": to})]

    return Built(call, ref, g, {"dqkv": dqkv})


def _rope_abs(v, cs, sn):
    """|R| v for the interleaved pair rotation with one angle per pair: cs / sn [T, d / 2] broadcast over [B, H, T, d]"""
    c, s = cs.abs(), sn.abs()
    v0, v1 = v[..., 0::2], v[..., 1::2]
    return torch.stack([v0 * c + v1 * s, v1 * c + v0 * s], -1).flatten(-2)


@case("qk_rope", "gemm", name="qk_rope_struct", opts=("eps", "Vt"))
def _gemm_qk_norm_rope():
    """EPI_QK_NORM_ROPE through ops.qk_rope: M 256 rows of one sample at joint position 64 of S 320, H 2 heads of 128, K 192 (the epilogue's preconditions:
    rows_per_batch a multiple of 256, head_dim 128, even H, N = 3 H 128).  The bound is derived here from the kernel's arithmetic (gemm.hip epilogue): the fp32
    accumulator x carries the GEMM bound s; r = rsqrt(mean x^2 + eps) then moves by (2 / hd) sum |x| s / (mean x^2 + eps) / 2 + the 128-term fp32 sum + rsqrtf
    (norm_bounds.rms_stats); y = x r w by |r w| s + |y| (e_r + 3 u); the pair rotation adds 3 u of its two terms; one RNE at the store"""
    L = _lib()
    g = Gen(1150)
    B, H, S, R, p0, hd, eps = 1, 2, 320, 256, 64, 128, 1e-6
    D = H * hd
    a, w, bias = g.mat(R, GK), g.mat(3 * D, GK, scale=0.08), g.blk(3 * D, scale=0.1)
    wq, wk = g.blk(hd, scale=0.2, shift=1.0), g.blk(hd, scale=0.2, shift=1.0)
    Q, K, Vt = g.blk(B, H, S, hd), g.blk(B, H, S, hd), g.blk(B, H, hd, S)
    rrms = g.blk(B * S * 2 * H, dtype=F32)
    ang = torch.arange(S, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(0, hd, 2, dtype=F64) / hd))[None] * 0.37
    cos_p, sin_p = g.blk(S, 64, dtype=F32), g.blk(S, 64, dtype=F32)
    cos_p.copy_(ang.cos().float())
    sin_p.copy_(ang.sin().float())
    out = g.mat(R, D, pad=8)
    rr_view = rrms.view(B, S, 2 * H)[:, p0:p0 + R]
    outs = {"Q": Q[:, :, p0:p0 + R], "K": K[:, :, p0:p0 + R], "Vt": Vt[..., p0:p0 + R], "rrms": rr_view, "out": out}

    def call(mod, T):
        rope = mod.qk_rope(T(Q), T(K), T(rrms), T(wq), T(wk), T(cos_p), T(sin_p), H, S, p0, eps=eps, Vt=T(Vt))
        return mod.gemm(T(a), T(w), bias=T(bias), out=T(out), epilogue=L.EPI_QK_NORM_ROPE, rope=rope, rows_per_batch=R)

    def ref(o):
        acc = GB.gemm_ref(a, w, None, None, bias)
        cs, sn = cos_p.double()[p0:p0 + R], sin_p.double()[p0:p0 + R]
        c2, s2 = cs.repeat_interleave(2, 1)[None, None], sn.repeat_interleave(2, 1)[None, None]
        res, rs, ers = [], [], []
        for j, (wt, nm) in enumerate(((wq, "Q"), (wk, "K"))):
            x = _hm(acc.ref[:, j * D:(j + 1) * D].reshape(B, R, D), H, hd)
            s = _hm(acc.s[:, j * D:(j + 1) * D].reshape(B, R, D), H, hd)
            ms = (x * x).mean(-1, keepdim=True)
            r, e_r = NB.rms_stats(x, eps, hd)
            e_r = e_r + 0.5 * (2.0 / hd) * (x.abs() * s).sum(-1, keepdim=True) / (ms + eps)
            wd = wt.double()
            y = x * r * wd
            e_y = (r * wd).abs() * s + y.abs() * (e_r + 3 * U)
            z, m = NB.rope_pairs(y, c2, s2)
            res.append((nm, z, _rope_abs(e_y, cs[None, None], sn[None, None]) + 3 * U * m, "bf16"))
            rs.append(r[..., 0].permute(0, 2, 1))
            ers.append((r * e_r)[..., 0].permute(0, 2, 1))
        res.append(("rrms", torch.cat(rs, -1), torch.cat(ers, -1), "f32"))
        res.append(("out", acc.ref[:, 2 * D:], acc.s[:, 2 * D:], "bf16"))
        res.append(("Vt", _hm(o["out"].reshape(B, R, D), H, hd).transpose(-1, -2).contiguous(), None, "exact"))
        return res

    return Built(call, ref, g, outs, same="out")


CASES.append(Case("gemm_qk_norm_rope", "gemm", "gemm", _gemm_qk_norm_rope, frozenset(("rope", "rows_per_batch"))))

"""The kernels called between the large families — activations / add, scale_cols, the stand-alone GEGLU, the row softmax and its backward, the timestep projection,
the TREAD gather / scatter, the bf16 transpose and the fp8 quantisers — element-wise against an fp64 reference of the same stored inputs (tests/ew_bounds.py), or
bit for bit where the operation is exact (scale_cols, the copies, the quantisers against oracle.train_math on the CPU).

Every case runs twice and must be bit-identical, prefills its outputs with the sentinel and asserts that everything outside the region the call owns keeps its
bits; where the ops wrapper allocates its own output the case calls the C ABI with guarded buffers.  The last tests assert that the cases launched all six
k_softmax_rows instantiations and the fp8 activation paths and loop passes, and print the worst ratios per family: run the module as a whole."""
import math

import pytest
import torch

from tests import ew_bounds as EB
from tests import gemm_bounds as GB
from tests import step_bounds as SB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U8 = torch.uint8
SENT = 73728.0           # the suite's sentinel (step_bounds' tests): exact in bf16 and fp32, far from every value these kernels produce
SENT_U8 = 0xA5           # byte buffers (fp8 bytes) cannot hold it: a byte pattern instead; what lies inside the owned region is compared with the oracle
PAD = 64                 # guard elements on both sides of every arena (a multiple of 8: 16-byte alignment)
HIT = set()
WORST = {}
ALL_HIT = {f"softmax<{m}>" for m in EB.SOFTMAX_MAXC} | {"fp8_act|dense", "fp8_act|strided", "fp8_act|odd tail", "fp8_act|absmax grid-stride dense", "fp8_act|quant grid-stride dense",
                                                              "fp8_act|absmax grid-stride strided", "fp8_act|quant grid-stride strided"}
GRID = 2048 * 256        # the element-wise grid cap in threads (ew_blocks); fp8_quantize_act's cap is the same


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from simpletuner_amd import lib as _l

    L = _l.load()

    def call(name, *args):
        _l.check(getattr(L, name)(torch.cuda.current_stream().cuda_stream, *args), name)
        torch.cuda.synchronize()
    return call


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=dev(), generator=g) * scale).to(BF16)


def _note(family, rep):
    w = WORST.setdefault(family, {"err/tol": 0.0, "block": 0.0})
    w["err/tol"] = max(w["err/tol"], rep.worst)
    w["block"] = max(w["block"], rep.block_rms)
    GB.assert_bound(rep)


class Arena:
    """a [rows, cols] view with row stride ld inside a sentinel-filled flat buffer with PAD guard elements on both sides (more in front with `off`)"""

    def __init__(self, rows, cols, ld=None, dtype=BF16, data=None, off=0):
        ld = cols if ld is None else ld
        sent = SENT_U8 if dtype == U8 else SENT
        lo = PAD + off
        self.buf = torch.full((lo + rows * ld + PAD,), sent, dtype=dtype, device=dev())
        self.view = self.buf[lo:lo + rows * ld].view(rows, ld)[:, :cols]
        self.own = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev())
        self.own[lo:lo + rows * ld].view(rows, ld)[:, :cols] = True
        self.ld, self.sent = ld, sent
        if data is not None:
            self.view.copy_(data)
        self.prior = self.buf.clone()

    def ptr(self):
        return self.view.data_ptr()

    def reset(self):
        self.buf.copy_(self.prior)

    def snap(self):
        return self.buf.clone()

    def outside_ok(self, what):
        assert torch.equal(self.buf[~self.own], self.prior[~self.own]), f"{what}: wrote outside the region it owns"

    def unchanged(self, what):
        assert torch.equal(self.buf, self.prior), f"{what}: an input was written"

    def all_written(self, what):
        assert not bool((self.view == self.sent).any()), f"{what}: elements left at the sentinel"


def _twice(run, outs, what, ins=()):
    """run() twice from the same prior state: bit-identical buffers, nothing outside the owned regions touched, inputs unchanged"""
    run()
    first = [o.snap() for o in outs]
    for o in outs:
        o.reset()
    run()
    for o, f in zip(outs, first):
        assert torch.equal(o.buf, f), f"{what}: two runs differ"
        o.outside_ok(what)
    for i in ins:
        i.unchanged(what)


# ------------------------------------------------------------------------------------------------
# activations and add
# ------------------------------------------------------------------------------------------------
def _act_inputs(seed, n):
    """randn * 3 with every eighth element uniform in [-80, 80]"""
    g = _gen(seed)
    x = torch.randn(n, device=dev(), generator=g) * 3
    x[::8] = torch.rand(x[::8].shape, device=dev(), generator=g) * 160 - 80
    return x.to(BF16), _randn(g, n)


def _act_call(lib, op, a, b):
    """the C ABI on guarded flat buffers; returns the output arena"""
    n = a.numel()
    A, Bv, Y = Arena(1, n, data=a), Arena(1, n, data=b), Arena(1, n)
    run = {"silu": lambda: lib("st355_silu", A.ptr(), Y.ptr(), n), "gelu_tanh": lambda: lib("st355_gelu_tanh", A.ptr(), Y.ptr(), n),
           "add": lambda: lib("st355_add", A.ptr(), Bv.ptr(), Y.ptr(), n), "silu_bwd": lambda: lib("st355_silu_bwd", A.ptr(), Bv.ptr(), Y.ptr(), n)}[op]
    _twice(run, [Y], f"{op} n={n}", ins=[A, Bv])
    return Y


ACT_REF = {"silu": lambda a, b: EB.silu(a), "gelu_tanh": lambda a, b: EB.gelu_tanh(a), "add": lambda a, b: EB.add(a, b), "silu_bwd": lambda a, b: EB.silu_bwd(a, b)}
ACT_N = [3, 8 * 1000 + 5, 4194304 + 8 * 300 + 5]          # tail only; vectors + tail; past 2048 x 256 vectors: a second grid-stride pass, and the tail


@pytest.mark.parametrize("op", ["silu", "silu_bwd", "gelu_tanh", "add"])
@pytest.mark.parametrize("n", ACT_N)
def test_activations_and_add(lib, op, n):
    assert (n // 8 > GRID) == (n == ACT_N[2])
    a, b = _act_inputs(n, n)
    Y = _act_call(lib, op, a, b)
    Y.all_written(f"{op} n={n}")
    want, e = ACT_REF[op](a, b)
    out = Y.view.reshape(-1)
    _note(op, EB.check_elem(f"{op} n={n}", out, want, e) if n == 3 else EB.check_bf16(f"{op} n={n}", out, want, e, flat=True))


@pytest.mark.parametrize("op", ["silu", "silu_bwd", "gelu_tanh", "add"])
def test_activation_edge_vector(lib, op):
    """+-0, +-2^-126, +-80, +-89, +-1e4, +-3e38 (n = 12: one vector and a tail of 4): finite, the right sign, never larger than the correctly rounded reference,
    and for x >= 80 (the identity side) exactly its bits; the elements with |x| <= 80 also keep the main bound"""
    a = EB.edge_vector(dev())
    b = (-0.5 * a.float()).to(BF16) if op == "add" else torch.full_like(a, 0.75)
    Y = _act_call(lib, op, a, b)
    out = Y.view.reshape(-1)
    want, e = ACT_REF[op](a, b)
    ok = EB.edge_ok(out, want)
    print(f"[edge] {op}: x = {a.float().tolist()}\n[edge] {op}: out = {out.float().tolist()}")
    assert bool(ok.all()), (op, a[~ok].float().tolist(), out[~ok].float().tolist())
    exact = EB.edge_exact(a, out, want)
    assert bool(exact.all()), (op, "x >= 80: not the rounded reference's bits", a[~exact].float().tolist(), out[~exact].float().tolist())
    main = a.float().abs() <= 80
    _note(op, EB.check_elem(f"{op} edge |x| <= 80", out[main], want[main], e[main]))


# ------------------------------------------------------------------------------------------------
# scale_cols
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rpb", [(192, 520, 96), (192, 520, 1), (8160, 520, 96), (8160, 520, 1)])
def test_scale_cols_is_one_rne_of_an_exact_product(lib, M, N, rpb):
    """ld_in > N, ld_out > N, the gate a column slice of a wider buffer, rows_per_batch 96 and 1; 8160 x 520 / 8 = 530 400 vectors: a second grid-stride pass"""
    assert (M * N // 8 > GRID) == (M == 8160)
    g = _gen(M + rpb)
    nb = M // rpb
    X = Arena(M, N, ld=N + 8, data=_randn(g, M, N, scale=3.0))
    G = Arena(nb, N, ld=N + 24, data=_randn(g, nb, N), off=8)
    Y = Arena(M, N, ld=N + 16)
    _twice(lambda: lib("st355_scale_cols", X.ptr(), X.ld, G.ptr(), G.ld, rpb, Y.ptr(), Y.ld, M, N), [Y], f"scale_cols M={M} rpb={rpb}", ins=[X, G])
    want = GB.to_bf16_rne(X.view.float() * G.view.float().repeat_interleave(rpb, 0))
    assert torch.equal(SB.bits(Y.view), SB.bits(want)), f"scale_cols M={M} rpb={rpb}: not one RNE of the exact product"


# ------------------------------------------------------------------------------------------------
# GEGLU
# ------------------------------------------------------------------------------------------------
GEGLU_SHAPES = [(70, 40), (2050, 2056)]          # 2050 x 257 = 526 850 vectors: a second grid-stride pass


def _geglu_inputs(seed, M, F_):
    g = _gen(seed)
    h = _randn(g, M, 2 * F_)
    h[:, F_:] = _randn(g, M, F_, scale=3.0)          # gates at three sigma: the tail below g = -5 is present
    return Arena(M, 2 * F_, ld=2 * F_ + 16, data=h), _randn(g, M, F_)


@pytest.mark.parametrize("M,F_", GEGLU_SHAPES)
def test_geglu_fwd(lib, M, F_):
    assert (M * F_ // 8 > GRID) == (M == 2050)
    H, _ = _geglu_inputs(M, M, F_)
    assert bool((H.view[:, F_:].float() < -5).any())
    Y = Arena(M, F_)
    _twice(lambda: lib("st355_geglu_fwd", H.ptr(), H.ld, Y.ptr(), M, F_), [Y], f"geglu_fwd M={M} F={F_}", ins=[H])
    Y.all_written("geglu_fwd")
    want, e = EB.geglu_fwd(H.view, F_)
    print(f"[geglu] block statistic over all elements, the tail below g = -5 included: {GB.check('geglu_fwd', Y.view, want, e, verbose=False).block_rms:.3f}")
    _note("geglu_fwd", EB.check_geglu(f"geglu_fwd M={M} F={F_} ldh={H.ld}", Y.view, want, e, H.view[:, F_:]))


@pytest.mark.parametrize("M,F_", GEGLU_SHAPES)
def test_geglu_bwd(lib, M, F_):
    H, d = _geglu_inputs(M + 1, M, F_)
    D = Arena(M, F_, data=d)
    DH = Arena(M, 2 * F_, ld=2 * F_ + 8)
    _twice(lambda: lib("st355_geglu_bwd", H.ptr(), H.ld, D.ptr(), DH.ptr(), DH.ld, M, F_), [DH], f"geglu_bwd M={M} F={F_}", ins=[H, D])
    DH.all_written("geglu_bwd")
    want, e = EB.geglu_bwd(H.view, d, F_)
    print(f"[geglu] block statistic over all elements, the tail below g = -5 included: {GB.check('geglu_bwd', DH.view, want, e, verbose=False).block_rms:.3f}")
    _note("geglu_bwd", EB.check_geglu(f"geglu_bwd M={M} F={F_} ldh={H.ld} lddh={DH.ld}", DH.view, want, e, H.view[:, F_:]))


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
SM_CASES = [(8, 67), (2040, 67), (2056, 67), (4104, 67), (8200, 3), (16392, 3), (32776, 3), (65536, 3)]


def _softmax(lib, x, scale, ldx):
    rows, n = x.shape
    X = Arena(rows, n, ld=ldx, data=x)
    _twice(lambda: lib("st355_softmax_rows", X.ptr(), X.ld, rows, n, scale), [X], f"softmax_rows n={n} ldx={ldx}")
    HIT.add(f"softmax<{EB.softmax_maxc(n)}>")
    return X.view


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n,rows", SM_CASES)
def test_softmax_rows(lib, n, rows, strided):
    x = _randn(_gen(n), rows, n, scale=3.0)
    want, e = EB.softmax_rows(x, 0.7)
    v = x.to(F64) * SB.f32(0.7)
    assert float((v - v.amax(1, keepdim=True)).min()) >= -80
    out = _softmax(lib, x, 0.7, n + 64 if strided else n)
    _note("softmax_rows", EB.check_bf16(f"softmax_rows n={n} rows={rows} MAXC={EB.softmax_maxc(n)} {'ldx=n+64' if strided else 'dense'}", out, want, e))


def test_softmax_rows_small(lib):
    n = 264
    eq = torch.full((2, n), 1.375, dtype=BF16, device=dev())
    out = _softmax(lib, eq, 0.7, n + 64)
    _note("softmax_rows small", EB.check_elem("softmax all-equal", out, *EB.softmax_rows(eq, 0.7)))
    assert torch.equal(SB.bits(out), SB.bits(torch.full((2, n), 1.0 / n, device=dev()).to(BF16))), "softmax of equal scores is not 1 / n"
    for scale, flush in ((1.0, False), (1.5, True)):          # z = -60: the rest are 8.8e-27; z = -90: below the smallest normal, may be flushed
        one = torch.zeros(2, n, dtype=BF16, device=dev())
        one[0, 5] = 60.0
        one[1, n - 1] = 60.0
        out = _softmax(lib, one, scale, n)
        _note("softmax_rows small", EB.check_elem(f"softmax one element 60 above the rest, scale {scale}", out, *EB.softmax_rows(one, scale, flush=flush)))
    vae = _randn(_gen(9), 3, 4104, scale=40.0)
    s = 1.0 / math.sqrt(512.0)
    out = _softmax(lib, vae, s, 4104)
    _note("softmax_rows small", EB.check_elem("softmax VAE form (1 / sqrt(512) on randn * 40)", out, *EB.softmax_rows(vae, s)))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n,rows", [(8, 67), (2040, 67), (2056, 67), (16384, 3), (20488, 3)])
def test_softmax_rows_bwd(lib, n, rows, strided):
    g = _gen(100 + n)
    p = torch.softmax(_randn(g, rows, n, scale=3.0).float() * 0.7, 1).to(BF16)          # a real softmax output as stored in bf16
    dp = _randn(g, rows, n)
    ld = n + 64 if strided else n
    P, DP = Arena(rows, n, ld=ld, data=p), Arena(rows, n, ld=ld, data=dp)
    _twice(lambda: lib("st355_softmax_rows_bwd", P.ptr(), DP.ptr(), ld, rows, n, 0.125), [DP], f"softmax_rows_bwd n={n} ld={ld}", ins=[P])
    want, e = EB.softmax_rows_bwd(p, dp, 0.125)
    _note("softmax_rows_bwd", EB.check_bf16(f"softmax_rows_bwd n={n} rows={rows} {'ld=n+64' if strided else 'dense'}", DP.view, want, e))


# ------------------------------------------------------------------------------------------------
# timestep projection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 320])
@pytest.mark.parametrize("ts,scale", [([0.0, 1e-4, 0.1234, 0.5, 1.0], 1000.0), ([0.0, 1.0, 37.0, 500.5, 999.0, 1000.0], 1.0)])
def test_timestep_proj(lib, dim, ts, scale):
    t = torch.tensor(ts, dtype=F32, device=dev())
    B = t.numel()
    T = Arena(1, B, dtype=F32, data=t)
    Y = Arena(B, dim)
    _twice(lambda: lib("st355_timestep_proj", T.ptr(), Y.ptr(), B, dim, scale), [Y], f"timestep_proj dim={dim} scale={scale}", ins=[T])
    Y.all_written("timestep_proj")
    want, e = EB.timestep_proj(t, dim, scale)
    _note("timestep_proj", EB.check_bf16(f"timestep_proj B={B} dim={dim} scale={scale}", Y.view, want, e))


# ------------------------------------------------------------------------------------------------
# TREAD gather / scatter, transpose: copies, bit for bit
# ------------------------------------------------------------------------------------------------
class Tokens:
    """a [B, S, D] view (row stride D + 24, batch stride (S + 5)(D + 24), storage offset PAD + 8 elements) into a sentinel-filled buffer"""

    def __init__(self, B, S, D, data=None):
        ld, bs = D + 24, (S + 5) * (D + 24)
        self.buf = torch.full((PAD + 8 + B * bs + PAD,), SENT, dtype=BF16, device=dev())
        self.view = torch.as_strided(self.buf, (B, S, D), (bs, ld, 1), PAD + 8)
        self.ld, self.bs = ld, bs
        if data is not None:
            self.view.copy_(data)
        self.prior = self.buf.clone()

    def ptr(self):
        return self.view.data_ptr()

    def expected(self, fn):
        """the whole buffer after fn(view of a copy of the prior buffer) — what a correct call leaves: every other byte keeps its prior bits"""
        want = self.prior.clone()
        fn(torch.as_strided(want, self.view.shape, self.view.stride(), PAD + 8))
        return want


@pytest.mark.parametrize("B,S,K,D", [(3, 37, 19, 72), (3, 1500, 1400, 1024)])
def test_gather_scatter_rows_strided(lib, B, S, K, D):
    """B K D / 8 = 537 600 chunks at the second size: a second grid-stride pass"""
    assert (B * K * D // 8 > GRID) == (K == 1400)
    g = _gen(B * S + K)
    idx = torch.stack([torch.randperm(S, device=dev(), generator=g)[:K] for _ in range(B)]).to(torch.int32).contiguous()
    li = idx.long()[:, :, None].expand(B, K, D)
    X = Tokens(B, S, D, data=_randn(g, B, S, D))
    # gather: out[b, j] = x[b, idx[b, j]]
    O = Tokens(B, K, D)
    for _ in range(2):
        O.buf.copy_(O.prior)
        lib("st355_gather_rows", X.ptr(), X.ld, X.bs, idx.data_ptr(), O.ptr(), O.ld, O.bs, B, K, D)
        assert torch.equal(SB.bits(O.buf), SB.bits(O.expected(lambda v: v.copy_(torch.gather(X.view, 1, li))))), "gather_rows: a row, a gap column or a guard differs"
    assert torch.equal(X.buf, X.prior), "gather_rows: the source was written"
    # scatter: dst[b, idx[b, j]] = src[b, j]; rows not in idx, gap columns and guard rows keep their prior bits
    Sr = Tokens(B, K, D, data=_randn(g, B, K, D))
    Dst = Tokens(B, S, D, data=_randn(g, B, S, D))
    want = Dst.expected(lambda v: v.scatter_(1, li, Sr.view))
    for _ in range(2):
        Dst.buf.copy_(Dst.prior)
        lib("st355_scatter_rows", Sr.ptr(), Sr.ld, Sr.bs, idx.data_ptr(), Dst.ptr(), Dst.ld, Dst.bs, B, K, D)
        assert torch.equal(SB.bits(Dst.buf), SB.bits(want)), "scatter_rows: a routed row differs, or a row outside idx / a gap column / a guard row was written"
    assert torch.equal(Sr.buf, Sr.prior), "scatter_rows: the source was written"
    routed = torch.zeros(B, S, dtype=torch.bool, device=dev()).scatter_(1, idx.long(), True)
    assert torch.equal(SB.bits(Dst.view[~routed]), SB.bits(torch.as_strided(Dst.prior, Dst.view.shape, Dst.view.stride(), PAD + 8)[~routed]))
    # the gather is the scatter's adjoint: a round trip through the same idx restores the routed rows
    Back = Tokens(B, K, D)
    lib("st355_gather_rows", Dst.ptr(), Dst.ld, Dst.bs, idx.data_ptr(), Back.ptr(), Back.ld, Back.bs, B, K, D)
    assert torch.equal(SB.bits(Back.view), SB.bits(Sr.view)), "gather(scatter(src)) != src"
    assert torch.equal(SB.bits(Back.buf), SB.bits(Back.expected(lambda v: v.copy_(Sr.view))))


@pytest.mark.parametrize("rows,cols", [(8, 8), (72, 200), (200, 72), (64, 136)])
def test_transpose_ragged_tiles(lib, rows, cols):
    """rows / cols multiples of 8 but not of 64: the ragged 64 x 64 edge tiles; ld_src and ld_dst larger than the logical width"""
    Sx = Arena(rows, cols, ld=cols + 8, data=_randn(_gen(rows * cols), rows, cols))
    Dx = Arena(cols, rows, ld=rows + 16)
    _twice(lambda: lib("st355_transpose_bf16", Sx.ptr(), Sx.ld, Dx.ptr(), Dx.ld, rows, cols), [Dx], f"transpose {rows} x {cols}", ins=[Sx])
    assert torch.equal(SB.bits(Dx.view), SB.bits(Sx.view.t())), f"transpose {rows} x {cols}"


# ------------------------------------------------------------------------------------------------
# fp8 quantisers: bytes and scales against the oracle on the CPU
# ------------------------------------------------------------------------------------------------
def _quant_act(lib, x, ldx=None):
    """st355_fp8_quantize_act through the C ABI on guarded buffers; x [M, K] bf16 (device).  Returns (bytes [M, K] cpu, scale_a cpu [1])"""
    M, K = x.shape
    X = Arena(M, K, ld=ldx, data=x, off=8 if ldx else 0)
    Q = Arena(M, K, dtype=U8)
    S = Arena(1, 1, dtype=F32)
    W = Arena(1, 1, dtype=F32)          # the 4-byte workspace (the kernel's amax word), guarded like an output
    strided = ldx is not None and ldx != K
    _twice(lambda: lib("st355_fp8_quantize_act", X.ptr(), X.ld, Q.ptr(), S.ptr(), M, K, W.ptr()), [Q, S, W], f"fp8_quantize_act M={M} K={K} ldx={X.ld}", ins=[X])
    HIT.add("fp8_act|strided" if strided else "fp8_act|dense")
    nv = M * (K // 8)
    if not strided and nv & 1:
        HIT.add("fp8_act|odd tail")
    # the kernels' own loop rules (fp8.hip): k_absmax takes one vector per thread and step on both paths; k_fp8_quant_act takes one vector on the strided path
    # and a PAIR of vectors (np = nv / 2 items) on the dense path, so its dense loop runs a second pass only when nv / 2 exceeds the grid
    path = "strided" if strided else "dense"
    if nv > GRID:
        HIT.add(f"fp8_act|absmax grid-stride {path}")
    if (nv if strided else nv // 2) > GRID:
        HIT.add(f"fp8_act|quant grid-stride {path}")
    return Q.view.cpu(), S.view.reshape(1).cpu()


def _act_matches_oracle(lib, x, what, ldx=None):
    from oracle import train_math as TM

    q, s = _quant_act(lib, x, ldx)
    oq, os_ = TM.fp8_quantize_act(x.cpu())
    oq = oq.view(U8)
    bad = (q != oq)
    if bool(bad.any()):
        i = bad.nonzero()[0]
        xv = float(x.cpu()[i[0], i[1]])
        raise AssertionError(f"{what}: {int(bad.sum())} bytes differ from the oracle; first at {i.tolist()}: x = {xv!r} (bits {int(SB.bits(x.cpu())[i[0], i[1]]) & 0xFFFF:#06x}) "
                             f"kernel {int(q[i[0], i[1]]):#04x} oracle {int(oq[i[0], i[1]]):#04x}")
    assert float(s) == float(os_) and SB.bits(s).item() == SB.bits(os_.reshape(1)).item(), f"{what}: scale_a {float(s)!r} != oracle {float(os_)!r}"
    return q, s


ACT_A = [2.0 ** -100, 1.0, 7.5, 300.0, 57344.0, 3e38]


@pytest.mark.parametrize("A", ACT_A)
def test_fp8_act_every_normal_bf16_pattern(lib, A):
    """every finite normal bf16 pattern (and +-0) with |x| <= A as one [M, 264] tensor: every e5m2 tie, the e5m2 subnormal grid, saturation, the two-rounding scale"""
    x = EB.pad_to(EB.bf16_patterns(A), 264).to(dev())
    _act_matches_oracle(lib, x, f"fp8_quantize_act, every pattern with |x| <= {A}")


@pytest.mark.parametrize("A", [None, 1.0, 57344.0])
def test_fp8_act_bf16_subnormal_inputs(lib, A):
    """the bf16-subnormal inputs on their own (A None: amax itself subnormal) and beside one normal value A that sets the scale: a flush-to-zero difference
    between the kernel and the oracle would show here and nowhere else"""
    v = EB.bf16_patterns(1.0, subnormal=True)
    if A is not None:
        v = torch.cat([v, torch.tensor([A], dtype=BF16)])
    _act_matches_oracle(lib, EB.pad_to(v, 264).to(dev()), f"fp8_quantize_act, bf16 subnormals beside {A}")


def test_fp8_act_branches(lib):
    g = _gen(77)
    x = _randn(g, 5, 24, scale=2.0)                       # nv = 15: odd, the single-vector tail of the dense path
    q, s = _act_matches_oracle(lib, x, "fp8_quantize_act 5 x 24 dense")
    q2, s2 = _act_matches_oracle(lib, x, "fp8_quantize_act 5 x 24 as a column slice (ldx = 56)", ldx=56)
    assert torch.equal(q, q2) and torch.equal(s, s2), "the strided run differs from the dense run of the same data"
    z = torch.zeros(5, 24, dtype=BF16, device=dev())
    qz, sz = _act_matches_oracle(lib, z, "fp8_quantize_act all-zero")
    assert not bool(qz.any())
    _act_matches_oracle(lib, z, "fp8_quantize_act all-zero strided", ldx=40)


@pytest.mark.parametrize("M,strided", [(2050, False), (2050, True), (4100, False)])
def test_fp8_act_past_the_grid_cap(lib, M, strided):
    """K = 2056, the grid is 2048 x 256 threads.  M = 2050: 526 850 vectors — a second pass of k_absmax (dense and strided) and of the strided quantise loop; the
    dense quantise loop takes two vectors per thread (263 425 pairs: ONE pass).  M = 4100 dense: 1 053 700 vectors, 526 850 pairs — a second pass of the dense
    quantise loop (q + 16 i, xv[2 i]) and a third of k_absmax.  The maximum sits in the last vector"""
    x = _randn(_gen(78 + M), M, 2056, scale=2.0)
    x[-1, -1] = 97.0
    _act_matches_oracle(lib, x, f"fp8_quantize_act {M} x 2056 {'strided' if strided else 'dense'}", ldx=2056 + 24 if strided else None)


def _weight_matches_oracle(lib, w, what, ldw=None):
    from oracle import train_math as TM

    N, K = w.shape
    Wt = Arena(N, K, ld=ldw, data=w, off=8 if ldw else 0)
    Q = Arena(N, K, dtype=U8)
    S = Arena(1, N, dtype=F32)
    _twice(lambda: lib("st355_fp8_quantize_weight", Wt.ptr(), Wt.ld, Q.ptr(), S.ptr(), N, K), [Q, S], what, ins=[Wt])
    oq, os_ = TM.fp8_quantize_weight(w.cpu())
    q, s, oq = Q.view.cpu(), S.view.reshape(-1).cpu(), oq.view(U8)
    bad = q != oq
    if bool(bad.any()):
        i = bad.nonzero()[0]
        raise AssertionError(f"{what}: {int(bad.sum())} bytes differ from the oracle; first at {i.tolist()}: w = {float(w.cpu()[i[0], i[1]])!r} "
                             f"kernel {int(q[i[0], i[1]]):#04x} oracle {int(oq[i[0], i[1]]):#04x}, row scale {float(s[i[0]])!r} / {float(os_[i[0]])!r}")
    assert torch.equal(SB.bits(s), SB.bits(os_)), f"{what}: scales differ: {s.tolist()} / {os_.tolist()}"


def _weight_rows(As, subnormal=False):
    """two rows per A: the non-negative and the negative patterns with |w| <= A (K = 33 024 holds one sign's 32 640), zero-padded"""
    K = 33024
    rows = []
    for A in As:
        v = EB.bf16_patterns(A, subnormal=subnormal)
        if subnormal:
            v = torch.cat([v, torch.tensor([A, -A], dtype=BF16)])
        neg = torch.signbit(v.float())
        rows += [EB.pad_to(v[~neg], K)[0], EB.pad_to(v[neg], K)[0]]
    return torch.stack(rows)


def test_fp8_weight_every_normal_bf16_pattern(lib):
    """N = 10 (not a multiple of 4: the last workgroup has two idle waves), K = 33 024 (not a multiple of 512)"""
    w = _weight_rows([2.0 ** -100, 1.0, 7.5, 448.0, 3e38])
    assert w.shape == (10, 33024) and 33024 % 512 != 0
    _weight_matches_oracle(lib, w.to(dev()), "fp8_quantize_weight, every pattern")


def test_fp8_weight_bf16_subnormal_inputs(lib):
    _weight_matches_oracle(lib, _weight_rows([2.0 ** -120, 1.0], subnormal=True).to(dev()), "fp8_quantize_weight, bf16 subnormals")


def test_fp8_weight_strided_with_a_zero_row(lib):
    w = _randn(_gen(79), 7, 520, scale=0.05)
    w[3] = 0
    _weight_matches_oracle(lib, w, "fp8_quantize_weight N=7 K=520 ldw=544, row 3 all zero", ldw=544)


# ------------------------------------------------------------------------------------------------
def test_every_instantiation_and_path_was_hit():
    missing = ALL_HIT - HIT
    assert not missing, f"never run by this module: {sorted(missing)}"


def test_worst_ratios_report():
    print("\n| family | worst err/tol | worst block statistic |\n|---|---|---|")
    for fam, w in sorted(WORST.items()):
        print(f"| {fam} | {w['err/tol']:.3f} | {w['block']:.3f} |")

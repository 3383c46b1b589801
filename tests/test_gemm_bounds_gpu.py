"""Every GEMM route, element-wise against an fp64 reference (tests/gemm_bounds.py).

Each case first asserts the schedule it runs on (ops.gemm_plan -> st355_gemm_plan: the same decision functions the launchers call), then bounds every stored
output element by element: one RNE rounding of an fp32 sum of exact products, plus the fp32 summation error, plus the epilogue's own fp32 arithmetic; and the RMS
error of every 64 x 64 block in bf16 ulps.  A defect confined to one tile, one ragged edge or one epilogue of one schedule fails here even where the suite's global
rel-L2 < 5e-3 checks cannot see it.  The last test asserts that the cases reached every ST355_ROUTE_*: run the module as a whole."""
import math

import pytest
import torch

from tests import gemm_bounds as GB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HIT = set()
ALL_ROUTES = {"ROWS", "THIN", "SPLITK", "S2", "P3", "PQ", "PZ", "PQ_TAIL", "PQ_QK_ROPE", "PQ_HEADS", "PQ_GEGLU", "PZ_GEGLU_GRAD", "PAIR_PQ", "PAIR_P3", "PAIR_HEADS",
              "PAIR_QK_ROPE"}
TILES = {"S2": (128, 128), "SPLITK": (128, 128), "P3": (256, 128), "ROWS": (64, 128), "THIN": (64, 128)}
REPEAT = {"PZ", "PQ_TAIL", "PZ_GEGLU_GRAD"}        # launched twice: bit-identical


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device=dev(), generator=g) * scale + shift).to(BF16)


def _operands(seed, M, N, K, k2=0, bias=False):
    g = _gen(seed)
    A = _randn(g, M, K)
    B = _randn(g, N, K, scale=1 / math.sqrt(K))
    kw = {}
    if k2:
        kw.update(a2=_randn(g, M, k2), b2=_randn(g, N, k2, scale=0.1))
    if bias:
        kw["bias"] = _randn(g, N, scale=0.5)
    return g, A, B, kw


def _acc(A, B, kw):
    return GB.gemm_ref(A, B, kw.get("a2"), kw.get("b2"), kw.get("bias"))


def _plan(ops, problems, routes):
    got = ops.gemm_plan(problems)
    assert got == routes, f"planned {got}, the case is meant for {routes}"
    HIT.update(routes)


def _run(ops, A, B, kw, route):
    """plan == route, launch (twice where the schedule must be repeatable: bit-identical)"""
    _plan(ops, [dict(a=A, w=B, **kw)], [route])
    ops.gemm(A, B, **kw)
    if route in REPEAT:
        first = {k: v.clone() for k, v in kw.items() if k in ("out", "aux_out")}
        ops.gemm(A, B, **kw)
        for k, v in first.items():
            assert torch.equal(kw[k], v), f"{route}: a second launch changed {k}"


def _bound(name, out, want_e, route, rounds=1):
    want, e = want_e
    GB.assert_bound(GB.check(f"{route} {name}", out, want, e, rounds=rounds, tile=TILES.get(route, (256, 256))))


EPIS = ["none", "gelu", "gelu_aux", "gate", "gate_aux", "gelu_grad", "add"]


def _epilogue_case(ops, g, A, B, kw, acc, epi, route, rpb, label):
    """one epilogue on one schedule: builds its operands, runs, bounds every stored output (aux_out first, then what is computed from it)"""
    M, N = acc.ref.shape
    kw = dict(kw)
    kw["out"] = torch.empty(M, N, device=dev(), dtype=BF16)
    if epi in ("gelu", "gelu_aux"):
        kw["epilogue"] = ops.EPI_GELU
    if epi in ("gate", "gate_aux"):
        nb = (M + rpb - 1) // rpb
        gate = _randn(g, nb, N, scale=0.2, shift=1.0)
        kw.update(epilogue=ops.EPI_GATE_RESIDUAL, aux_in=_randn(g, M, N), gate=gate, rows_per_batch=rpb)
    if epi in ("gelu_aux", "gate_aux"):
        kw["aux_out"] = torch.empty(M, N, device=dev(), dtype=BF16)
    if epi == "gelu_grad":
        kw.update(epilogue=ops.EPI_MUL_GELU_GRAD, aux_in=_randn(g, M, N))
    if epi == "add":
        kw.update(epilogue=ops.EPI_ADD, aux_in=_randn(g, M, N))
    _run(ops, A, B, kw, route)
    name = f"{label} {epi}"
    if "aux_out" in kw:
        _bound(name + " aux_out", kw["aux_out"], GB.epi_none(acc), route)
    C = kw["out"]
    if epi == "none":
        _bound(name, C, GB.epi_none(acc), route)
    elif epi == "gelu":
        _bound(name, C, GB.epi_gelu(acc), route)
    elif epi == "gelu_aux":
        _bound(name, C, GB.epi_gelu_of_stored(kw["aux_out"]), route)
    elif epi in ("gate", "gate_aux"):
        rows = torch.arange(M, device=dev()) // rpb
        _bound(name, C, GB.epi_gate_residual(acc, kw["aux_in"], kw["gate"][rows]), route)
    elif epi == "gelu_grad":
        _bound(name, C, GB.epi_mul_gelu_grad(acc, kw["aux_in"]), route)
    else:
        _bound(name, C, GB.epi_add(acc, kw["aux_in"]), route)


# ------------------------------------------------------------------------------------------------
# every schedule x ragged edges (plain product)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,bias,route", [
    (1, 3072, 256, False, "S2"), (300, 200, 256, True, "S2"), (129, 132, 1024, False, "S2"),
    (2000, 2196, 320, False, "P3"),                  # by tile count (72 tiles of 256 x 256, 144 of 256 x 128)
    (36864, 128, 3072, False, "P3"),                 # narrow: N <= 128 on a long batch
    (4100, 3076, 1024, True, "PQ"), (4096, 4096, 512, False, "PQ"),
    (4608, 9216, 3072, False, "PZ"), (4608, 4608, 1024, True, "PZ"),
    (2000, 96, 3072, False, "SPLITK"), (2000, 96, 3072, True, "SPLITK"),       # with bias: the slab reduce adds it
    (1061, 64, 512, False, "ROWS"), (16421, 128, 1280, False, "ROWS"),
    (5000, 64, 704, False, "THIN"), (36864, 64, 3072, False, "THIN"),
])
def test_schedule_ragged_edges(ops, M, N, K, bias, route):
    g, A, B, kw = _operands(11, M, N, K, bias=bias)
    kw["out"] = torch.empty(M, N, device=dev(), dtype=BF16)
    _run(ops, A, B, kw, route)
    _bound(f"{M}x{N}x{K}{' +bias' if bias else ''}", kw["out"], GB.epi_none(_acc(A, B, kw)), route)


TAIL_SHAPES = [(16384, 1280, 2560, 64, False), (16384, 1280, 5120, 0, True), (16384, 1280, 10240, 64, True), (16000, 1280, 2048, 0, True),
               (34816, 1536, 6144, 0, True), (32768, 256, 2048, 0, False)]


def test_stream_k_tail_probe_confirms_round_robin_placement(ops):
    """the first tail case: warms the XCD placement probe (one launch of a cut shape), which must confirm round-robin placement; only then does the plan report the tail"""
    M, N, K, k2, bias = TAIL_SHAPES[0]
    g, A, B, kw = _operands(12, M, N, K, k2, bias)
    ops.gemm(A, B, **kw)
    torch.cuda.synchronize()
    assert ops.gemm_tail_placement() == 1
    kw["out"] = torch.empty(M, N, device=dev(), dtype=BF16)
    _run(ops, A, B, kw, "PQ_TAIL")
    _bound(f"{M}x{N}x{K}+{k2}", kw["out"], GB.epi_none(_acc(A, B, kw)), "PQ_TAIL")


@pytest.mark.parametrize("M,N,K,k2,bias", TAIL_SHAPES[1:])
def test_stream_k_tail_shapes(ops, M, N, K, k2, bias):
    assert ops.gemm_tail_placement() == 1, "the probe test runs first"
    g, A, B, kw = _operands(13, M, N, K, k2, bias)
    acc = _acc(A, B, kw)
    for epi in ("none", "gate_aux") if M == 34816 else ("none",):
        _epilogue_case(ops, g, A, B, kw, acc, epi, "PQ_TAIL", 4327, f"{M}x{N}x{K}+{k2}")


# ------------------------------------------------------------------------------------------------
# epilogue x schedule, bias and K-extension on / off
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ext", [False, True], ids=["plain", "bias+K2"])
@pytest.mark.parametrize("M,N,K,route,rpb", [
    (300, 200, 256, "S2", 100),
    (2000, 2196, 320, "P3", 1000),
    (4100, 3076, 1024, "PQ", 4327 // 4),
    (8654, 1536, 1536, "PQ", 4327),                  # the SD3 bucket's 4327 rows per sample: batch boundaries inside tiles
    (4608, 4608, 1024, "PZ", 576),
    (16384, 1280, 2560, "PQ_TAIL", 1000),
])
def test_epilogues_on_every_schedule(ops, M, N, K, route, rpb, with_ext):
    if route == "PQ_TAIL":
        assert ops.gemm_tail_placement() == 1, "the probe test runs first"
    g, A, B, kw = _operands(14, M, N, K, 64 if with_ext else 0, with_ext)
    acc = _acc(A, B, kw)
    for epi in EPIS:
        _epilogue_case(ops, g, A, B, kw, acc, epi, route, rpb, f"{M}x{N}x{K}{' bias+K2' if with_ext else ''}")


@pytest.mark.parametrize("M,K,F,route", [(4100, 640, 1024, "PQ_GEGLU"), (4608, 1024, 4608, "PQ_GEGLU")])
@pytest.mark.parametrize("bias", [False, True])
def test_geglu_forward(ops, M, K, F, route, bias):
    """EPI_GEGLU: aux_out = the interleaved pre-activation (one rounding), C = value * gelu(gate) of the STORED halves (chained on aux_out)"""
    g, A, B, kw = _operands(15, M, 2 * F, K, bias=bias)
    kw.update(epilogue=ops.EPI_GEGLU, aux_out=torch.empty(M, 2 * F, device=dev(), dtype=BF16), out=torch.empty(M, F, device=dev(), dtype=BF16))
    _run(ops, A, B, kw, route)
    _bound(f"geglu {M}x{2 * F}x{K} aux_out", kw["aux_out"], GB.epi_none(_acc(A, B, kw)), route)
    _bound(f"geglu {M}x{2 * F}x{K}", kw["out"], GB.epi_geglu_of_stored(kw["aux_out"]), route)


@pytest.mark.parametrize("M,K,F,route", [(4100, 640, 1024, "PQ_GEGLU"), (4608, 1024, 4608, "PZ_GEGLU_GRAD")])
def test_geglu_backward(ops, M, K, F, route):
    """EPI_GEGLU_GRAD: d out = acc rounded to bf16, then d value | d gate (rounded again): one extra ulp"""
    g, A, B, kw = _operands(16, M, F, K)
    pre = _randn(g, M, 2 * F)
    kw.update(epilogue=ops.EPI_GEGLU_GRAD, aux_in=pre, out=torch.empty(M, 2 * F, device=dev(), dtype=BF16))
    _run(ops, A, B, kw, route)
    want, e = GB.epi_geglu_grad(_acc(A, B, kw), pre)
    GB.assert_bound(GB.check(f"{route} geglu grad {M}x{F}x{K}", kw["out"], want, e, rounds=2))


# ------------------------------------------------------------------------------------------------
# strides and layouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,route", [(300, 200, 256, "S2"), (2000, 2196, 320, "P3"), (4100, 3076, 1024, "PQ"), (4608, 4608, 1024, "PZ")])
def test_column_blocks_of_wider_buffers(ops, M, N, K, route):
    """A a column slice (lda > K); C, aux_in, aux_out column blocks of wider buffers (gated residual with the branch store): columns outside the block stay untouched"""
    g = _gen(17)
    Abuf = _randn(g, M, K + 128)
    A = Abuf[:, 64:64 + K]
    B = _randn(g, N, K, scale=1 / math.sqrt(K))
    bias = _randn(g, N, scale=0.5)
    Cbuf = torch.full((M, N + 64), 7.0, device=dev(), dtype=BF16)
    Obuf = torch.full((M, N + 128), 7.0, device=dev(), dtype=BF16)
    Rbuf = _randn(g, M, N + 32)
    rpb = 1000
    gate = _randn(g, (M + rpb - 1) // rpb, N, scale=0.2, shift=1.0)
    kw = dict(bias=bias, out=Cbuf[:, 32:32 + N], aux_out=Obuf[:, 64:64 + N], aux_in=Rbuf[:, 16:16 + N], gate=gate, rows_per_batch=rpb,
              epilogue=ops.EPI_GATE_RESIDUAL)
    _run(ops, A, B, kw, route)
    acc = GB.gemm_ref(A, B, bias=bias)
    _bound("strided aux_out", kw["aux_out"], GB.epi_none(acc), route)
    _bound("strided gate residual", kw["out"], GB.epi_gate_residual(acc, kw["aux_in"], gate[torch.arange(M, device=dev()) // rpb]), route)
    for buf, lo, hi in ((Cbuf, 32, 32 + N), (Obuf, 64, 64 + N)):
        rest = torch.cat([buf[:, :lo].reshape(-1), buf[:, hi:].reshape(-1)]).float()
        assert bool((rest == 7.0).all()), "a column outside the output block was written"


@pytest.mark.parametrize("nseg,seg,lead,N,K,route", [(4, 1024, 256, 3072, 1024, "PQ"), (4, 512, 77, 2176, 512, "P3")])
def test_segmented_rows(ops, nseg, seg, lead, N, K, route):
    """seg_rows: the image rows of every sample of a joint [B, lead + seg, *] buffer as one problem (A, C and aux_in segmented), EPI_ADD"""
    g = _gen(18)
    Ajoint = _randn(g, nseg, lead + seg, K)
    B = _randn(g, N, K, scale=1 / math.sqrt(K))
    Cjoint = torch.full((nseg, lead + seg, N), 7.0, device=dev(), dtype=BF16)
    Rjoint = _randn(g, nseg, lead + seg, N)
    kw = dict(out=Cjoint[:, lead:], aux_in=Rjoint[:, lead:], epilogue=ops.EPI_ADD)
    A = Ajoint[:, lead:]
    _run(ops, A, B, kw, route)
    acc = GB.gemm_ref(A.reshape(-1, K), B)
    _bound("segmented rows add", Cjoint[:, lead:].reshape(-1, N), GB.epi_add(acc, Rjoint[:, lead:].reshape(-1, N)), route)
    assert bool((Cjoint[:, :lead].float() == 7.0).all()), "rows outside the segments were written"


# ------------------------------------------------------------------------------------------------
# grouped problems
# ------------------------------------------------------------------------------------------------
GROUPS = {
    # (M, N, K, K2, bias) per problem
    "pair_pq": ([(4100, 3076, 1024, 64, True), (1000, 1540, 512, 0, False)], ["PAIR_PQ", "PAIR_PQ"]),
    "pair_p3": ([(2000, 1000, 512, 0, True), (1500, 1300, 256, 64, False)], ["PAIR_P3", "PAIR_P3"]),      # 68 tiles of 256 x 256, 130 of 256 x 128
    "separate_pz": ([(4608, 4608, 1024, 0, False), (5120, 4096, 1536, 64, True)], ["PZ", "PZ"]),
    "odd_last": ([(4100, 3076, 1024, 0, True), (1000, 1540, 512, 64, False), (300, 200, 256, 0, True)], ["PAIR_PQ", "PAIR_PQ", "S2"]),
}


@pytest.mark.parametrize("epi", ["none", "gelu_aux"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_grouped_problems(ops, group, epi):
    shapes, routes = GROUPS[group]
    probs, accs = [], []
    for i, (M, N, K, k2, bias) in enumerate(shapes):
        g, A, B, kw = _operands(20 + i, M, N, K, k2, bias)
        kw["out"] = torch.empty(M, N, device=dev(), dtype=BF16)
        if epi == "gelu_aux":
            kw.update(epilogue=ops.EPI_GELU, aux_out=torch.empty(M, N, device=dev(), dtype=BF16))
        probs.append(dict(a=A, w=B, **kw))
        accs.append(_acc(A, B, kw))
    _plan(ops, probs, routes)
    ops.gemm_grouped(probs)
    for p, acc, route in zip(probs, accs, routes):
        name = f"{group} {acc.ref.shape[0]}x{acc.ref.shape[1]}"
        if epi == "none":
            _bound(name, p["out"], GB.epi_none(acc), route)
        else:
            _bound(name + " aux_out", p["aux_out"], GB.epi_none(acc), route)
            _bound(name + " gelu", p["out"], GB.epi_gelu_of_stored(p["aux_out"]), route)


# ------------------------------------------------------------------------------------------------
# head-major epilogues (EPI_HEADS, EPI_QK_NORM_ROPE): the projection bound, read back through the head split
# ------------------------------------------------------------------------------------------------
def _heads_stream(ops, g, B_, R, K, H, bias):
    M, N = B_ * R, 3 * H * 64
    A = _randn(g, M, K)
    W = _randn(g, N, K, scale=1 / math.sqrt(K))
    kw = dict(bias=_randn(g, N, scale=0.5)) if bias else {}
    return A, W, kw


@pytest.mark.parametrize("pair", [False, True])
def test_heads_epilogue(ops, pair):
    """q / k head-major at pos0 + m % R of sample m / R, v row-major: each element within the projection bound; text and image rows of different counts"""
    g = _gen(30)
    B_, H, K, S = 2, 4, 512, 600
    streams = [(100, 0, False), (300, 100, True)] if pair else [(300, 50, True)]
    Q = torch.full((B_, H, S, 64), 7.0, device=dev(), dtype=BF16)
    Kh = torch.full_like(Q, 7.0)
    probs, refs = [], []
    for R, pos0, bias in streams:
        A, W, kw = _heads_stream(ops, g, B_, R, K, H, bias)
        out = torch.empty(B_ * R, H * 64, device=dev(), dtype=BF16)
        probs.append(dict(a=A, w=W, out=out, epilogue=ops.EPI_HEADS, heads=ops.heads(Q, Kh, None, H, S, pos0, H * 64, H * 64), rows_per_batch=R, **kw))
        refs.append((R, pos0, out, _acc(A, W, kw)))
    routes = ["PAIR_HEADS", "PAIR_HEADS"] if pair else ["PQ_HEADS"]
    _plan(ops, probs, routes)
    if pair:
        ops.gemm_grouped(probs)
    else:
        ops.gemm(**probs[0])
    D = H * 64
    for (R, pos0, out, acc), route in zip(refs, routes):
        for c0, dst in ((0, Q), (D, Kh)):
            got = dst[:, :, pos0:pos0 + R].permute(0, 2, 1, 3).reshape(B_ * R, D)
            _bound(f"heads R={R} part {c0 // D}", got, (acc.ref[:, c0:c0 + D], acc.s[:, c0:c0 + D]), route)
        _bound(f"heads R={R} v", out, (acc.ref[:, 2 * D:], acc.s[:, 2 * D:]), route)
    covered = torch.zeros(S, dtype=torch.bool)
    for R, pos0, _, _ in refs:
        covered[pos0:pos0 + R] = True
    assert bool((Q[:, :, ~covered.to(dev())].float() == 7.0).all()), "positions outside the streams were written"


def _norm_rope_ref(acc, w, cos_p, sin_p, pos, H, eps=1e-6):
    """fp64 RMSNorm(x) * w, then the interleaved-pair rotation, for one q or k part [M, H*128] of the projection; with its error budget: a perturbation s of x moves
    x / rms(x) by at most (s + |x| max(s) / rms) / rms, the rotation adds |cos| + |sin| of its pair, the fp32 norm itself ~2^-22 relative"""
    M = acc.ref.shape[0]
    x = acc.ref.view(M, H, 128)
    s = acc.s.view(M, H, 128)
    rms = torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    wv = w.double() if w is not None else torch.ones(128, device=x.device, dtype=torch.float64)
    xn = x / rms * wv
    c = cos_p.double()[pos].repeat_interleave(2, dim=1)[:, None, :]
    sn = sin_p.double()[pos].repeat_interleave(2, dim=1)[:, None, :]
    xr, xi = xn.view(M, H, 64, 2).unbind(-1)
    rot = torch.stack([-xi, xr], dim=-1).view(M, H, 128)
    f = xn * c + rot * sn
    en = wv.abs() * (s + x.abs() * s.amax(-1, keepdim=True) / rms) / rms
    en_pair = en.view(M, H, 64, 2).flip(-1).reshape(M, H, 128)
    e = en * c.abs() + en_pair * sn.abs() + GB.U20 * (1 + f.abs() + 2 * xn.abs())
    return f.view(M, H * 128), e.view(M, H * 128)


@pytest.mark.parametrize("pair", [False, True])
def test_qk_norm_rope_epilogue(ops, pair):
    g = _gen(31)
    B_, H, hd, St, Si, Kin = 2, 2, 128, 256, 512, 192
    S, D = St + Si, H * hd
    ang = torch.rand(S, 64, device=dev(), dtype=torch.float64, generator=g) * 6.0
    cos_p, sin_p = ang.cos().float().contiguous(), ang.sin().float().contiguous()
    Q = torch.zeros(B_, H, S, hd, device=dev(), dtype=BF16)
    Kh = torch.zeros_like(Q)
    rrms = torch.zeros(B_ * S, 2 * H, device=dev())
    V = torch.zeros(B_ * S, D, device=dev(), dtype=BF16)
    streams = [("txt", St, 0), ("img", Si, St)] if pair else [("img", Si, St)]
    probs, refs = [], []
    for i, (name, rows, pos0) in enumerate(streams):
        x = _randn(g, B_ * rows, Kin)
        W = _randn(g, 3 * D, Kin, scale=0.08)
        bias = _randn(g, 3 * D, scale=0.1)
        wq, wk = _randn(g, hd, scale=0.2, shift=1.0), _randn(g, hd, scale=0.2, shift=1.0)
        kw = dict(a2=_randn(g, B_ * rows, 64), b2=_randn(g, 3 * D, 64, scale=0.05)) if i == 0 else {}
        probs.append(dict(a=x, w=W, bias=bias, out=V.view(B_, S, D)[:, pos0:pos0 + rows], epilogue=ops.EPI_QK_NORM_ROPE,
                          rope=ops.qk_rope(Q, Kh, rrms, wq, wk, cos_p, sin_p, H, S, pos0), rows_per_batch=rows, **kw))
        refs.append((rows, pos0, wq, wk, GB.gemm_ref(x, W, kw.get("a2"), kw.get("b2"), bias)))
    routes = ["PAIR_QK_ROPE", "PAIR_QK_ROPE"] if pair else ["PQ_QK_ROPE"]
    _plan(ops, probs, routes)
    ops.gemm_grouped(probs)
    for (rows, pos0, wq, wk, acc), route in zip(refs, routes):
        pos = pos0 + torch.arange(B_ * rows, device=dev()) % rows
        for part, w, dst in ((0, wq, Q), (1, wk, Kh)):
            sub = GB.Acc(acc.ref[:, part * D:(part + 1) * D], acc.s[:, part * D:(part + 1) * D])
            got = dst[:, :, pos0:pos0 + rows].permute(0, 2, 1, 3).reshape(B_ * rows, D)
            _bound(f"qk rope rows={rows} part {part}", got, _norm_rope_ref(sub, w, cos_p, sin_p, pos, H), route)
        _bound(f"qk rope rows={rows} v", V.view(B_, S, D)[:, pos0:pos0 + rows].reshape(-1, D), (acc.ref[:, 2 * D:], acc.s[:, 2 * D:]), route)


# ------------------------------------------------------------------------------------------------
# weight gradient (st355_gemm_tn_bf16 / _seg), fp8 Linear
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mc,P,Q,accumulate", [(4096, 1000, 520, False), (4096, 1000, 520, True), (16384, 3072, 3072, True), (512, 264, 3080, False)])
def test_weight_gradient(ops, Mc, P, Q, accumulate):
    g = _gen(40)
    L = _randn(g, Mc, P)
    R = _randn(g, Mc, Q, scale=1 / math.sqrt(Mc))
    C0 = _randn(g, P, Q)
    out = C0.clone() if accumulate else torch.empty(P, Q, device=dev(), dtype=BF16)
    ops.gemm_tn(L, R, out=out, accumulate=accumulate)
    acc = GB.gemm_ref(L.t(), R.t())
    want_e = GB.epi_add(acc, C0) if accumulate else GB.epi_none(acc)
    GB.assert_bound(GB.check(f"tn {Mc}:{P}x{Q}{' accumulate' if accumulate else ''}", out, *want_e))


@pytest.mark.parametrize("accumulate", [False, True])
def test_weight_gradient_segmented_contraction(ops, accumulate):
    g = _gen(41)
    B_, lead, rows, P, Q = 3, 64, 512, 1000, 520
    Lj = _randn(g, B_, lead + rows, P)
    Rj = _randn(g, B_, lead + rows, Q, scale=1 / math.sqrt(B_ * rows))
    C0 = _randn(g, P, Q)
    out = C0.clone() if accumulate else torch.empty(P, Q, device=dev(), dtype=BF16)
    ops.gemm_tn(Lj[:, lead:], Rj[:, lead:], out=out, accumulate=accumulate)
    acc = GB.gemm_ref(Lj[:, lead:].reshape(-1, P).t(), Rj[:, lead:].reshape(-1, Q).t())
    GB.assert_bound(GB.check("tn segmented", out, *(GB.epi_add(acc, C0) if accumulate else GB.epi_none(acc))))


@pytest.mark.parametrize("M,N,K", [(4608, 3072, 3072), (1000, 520, 256), (18432, 12288, 3072), (1000, 264, 1024)])
def test_fp8_linear_all_rows(ops, M, N, K):
    """st355_linear_fp8 over EVERY row: fp64 over the dequantised e5m2 x e4m3 operands, the product and its magnitude scaled by sa * sw[n], + bias"""
    g = _gen(42)
    x = _randn(g, M, K)
    w = _randn(g, N, K, scale=0.03)
    bias = _randn(g, N)
    q, sc = ops.fp8_quantize_weight(w)
    xq, sa = ops.fp8_quantize_act(x)
    out = ops.linear_fp8(xq, sa, q, sc, bias=bias)
    a = xq.view(torch.float8_e5m2).float()
    b = q.view(torch.float8_e4m3fn).float()
    del x, w
    acc = GB.gemm_ref(a, b, scale=sa.double()[0] * sc.double()[None, :])
    f = acc.ref + bias.double()
    e = acc.s + GB.U20 * (1 + f.abs() + acc.ref.abs())
    GB.assert_bound(GB.check(f"fp8 {M}x{N}x{K}", out, f, e))


# ------------------------------------------------------------------------------------------------
# addressing beyond 32 bits
# ------------------------------------------------------------------------------------------------
def test_operands_beyond_4_gib(ops):
    """A spans 4.6 GB, C 2.3 GB: correct (checked on the row tiles around the 2 GiB and 4 GiB byte offsets of A and C, and the last tile) or refused by validate()"""
    M, K, N = 139264, 16384, 8192
    g = _gen(43)
    A = torch.empty(M, K, device=dev(), dtype=BF16)
    for r in range(0, M, 16384):
        A[r:r + 16384] = _randn(g, min(16384, M - r), K)
    B = _randn(g, N, K, scale=1 / math.sqrt(K))
    C = torch.empty(M, N, device=dev(), dtype=BF16)
    from simpletuner_amd.lib import St355Error

    try:
        _plan(ops, [dict(a=A, w=B, out=C)], ["PQ"])
        ops.gemm(A, B, out=C)
    except St355Error as err:
        print(f"[bound] >4 GiB operands refused by validate(): {err}")
        return
    a_row, c_row = K * 2, N * 2
    rows = sorted({r for b in (2 ** 31 // a_row, 2 ** 32 // a_row, 2 ** 31 // c_row) for r in range(b // 256 * 256 - 256, b // 256 * 256 + 256)} |
                  set(range(M - 256, M)))
    idx = torch.tensor(rows, device=dev())
    acc = GB.gemm_ref(A[idx], B)
    GB.assert_bound(GB.check(f"beyond 4 GiB {M}x{N}x{K} ({len(rows)} sampled rows)", C[idx], *GB.epi_none(acc), rows=idx.cpu()))


def test_every_route_is_hit():
    """the cases above (the whole module) reached every ST355_ROUTE_*"""
    assert HIT == ALL_ROUTES, f"routes never reached: {sorted(ALL_ROUTES - HIT)}"

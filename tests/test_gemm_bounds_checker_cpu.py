"""The GEMM bound checker (tests/gemm_bounds.py) bites: on small synthetic problems computed in torch on the CPU (no GPU, no library), a correctly rounded result
passes it, and each modelled kernel defect fails it while the suite's global rel-L2 < 5e-3 check still passes."""
import torch

from tests import gemm_bounds as GB

BF16 = torch.bfloat16


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(BF16)
    B = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    return A, B


def _kernel_like(A, B, k_stop=None):
    """fp32 accumulation of the exact bf16 products, rounded once (RNE) — what a correct kernel stores; k_stop: sum only the first k_stop columns of K"""
    a, b = A.float(), B.float()
    if k_stop is not None:
        a, b = a[:, :k_stop], b[:, :k_stop]
    return a @ b.t()


def _verdict(name, out, want, e, rounds=1, tile=(256, 256)):
    rep = GB.check(name, out, want, e, rounds=rounds, tile=tile)
    rel = GB.rel_l2(out, want)
    print(f"[mutation] {name}: new checker {'PASS' if rep.ok else 'FAIL'} (worst err/tol {rep.worst:.2f}, block RMS {rep.block_rms:.2f}), old rel-L2 {rel:.2e}")
    return rep, rel


def test_correctly_rounded_results_pass():
    for (M, N, K) in ((300, 200, 256), (1000, 520, 1024), (257, 132, 4096)):
        A, B = _operands(M, N, K, 1)
        bias = torch.randn(N).to(BF16)
        acc = GB.gemm_ref(A, B, bias=bias)
        out = GB.to_bf16_rne(_kernel_like(A, B) + bias.float())
        rep, rel = _verdict(f"correct {M}x{N}x{K}", out, *GB.epi_none(acc))
        GB.assert_bound(rep)
        assert rel < 5e-3


def test_correctly_rounded_epilogues_pass():
    M, N, K = 256, 192, 512
    A, B = _operands(M, N, K, 2)
    acc32 = _kernel_like(A, B)
    acc = GB.gemm_ref(A, B)
    g = torch.Generator().manual_seed(3)
    res = torch.randn(M, N, generator=g).to(BF16)
    gate = torch.randn(3, N, generator=g).to(BF16)
    gate_rows = gate.float().repeat_interleave(100, 0)[:M]
    h = torch.randn(M, N, generator=g).to(BF16)
    GB.assert_bound(GB.check("add", GB.to_bf16_rne(acc32 + res.float()), *GB.epi_add(acc, res)))
    GB.assert_bound(GB.check("gelu", GB.to_bf16_rne(torch.nn.functional.gelu(acc32, approximate="tanh")), *GB.epi_gelu(acc)))
    pre = GB.to_bf16_rne(acc32)
    GB.assert_bound(GB.check("gelu of aux_out", GB.to_bf16_rne(torch.nn.functional.gelu(pre.float(), approximate="tanh")), *GB.epi_gelu_of_stored(pre)))
    GB.assert_bound(GB.check("gate residual", GB.to_bf16_rne(res.float() + gate_rows * acc32), *GB.epi_gate_residual(acc, res, gate_rows)))
    GB.assert_bound(GB.check("x gelu'", GB.to_bf16_rne(acc32 * GB.gelu_tanh_grad(h.double()).float()), *GB.epi_mul_gelu_grad(acc, h)))
    # GEGLU forward from the stored interleaved pre-activation; backward with d out rounded first (twice-rounded outputs)
    v, gt = GB.geglu_split(pre.float())
    GB.assert_bound(GB.check("geglu", GB.to_bf16_rne(v * torch.nn.functional.gelu(gt)), *GB.epi_geglu_of_stored(pre)))
    pre2 = torch.randn(M, 2 * N, generator=g).to(BF16)
    d = GB.to_bf16_rne(acc32).float()
    v2, g2 = GB.geglu_split(pre2.float())
    out = GB.to_bf16_rne(GB.geglu_join(d * torch.nn.functional.gelu(g2), d * v2 * GB.gelu_erf_grad(g2.double()).float()))
    want, e = GB.epi_geglu_grad(acc, pre2)
    GB.assert_bound(GB.check("geglu grad", out, want, e, rounds=2))
    assert not GB.check("geglu grad, one ulp too strict", out, want, e, rounds=1, verbose=False).ok_elem      # the extra ulp is needed


def test_one_block_scaled_by_1_plus_2_to_minus_6_fails():
    """a long contraction (K = 16384), where the worst-case per-element bound is loose: only the block RMS catches it"""
    M, N, K = 512, 512, 16384
    A, B = _operands(M, N, K, 4)
    acc32 = _kernel_like(A, B)
    y = acc32.clone()
    y[256:320, 128:192] *= 1 + 2 ** -6
    rep, rel = _verdict("one 64x64 block x (1 + 2^-6)", GB.to_bf16_rne(y), *GB.epi_none(GB.gemm_ref(A, B)))
    assert not rep.ok and not rep.ok_block and rep.block_at == (4, 2)
    assert rel < 5e-3


def test_last_k_tile_dropped_in_the_ragged_edge_tiles_fails():
    M, N, K = 8193, 512, 1024                   # one ragged 256-row tile of one row
    A, B = _operands(M, N, K, 5)
    y = _kernel_like(A, B)
    y[8192:] = _kernel_like(A[8192:], B, k_stop=K - 64)
    rep, rel = _verdict("last K-tile dropped in the edge tiles", GB.to_bf16_rne(y), *GB.epi_none(GB.gemm_ref(A, B)))
    assert not rep.ok_elem and rep.worst_at[0] == 8192 and rep.block_edge
    assert rel < 5e-3


def test_last_ragged_row_tile_shifted_by_one_row_fails():
    M, N, K = 256 * 800 + 2, 64, 128
    A, B = _operands(M, N, K, 6)
    y = _kernel_like(A, B)
    t0 = M // 256 * 256
    y[t0:] = y[t0 - 1:M - 1].clone()             # the last tile's rows one row early
    rep, rel = _verdict("last ragged row tile shifted by one row", GB.to_bf16_rne(y), *GB.epi_none(GB.gemm_ref(A, B)))
    assert not rep.ok_elem and rep.worst_at[0] >= t0
    assert rel < 5e-3


def test_gate_rows_from_the_wrong_batch_inside_a_tile_fails():
    """EPI_GATE_RESIDUAL with rows_per_batch = 4327 (not a multiple of 256): the rows of a tile past a batch boundary take the gate of the tile's first row"""
    rpb, nb, N, K = 4327, 8, 256, 256
    M = rpb * nb
    A, B = _operands(M, N, K, 7)
    g = torch.Generator().manual_seed(8)
    res = torch.randn(M, N, generator=g).to(BF16)
    base = 1 + 0.2 * torch.randn(1, N, generator=g)
    gate = (base + 0.02 * torch.randn(nb, N, generator=g)).to(BF16)        # per-sample modulation gates of nearby timesteps: close, not equal
    rows = torch.arange(M)
    good = gate.float()[rows // rpb]
    bad = gate.float()[(rows // 256 * 256) // rpb]
    assert (good != bad).any()
    acc32 = _kernel_like(A, B)
    want, e = GB.epi_gate_residual(GB.gemm_ref(A, B), res, good)
    GB.assert_bound(GB.check("gate residual, rows_per_batch 4327", GB.to_bf16_rne(res.float() + good * acc32), want, e))
    rep, rel = _verdict("gate rows from the wrong batch", GB.to_bf16_rne(res.float() + bad * acc32), want, e)
    assert not rep.ok_elem
    assert rel < 5e-3


def test_round_toward_zero_instead_of_rne_fails():
    M, N, K = 1024, 1024, 512
    A, B = _operands(M, N, K, 9)
    acc32 = _kernel_like(A, B)
    rtz = (acc32.view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)        # truncate the low 16 bits: exact in bf16
    rep, rel = _verdict("round toward zero", rtz, *GB.epi_none(GB.gemm_ref(A, B)))
    assert not rep.ok
    assert rel < 5e-3

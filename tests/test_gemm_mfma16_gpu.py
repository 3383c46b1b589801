"""The one family of instantiations of the 16x16x32 K loop (k_gemm_pq / k_gemm_pz, NT bf16) that tests/test_gemm_bounds_gpu.py and tests/test_conv_bounds_gpu.py
do not reach: the stream-K tail cut into THREE slices (k_gemm_pq<EPI, SK = 3>).  Those suites run k_gemm_pq<none .. add>, <QK norm + RoPE> (v heads included),
<GEGLU>, <GEGLU grad>, <heads>, k_gemm_pz<none .. add, GEGLU grad> (the conv-mode instances keep the 32x32x16 loop) and the tail at two and
four slices; the tail's slice count is cus / (tiles % cus) capped at 4 (2 below K = 4096), and none of their shapes leaves 65-85 tiles in the last round of 256 CUs.
Same bound as there (tests/gemm_bounds.py): every element against the fp64 reference.

Limits: the slice count is not observable through ops.gemm_plan (it reports the route only), so the test relies on tail_plan's arithmetic for this shape
(336 tiles on 256 CUs leave 80: 256 / 80 = 3, K = 4096 keeps the count above 2); if those defaults change it covers two or four slices again.  Only the plain and
the add epilogue run at three slices: the slab exchange sits before the epilogue and does not depend on it, and every epilogue is bounded at two slices in
tests/test_gemm_bounds_gpu.py.  A coverage addition: it holds for the 32x32x16 loop as well."""
import math

import pytest
import torch

from tests import gemm_bounds as GB

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.mark.parametrize("epi", ["none", "add"])
def test_stream_k_tail_in_three_slices(epi):
    from simpletuner_amd import ops

    d = torch.device("cuda:0")
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the shape below leaves 80 of 336 tiles in the last round of 256 CUs: 256 / 80 = 3 slices"
    M, N, K = 12288, 1792, 4096                                  # 48 x 7 tiles of 256 x 256
    g = torch.Generator(device="cuda").manual_seed(31)
    A = torch.randn(M, K, device=d, generator=g).to(BF16)
    B = (torch.randn(N, K, device=d, generator=g) / math.sqrt(K)).to(BF16)
    bias = (torch.randn(N, device=d, generator=g) * 0.5).to(BF16)
    kw = dict(bias=bias)
    if epi == "add":
        kw.update(epilogue=ops.EPI_ADD, aux_in=torch.randn(M, N, device=d, generator=g).to(BF16))
    ops.gemm(A, B, **kw)                                         # (the first cut launch of a process runs the XCD placement probe)
    torch.cuda.synchronize()
    assert ops.gemm_tail_placement() == 1
    kw["out"] = torch.empty(M, N, device=d, dtype=BF16)
    assert ops.gemm_plan([dict(a=A, w=B, **kw)]) == ["PQ_TAIL"]
    ops.gemm(A, B, **kw)
    first = kw["out"].clone()
    ops.gemm(A, B, **kw)
    assert torch.equal(kw["out"], first), "a second launch changed the output (the slices are summed in a fixed order)"
    acc = GB.gemm_ref(A, B, None, None, bias)
    want, e = GB.epi_add(acc, kw["aux_in"]) if epi == "add" else GB.epi_none(acc)
    GB.assert_bound(GB.check(f"PQ_TAIL three slices {M}x{N}x{K} {epi}", kw["out"], want, e, rounds=1, tile=(256, 256)))

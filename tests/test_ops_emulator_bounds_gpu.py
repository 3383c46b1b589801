"""simpletuner_amd.ops on the MI355X under the same table (tests/emulator_cases.py), the same references and the same bounds that hold tests/ops_emulator.py on
the CPU (tests/test_ops_emulator_bounds_cpu.py).  Per case: the family's full checker (the block rounding statistic included where the family has one), the
guard check over every backing buffer, two launches that must agree bit for bit, bit equality with the emulator's output for the exact kinds, and the distance
between the two sides in units of their tolerances, |dev - emu| / (tol_dev + tol_emu), whose worst value per family the last test prints.  An output whose
reference is chained on this side's own stored intermediate (GELU of the stored pre-activation, step 2 of an optimizer, a transposed copy of the stored Q) is
held to its own bound on each side; the two sides are compared only where they answer to the same fp64 value.

Refusals: where the emulator raises EmuError for a precondition of gemm, gemm_tn, colsum_prod, transpose or skinny_tn, the device wrapper must raise before any
launch.  Each refusal case cites the ST_REQUIRE line that refuses the same condition in the C entry."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests import emulator_cases as EC
from tests import ew_bounds as EB
from tests import gemm_bounds as GB
from tests import norm_bounds as NB
from tests import ops_emulator as EMU

pytestmark = pytest.mark.gpu
F64 = torch.float64
BF16 = torch.bfloat16
WORST = {}          # family -> [worst dev err / tol, worst block statistic / limit, worst |dev - emu| / (tol_dev + tol_emu)]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


def _two_d(t):
    return t.reshape(-1, t.shape[-1]) if t.dim() != 2 else t


def _full_check(name, out, want, e, kind, extra):
    """the family's checker for one stored output of the device: (worst element ratio, block statistic / its limit)"""
    if kind in ("bf16", "bf16x2"):
        rep = GB.check(name, _two_d(out), _two_d(want.to(F64).reshape(out.shape)), _two_d(e.to(F64).reshape(out.shape)), rounds=2 if kind == "bf16x2" else 1)
        GB.assert_bound(rep)
        return rep.worst, rep.block_rms / rep.rms_limit
    if kind == "geglu":
        rep = EB.check_geglu(name, out, want, e, extra["gate"])
        GB.assert_bound(rep)
        return rep.worst, rep.block_rms / rep.rms_limit
    if kind == "f32s":
        rep = NB.check_f32(name, out, want, e)
        assert rep.ok, rep.line()
        return rep.worst, rep.block_rms / NB.SUM_RMS_LIMIT
    if kind == "attn":
        f = extra["to_bhsd"]
        rep = AB.check(name, f(out), f(want.reshape(out.shape)), f(e.reshape(out.shape)), f(extra["var"].reshape(out.shape)),
                       final=None if "final" not in extra else f(extra["final"].reshape(out.shape)))
        AB.assert_bound(rep)
        return rep.worst, rep.block_stat / rep.block_limit
    r = EC.elem_ratio(out, want, e, kind, extra)
    print(f"[bound] {name}: worst err/tol={r:.3f} ({kind})")
    assert r <= 1.0, f"{name}: worst |err| / tol = {r:.3f}"
    return r, 0.0


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_device_inside_the_kernel_bound(ops, case):
    first, built = EC.run(case, ops, dev())
    second, _ = EC.run(case, ops, dev())
    host, hbuilt = EC.run(case, EMU)
    assert first.guard_ok, f"{case.name}: {first.guard_msg}"
    assert first.same_ok, f"{case.name}: the wrapper did not return the view it was given"
    for label in first.out:
        assert torch.equal(EC.bits(first.out[label]), EC.bits(second.out[label])), f"{case.name} {label}: two launches differ"
    w = WORST.setdefault(case.family, [0.0, 0.0, 0.0])
    href = {r[0]: r for r in hbuilt.ref(host.out)}
    for label, want, e, kind, *extra in built.ref(first.out):
        ex = extra[0] if extra else None
        derived = bool(ex) and "out" in ex          # a quantity derived from stored outputs (O + O_res): judged by the bound alone
        elem, block = _full_check(f"{case.name} {label}", ex["out"] if derived else first.out[label], want, e, kind, ex)
        w[0], w[1] = max(w[0], elem), max(w[1], block)
        if kind == "zero" or derived:
            continue
        _, hwant, he, hkind, *hextra = href[label]
        if not torch.equal(want, hwant):
            continue          # a chained reference (fp64 of this side's own stored intermediate): the two sides answer to different values, each to its own bound
        if kind == "exact":
            assert torch.equal(EC.bits(first.out[label]), EC.bits(host.out[label])), f"{case.name} {label}: the device and the emulator differ in bits"
            continue
        tol = EC.elem_tol(first.out[label], want, e, kind, ex) + EC.elem_tol(host.out[label], hwant, he, hkind, hextra[0] if hextra else None)
        d = (first.out[label].to(F64) - host.out[label].to(F64)).abs() / tol
        if kind == "edge":
            d = d[ex["x"].float().abs() <= 80]
        w[2] = max(w[2], float(d.max()))
        assert float(d.max()) <= 1.0, f"{case.name} {label}: |dev - emu| / (tol_dev + tol_emu) = {float(d.max()):.3f}"


# ---- refusals: (name, the device call, the ST_REQUIRE that refuses it) ------------------------------------------------------------------------------------
def _bf(*shape):
    return torch.ones(*shape, dtype=BF16, device=dev())


REFUSALS = [
    # gemm.hip st355_gemm_bf16: ST_REQUIRE(a->K % BK == 0 && a->K2 % BK == 0, "gemm: K (%d) and K2 (%d) must be multiples of 64", ...)
    ("gemm K = 96", lambda m, t: m.gemm(t(64, 96), t(64, 96))),
    # gemm.hip st355_gemm_tn_bf16: ST_REQUIRE(Mc % PQ_BK == 0, "gemm_tn: the contraction length (%lld rows) must be a multiple of 64 ...")
    ("gemm_tn contraction 96", lambda m, t: m.gemm_tn(t(96, 64), t(96, 64))),
    # reduce.hip st355_colsum_prod: ST_REQUIRE(N % 8 == 0 && lda % 8 == 0 && ..., "colsum_prod: alignment")
    ("colsum_prod N = 12", lambda m, t: m.colsum_prod(t(64, 16)[:, :12], torch.zeros(1, 12, device=t(1).device))),
    # reduce.hip st355_transpose_bf16: ST_REQUIRE(... rows % 8 == 0 && cols % 8 == 0 && ..., "transpose_bf16: bad args")
    ("transpose 12 rows", lambda m, t: m.transpose(t(12, 64))),
    # skinny.hip st355_skinny_tn_seg: ST_REQUIRE((Rn == 32 || Rn == 64) && r_used > 0 && r_used <= Rn, "skinny_tn: Rn must be 32 or 64 (got %d)", Rn)
    ("skinny_tn Rn = 48", lambda m, t: m.skinny_tn(t(256, 64), t(256, 48), torch.zeros(64, 48, device=t(1).device), 48, 1, 16)),
]


@pytest.mark.parametrize("name,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_precondition_raises_on_both_sides(ops, name, call):
    from simpletuner_amd.lib import St355Error

    with pytest.raises(EMU.EmuError):
        call(EMU, lambda *s: torch.ones(*s, dtype=BF16))
    with pytest.raises(St355Error):
        call(ops, _bf)
    torch.cuda.synchronize()


def test_report():
    """the worst ratios per family (profiles/emulator_bounds.md records them); run the module as a whole"""
    for fam, (elem, block, both) in sorted(WORST.items()):
        print(f"[emulator bounds, gpu] {fam}: worst dev |err| / tol = {elem:.3f}; worst block statistic / limit = {block:.3f}; "
              f"worst |dev - emu| / (tol_dev + tol_emu) = {both:.3f}")
    assert all(math.isfinite(v) for w in WORST.values() for v in w)

"""tests/ops_emulator.py held to the kernels' own fp64 element bounds, wrapper by wrapper, on the CPU: the table of tests/emulator_cases.py run on the emulator.
For every case each stored output stays inside the family's element rule (or is bit-equal for the exact kinds), everything outside the owned region of every
backing buffer keeps its bits, and the returned object is the view that was passed in.  The 64 x 64 block rounding statistic is NOT asserted here: it measures
the kernel's rounding behaviour (tests/test_ops_emulator_bounds_gpu.py asserts it on the device).  The same table runs on the MI355X there, so one reference and
one bound judge both sides of the boundary the CPU host-sequencing tests rest on."""
import inspect
import math
import time

import pytest
import torch

from tests import emulator_cases as EC
from tests import ops_emulator as EMU

BF16 = torch.bfloat16
WORST = {}
SECONDS = {}

# wrappers of ops_emulator._EMULATED that need no case of their own, with the reason
EXEMPT = {
    "grid_rows": "pure host helper (an integer)",
    "grid_zeros": "pure host helper (torch.zeros of grid_rows)",
    "block_pixart_fwd": "a sequence of the wrappers pinned here; both sides are held bit-identical to the host sequencing (tests/test_pixart_model_gpu.py)",
    "block_pixart_bwd": "a sequence of the wrappers pinned here; both sides are held bit-identical to the host sequencing (tests/test_pixart_model_gpu.py)",
    "block_sd3_joint_fwd": "a sequence of the wrappers pinned here; both sides are held bit-identical to the host sequencing (tests/test_sd3_model_gpu.py)",
    "block_sd3_joint_bwd": "a sequence of the wrappers pinned here; both sides are held bit-identical to the host sequencing (tests/test_sd3_model_gpu.py)",
}

# the arguments that only seed the device's own Philox stream: the emulator draws from another generator (distributional equivalence only), so the
# cases pass what is random explicitly instead (noise= / rand_bits=) and these select nothing that could be compared
DEVICE_RANDOM = {"flow_noise_mix": {"seed", "offset"}, "adamw_bf16_sr_step": {"seed", "offset"}}


def check_case(case, mod, device=None):
    """run one case and apply the element rule, the guard check and the identity check; returns {label: worst ratio}"""
    ran, built = EC.run(case, mod, device)
    assert ran.guard_ok, f"{case.name}: {ran.guard_msg}"
    assert ran.same_ok, f"{case.name}: the wrapper did not return the view it was given"
    ratios = {}
    for label, want, e, kind, *extra in built.ref(ran.out):
        ex = extra[0] if extra else None
        assert label in ran.out or (ex and "out" in ex), f"{case.name}: output {label} was not produced"
        ratios[label] = EC.elem_ratio(ex["out"] if ex and "out" in ex else ran.out[label], want, e, kind, ex)
    assert ratios, case.name
    return ratios, ran


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_emulator_inside_the_kernel_bound(case):
    t0 = time.perf_counter()
    ratios, _ = check_case(case, EMU)
    SECONDS[case.name] = time.perf_counter() - t0
    for label, r in ratios.items():
        WORST[case.family] = max(WORST.get(case.family, 0.0), r)
        assert r <= 1.0, f"{case.name} {label}: worst |err| / tol = {r:.3f}"


def test_every_emulated_wrapper_has_a_case_for_every_optional_argument():
    names = {c.wrapper for c in EC.CASES}
    assert set(EXEMPT) <= set(EMU._EMULATED) and not (names & set(EXEMPT))
    assert names | set(EXEMPT) == set(EMU._EMULATED), (sorted(set(EMU._EMULATED) - names - set(EXEMPT)), sorted(names - set(EMU._EMULATED)))
    missing = {}
    for w in sorted(names):
        optional = {n for n, p in inspect.signature(getattr(EMU, w)).parameters.items() if p.default is not inspect.Parameter.empty}
        passed = set().union(*(c.opts for c in EC.CASES if c.wrapper == w))
        assert passed <= optional, (w, sorted(passed - optional))
        if optional - passed - DEVICE_RANDOM.get(w, set()):
            missing[w] = sorted(optional - passed - DEVICE_RANDOM.get(w, set()))
    assert not missing, missing


# ---- the check must bite: three modelled defects on a patched copy of an emulated wrapper ---------------------------------------------------------------------
def _old_close(a, b, tol=1e-2):
    """the criterion of tests/test_ops_emulator_crosscheck_gpu.py"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item() < tol


class _Patched:
    """the emulator with one wrapper replaced"""

    def __init__(self, name, fn):
        self._name, self._fn = name, fn

    def __getattr__(self, name):
        return self._fn if name == self._name else getattr(EMU, name)


def _case(name):
    return next(c for c in EC.CASES if c.name == name)


def _fails_new_passes_old(case, patched, label="out"):
    clean, _ = EC.run(case, EMU)
    ran, built = EC.run(case, patched)
    assert _old_close(ran.out[label], clean.out[label]), "the defect must pass the old criterion for this test to mean anything"
    if not ran.guard_ok:
        return True
    return any(EC.elem_ratio(ran.out[lab], want, e, kind) > 1.0 for lab, want, e, kind in built.ref(ran.out))


def test_defect_one_element_off_by_its_own_magnitude():
    def gemm(*a, **kw):
        out = EMU.gemm(*a, **kw)
        out[37, 101] = out[37, 101] * 2
        return out
    assert _fails_new_passes_old(_case("gemm_none"), _Patched("gemm", gemm))


def test_defect_truncation_instead_of_rne_at_the_bf16_store(monkeypatch):
    def put_trunc(dst, val):
        v = val.reshape(dst.shape).float().contiguous()
        dst.copy_((v.view(torch.int32) & -65536).view(torch.float32).to(dst.dtype) if dst.dtype == BF16 else v)
        return dst
    case = _case("gemm_none")
    clean, _ = EC.run(case, EMU)
    monkeypatch.setattr(EMU, "_put", put_trunc)
    ran, built = EC.run(case, EMU)
    monkeypatch.undo()
    assert _old_close(ran.out["out"], clean.out["out"])
    assert max(EC.elem_ratio(ran.out[lab], want, e, kind) for lab, want, e, kind in built.ref(ran.out)) > 1.0


def test_defect_store_one_row_past_the_owned_block():
    def gemm(*a, **kw):
        out = EMU.gemm(*a, **kw)
        past = torch.as_strided(out, (1, out.shape[1]), out.stride(), out.storage_offset() + out.shape[0] * out.stride(0))
        past.copy_(out[-1:])
        return out
    case = _case("gemm_none")
    ran, _ = EC.run(case, _Patched("gemm", gemm))
    clean, _ = EC.run(case, EMU)
    assert _old_close(ran.out["out"], clean.out["out"]) and torch.equal(EC.bits(ran.out["out"]), EC.bits(clean.out["out"]))
    assert not ran.guard_ok and "outside the owned region" in ran.guard_msg


def test_report():
    """the worst element ratio per family and the run time (profiles/emulator_bounds.md records them); run the module as a whole"""
    for fam, w in sorted(WORST.items()):
        print(f"[emulator bounds, cpu] {fam}: worst |err| / tol = {w:.3f}")
    if SECONDS:
        slow = max(SECONDS, key=SECONDS.get)
        print(f"[emulator bounds, cpu] {len(SECONDS)} cases in {sum(SECONDS.values()):.2f} s; slowest {slow} {SECONDS[slow]:.2f} s")
    assert all(math.isfinite(w) for w in WORST.values())

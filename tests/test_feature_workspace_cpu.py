"""The six per-sample streaming losses (reflexflow, flow_dpo, twinflow, eval_loss, diff2flow, lcm) size their stage-1 workspace by ONE grid rule
(csrc/feature_common.h `sample_parts`): 256 lanes of 8 elements per partial workgroup, at most 2048 // batch of them per sample, at least one.  The rule is
written out again here, independently, and the library's `*_workspace` entries are held to it."""
import pytest

BATCHES = (1, 3, 300, 2048, 2049, 32767)
PER_SAMPLE = (8, 2048, 2056, 16384, 1 << 20)
TAILS = (1, 4099)          # diff2flow and lcm alone take a per-sample size that is no multiple of 8
EVAL_K = (1, 5, 64)


def _cdiv(a, b):
    return -(-a // b)


def _bytes(batch, n, accumulators):
    parts = max(1, min(_cdiv(_cdiv(n, 8), 256), 2048 // batch))
    return 4 * accumulators * batch * parts


def test_workspace_entries_follow_the_one_grid_rule():
    from simpletuner_amd import lib
    if not lib.is_built():
        pytest.skip("libst355.so is not built")
    L = lib.load()
    fixed = (("st355_reflexflow_workspace", 4, ()), ("st355_flow_dpo_workspace", 9, ()), ("st355_twinflow_workspace", 2, ()),
             ("st355_diff2flow_workspace", 1, TAILS), ("st355_lcm_workspace", 1, TAILS))
    for batch in BATCHES:
        for name, acc, extra in fixed:
            for n in PER_SAMPLE + extra:
                assert getattr(L, name)(batch, n) == _bytes(batch, n, acc), (name, batch, n)
        for n in PER_SAMPLE:
            for k in EVAL_K:
                assert L.st355_eval_loss_workspace(batch, n, k) == _bytes(batch, n, k), (batch, n, k)
    # nothing to size: no bytes
    for name, _, _ in fixed:
        assert getattr(L, name)(0, 2048) == 0 and getattr(L, name)(4, 0) == 0, name
    assert L.st355_eval_loss_workspace(4, 2048, 0) == 0

"""Activation-checkpoint segment plans: FluxTransformer2DModel._checkpoint_segments must cut the block stacks exactly where the
reference's `checkpoint_sequential_state` (helpers/training/gradient_checkpointing_interval.py:69-120) opens / closes its checkpoint calls, for the
published-table modes `layer`, `interval2`, `seg2-stride4` and a few others.  The reference's plans are executed results stored in
tests/golden/checkpoint_plan_vectors.json (tools/gen_checkpoint_plan_golden.py)."""
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "checkpoint_plan_vectors.json"


def _model():
    from simpletuner_amd.flux.transformer import FluxTransformer2DModel
    return FluxTransformer2DModel.__new__(FluxTransformer2DModel)


def test_segment_plans_equal_the_reference_helper():
    ref = json.loads(GOLDEN.read_text())
    cases = {(c["n"], c["interval"], c["stride"]) for c in ref["segmented"]}
    assert cases == {(n, i, s) for n in (19, 38, 5, 1) for i, s in ((2, None), (2, 4), (3, 3), (4, 6), (2, 2))}, cases
    m = _model()
    m.gradient_checkpointing = True
    for c in ref["segmented"]:
        m.gradient_checkpointing_interval, m.gradient_checkpointing_segment_stride = c["interval"], c["stride"]
        assert m._checkpoint_segments(c["n"]) == [tuple(seg) for seg in c["plan"]], (c["n"], c["interval"], c["stride"])
    # non-segmented: should_checkpoint_block(interval None) == every block its own checkpoint
    assert sorted(c["n"] for c in ref["every_block"]) == [1, 5, 19, 38]
    m.gradient_checkpointing_interval, m.gradient_checkpointing_segment_stride = None, None
    for c in ref["every_block"]:
        assert m._checkpoint_segments(c["n"]) == [(i, 1, ck) for i, ck in enumerate(c["checkpointed"])], c["n"]


def test_modes_off_layer_and_bad_stride():
    m = _model()
    m.gradient_checkpointing, m.gradient_checkpointing_interval, m.gradient_checkpointing_segment_stride = False, 2, 4
    assert m._checkpoint_segments(4) == [(0, 1, False), (1, 1, False), (2, 1, False), (3, 1, False)]
    m.gradient_checkpointing = True
    assert m._checkpoint_segments(6) == [(0, 2, True), (2, 1, False), (3, 1, False), (4, 2, True)]       # seg2-stride4
    m.gradient_checkpointing_segment_stride = 1
    with pytest.raises(ValueError, match="segment_stride must be at least"):
        m._checkpoint_segments(6)
    m.gradient_checkpointing_backend = "torch"
    with pytest.raises(NotImplementedError):
        m.set_gradient_checkpointing_backend("unsloth")

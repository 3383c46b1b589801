#!/usr/bin/env python3
"""Generate tests/golden/checkpoint_plan_vectors.json by EXECUTING the reference's activation-checkpoint helper
(simpletuner/helpers/training/gradient_checkpointing_interval.py, a pure-python module loaded from where it lies in a SimpleTuner checkout):
the block segments `checkpoint_sequential_state` opens / closes for every (block count, interval, stride) case of
tests/test_checkpoint_plan_cpu.py, and the answers of `should_checkpoint_block` without an interval.  Only the executed results are
written; the test reads them and never needs the reference tree.

    python tools/gen_checkpoint_plan_golden.py <SimpleTuner checkout>
"""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "checkpoint_plan_vectors.json"

PLAN_NS = (19, 38, 5, 1)
PLAN_MODES = ((2, None), (2, 4), (3, 3), (4, 6), (2, 2))


def checkpoint_plans(helper: Path) -> dict:
    spec = importlib.util.spec_from_file_location("ref_gci", str(helper))
    gci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gci)

    def plan(n, interval, stride):
        """[[first block, block count, checkpointed]] in the order the reference runs them"""
        log = []

        def run_block(i, blk, *st):
            log.append(("blk", i))
            return st

        def ck(fn, *st, **kw):
            log.append(("begin",))
            r = fn(*st)
            log.append(("end",))
            return r

        gci.checkpoint_sequential_state(list(range(n)), interval, (0,), run_block, ck, {}, stride)
        segs, cur = [], None
        for e in log:
            if e[0] == "begin":
                cur = []
            elif e[0] == "end":
                segs.append([cur[0], len(cur), True])
                cur = None
            elif cur is not None:
                cur.append(e[1])
            else:
                segs.append([e[1], 1, False])
        return segs

    return {
        "source": "simpletuner/helpers/training/gradient_checkpointing_interval.py: checkpoint_sequential_state, should_checkpoint_block (executed)",
        "segmented": [{"n": n, "interval": i, "stride": s, "plan": plan(n, i, s)} for n in PLAN_NS for i, s in PLAN_MODES],
        "every_block": [{"n": n, "checkpointed": [bool(gci.should_checkpoint_block(b, True, None)) for b in range(n)]} for n in PLAN_NS],
    }


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    helper = Path(argv[1]) / "simpletuner" / "helpers" / "training" / "gradient_checkpointing_interval.py"
    OUT.write_text(json.dumps(checkpoint_plans(helper), indent=1) + "\n")
    print(f"wrote {OUT.relative_to(OUT.parents[2])}")


if __name__ == "__main__":
    main(sys.argv)

#!/usr/bin/env python3
"""Generate tests/golden/lokr_vectors.pt by EXECUTING THE REFERENCE'S `approximate_normal_tensor` (helpers/training/peft_init.py, pure torch) on the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path, at generation time only; nothing of it is copied here and the tests read only the
recorded tensors and numbers.  `init_lokr_norm` fills every `lokr_w1` with 1 and hands (frozen weight, lokr_w2, scale) to that function; recorded per case:

  weight     the frozen weight (bf16 or fp32), seed, scale, and the fp32 w2 the function left behind after `torch.manual_seed(seed)` on the CPU

    python tools/gen_lokr_golden.py <SimpleTuner checkout>      (writes tests/golden/lokr_vectors.pt)
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "lokr_vectors.pt"
CASES = [dict(N=64, K=128, ok=32, in_=64, dtype=torch.bfloat16, seed=3, scale=1e-3), dict(N=48, K=64, ok=24, in_=8, dtype=torch.float32, seed=4, scale=0.5)]


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_peft_init", ref / "helpers/training/peft_init.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.approximate_normal_tensor


def main(ref: Path):
    fn = _load(ref / "simpletuner" if (ref / "simpletuner").is_dir() else ref)
    out = []
    for c in CASES:
        g = torch.Generator().manual_seed(100 + c["seed"])
        W = (0.01 + torch.randn(c["N"], c["K"], generator=g) / c["K"] ** 0.5).to(c["dtype"])
        w2 = torch.zeros(c["ok"], c["in_"], dtype=torch.float32)
        torch.manual_seed(c["seed"])
        with torch.no_grad():
            fn(W, w2, scale=c["scale"])
        out.append({"weight": W, "seed": c["seed"], "scale": c["scale"], "w2": w2})
    torch.save({"init_lokr_norm": out}, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main(Path(sys.argv[1]))

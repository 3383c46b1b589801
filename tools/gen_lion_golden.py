#!/usr/bin/env python3
"""Generate tests/golden/lion_vectors.pt: what the Lion tests share.

optimi is not vendored by the reference, so — unlike tools/gen_muon_golden.py — nothing is EXECUTED here.  What is recorded:

  default_settings   the registry entry "optimi-lion" (optimizer_param.py:327-338), read from the source with ast
  seeds              the torch.Generator seeds of the inputs tests/lion_bounds.make_inputs draws (g ~ N(0, 1), m ~ 0.5 N(0, 1), p ~ 0.05 N(0, 1), a leading
                     block of exact zeros, 64 elements built to cancel); the arenas themselves (up to 2 097 160 elements) are far above what a fixture may hold
  hyper              the hyper-parameters of the kernel cases (lr, betas, the two weight decays, grad_scale, ema_decay)
  sample             the first 2048 elements of the fp32 case's (g, m, p) as drawn here: tests/test_lion_cpu.py checks that make_inputs reproduces them

    python tools/gen_lion_golden.py <SimpleTuner checkout>      (writes tests/golden/lion_vectors.pt)
"""
from __future__ import annotations

import ast
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "lion_vectors.pt"
sys.path.insert(0, str(ROOT))


def _default_settings(ref: Path) -> dict:
    tree = ast.parse((ref / "helpers/training/optimizer_param.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Dict):
            for k, v in zip(node.keys, node.values):
                if isinstance(k, ast.Constant) and k.value == "optimi-lion" and isinstance(v, ast.Dict):
                    for k2, v2 in zip(v.keys, v.values):
                        if isinstance(k2, ast.Constant) and k2.value == "default_settings":
                            return ast.literal_eval(v2)
    raise KeyError("optimizer_param.py: no 'optimi-lion' entry")


def main(ref: Path):
    from tests import lion_bounds as LB
    out = {"default_settings": _default_settings(ref)}
    out["seeds"] = {"fp32": 7100, "bf16": 7200, "kahan": 7300, "optimizer": 7400, "trainer": 7500}
    out["hyper"] = dict(lr=1e-3, beta1=0.9, beta2=0.99, weight_decays=(0.0, 1e-2), grad_scale=0.5, ema_decay=0.99)
    x = LB.make_inputs(2097155, torch.float32, out["seeds"]["fp32"], grad_scale=out["hyper"]["grad_scale"], beta1=out["hyper"]["beta1"])
    out["sample"] = {k: x[k][:2048].clone() for k in ("g", "m", "p")}
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]) / "simpletuner")

#!/usr/bin/env python3
"""Generate tests/golden/layersync_vectors.pt by EXECUTING THE REFERENCE'S LayerSyncRegularizer (helpers/training/layersync.py, pure torch) on the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path, at generation time only; nothing of it is copied here and the tests read only the
recorded tensors, numbers and messages.  Recorded (B = 2, S = 24, D = 64, fp32):

  case            student / teacher hidden states, lambda, `compute_loss`'s loss and logs, autograd.grad of the loss with respect to the student
  zero_rows       the same with one all-zero student row and one all-zero teacher row: what F.normalize's clamp makes of them (loss, logs, gradient)
  same_layer      teacher block unset: the teacher is the student's own layer
  index_table     for student index in {0, 1, 2, 5}, teacher unset and teacher = 7: which captured layer `_resolve_layer` hands back, over the layers the reference
                  captures for LayerSync (common.py:5237-5243: idx and idx - 1)
  errors          the constructor's and the resolver's ValueError texts; the default lambda

    python tools/gen_layersync_golden.py <SimpleTuner checkout>      (writes tests/golden/layersync_vectors.pt)
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "layersync_vectors.pt"
B, S, D, N_LAYERS = 2, 24, 64, 8


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_layersync", ref / "helpers/training/layersync.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LayerSyncRegularizer


def _cfg(**kw):
    return SimpleNamespace(layersync_enabled=True, **kw)


def _captured(student, teacher):
    """the layer indices common.py:5237-5243 asks the transformer to capture"""
    out = set()
    for layer in (student, teacher):
        if layer is None:
            continue
        out.add(int(layer))
        if int(layer) > 0:
            out.add(int(layer) - 1)
    return sorted(i for i in out if 0 <= i < N_LAYERS)


def _run(Reg, cfg, student_h, teacher_h, s_key, t_key):
    reg = Reg(cfg)
    s = student_h.clone().requires_grad_(True)
    buf = {s_key: s} if t_key == s_key else {s_key: s, t_key: teacher_h.clone()}
    loss, logs = reg.compute_loss(buf)
    (g,) = torch.autograd.grad(loss, s)
    return {"student": student_h, "teacher": teacher_h, "weight": reg.weight, "loss": loss.detach(), "logs": dict(logs), "grad_student": g}


def _err(fn):
    try:
        fn()
    except ValueError as e:
        return str(e)
    raise AssertionError("expected a ValueError")


def main(ref: Path):
    Reg = _load(ref)
    g = torch.Generator().manual_seed(1234)
    student = torch.randn(B, S, D, generator=g)
    teacher = 0.6 * student + 0.8 * torch.randn(B, S, D, generator=g)
    out = {"shape": (B, S, D)}
    # student_block 3 -> layer_2, teacher_block 6 -> layer_5 (1-based depths)
    out["case"] = _run(Reg, _cfg(layersync_student_block=3, layersync_teacher_block=6, layersync_lambda=0.35), student, teacher, "layer_2", "layer_5")
    zs, zt = student.clone(), teacher.clone()
    zs[0, 3] = 0.0
    zt[1, 7] = 0.0
    out["zero_rows"] = dict(_run(Reg, _cfg(layersync_student_block=3, layersync_teacher_block=6), zs, zt, "layer_2", "layer_5"), zero_student_row=(0, 3), zero_teacher_row=(1, 7))
    out["same_layer"] = _run(Reg, _cfg(layersync_student_block=3), student, student, "layer_2", "layer_2")
    table = {}
    for si in (0, 1, 2, 5):
        for ti in (None, 7):
            buf = {f"layer_{i}": torch.full((1, 1, 1), float(i)) for i in _captured(si, ti)}
            table[(si, ti)] = (int(Reg._resolve_layer(buf, si, role="student").item()), int(Reg._resolve_layer(buf, ti if ti is not None else si, role="teacher").item()))
    out["index_table"] = table
    out["errors"] = {
        "no_student": _err(lambda: Reg(_cfg())),
        "bad_lambda": _err(lambda: Reg(_cfg(layersync_student_block=1, layersync_lambda=-0.5))),
        "negative_index": _err(lambda: Reg._resolve_layer({"layer_0": student}, -1, role="student")),
        "not_an_int": _err(lambda: Reg._resolve_layer({"layer_0": student}, "three", role="teacher")),
        "out_of_range": _err(lambda: Reg._resolve_layer({f"layer_{i}": student for i in range(N_LAYERS)}, N_LAYERS + 2, role="teacher")),
        "none_index": _err(lambda: Reg._resolve_layer({"layer_0": student}, None, role="student")),
        "no_buffer": _err(lambda: Reg(_cfg(layersync_student_block=1)).compute_loss(None)),
    }
    out["n_layers"] = N_LAYERS
    out["default_lambda"] = Reg(_cfg(layersync_student_block=1)).weight
    out["lambda_zero_means_default"] = Reg(_cfg(layersync_student_block=1, layersync_lambda=0)).weight
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))

"""Wide-arithmetic mode for the CPU engine tests — TEST INFRASTRUCTURE ONLY.

Every engine and feature module, the kernel-contract emulator and the feature stand-ins name their storage type through ONE module constant `BF16`.
`install(monkeypatch)` rebinds that constant to fp32 everywhere it is bound, so the same host sequencing (which kernel, on which view, which gradient term
lands where) runs with fp32 storage: the few-percent bf16 rounding noise through depth is gone and the engines' hand-written backward can be held to
autograd on the fp64 oracle four orders of magnitude tighter than the bf16 parity tests can (tests/engine_parity.py, tests/test_engine_algebra_cpu.py).

fp32 is the mode: the emulator's `.float()` intermediates cap what fp64 storage would buy.  The list below is explicit, and
tests/test_engine_algebra_cpu.py::test_every_module_that_binds_the_storage_constant_is_listed fails when a module under simpletuner_amd/ or a tests/*_ref.py
binds `BF16` without being listed here.  A plain function: it needs no conftest and no pytest setting; pytest's monkeypatch puts everything back."""
from __future__ import annotations

import importlib
import pathlib
import re

import torch

PRODUCT_MODULES = (
    "simpletuner_amd.ops", "simpletuner_amd.foundation", "simpletuner_amd.engine",
    "simpletuner_amd.flux.transformer", "simpletuner_amd.flux.model",
    "simpletuner_amd.sd3.transformer", "simpletuner_amd.sd3.model",
    "simpletuner_amd.pixart.transformer", "simpletuner_amd.pixart.model",
    "simpletuner_amd.unet.unet", "simpletuner_amd.sdxl.model", "simpletuner_amd.sd1x.model",
    "simpletuner_amd.vae.autoencoder_kl",
)
TEST_MODULES = (
    "tests.ops_emulator",
    "tests.dora_ref", "tests.lokr_ref", "tests.lora_dropout_ref", "tests.internal_guidance_ref", "tests.nextlat_ref", "tests.layersync_ref", "tests.reflexflow_ref",
    "tests.adafactor_ref",              # an optimizer stand-in, off the engine path: listed so that the completeness rule has no exceptions
)
MODULES = PRODUCT_MODULES + TEST_MODULES

_ASSIGNS = re.compile(r"^([A-Za-z0-9_]+(?:\s*,\s*[A-Za-z0-9_]+)*)\s*(?::[^=]+)?=[^=]")
_IMPORTS = re.compile(r"^(?:from\s+\S+\s+)?import\s+(.*)$")


def install(monkeypatch, dtype=torch.float32):
    """rebind `BF16` in every listed module to `dtype` and install the emulator; returns the patched simpletuner_amd.ops"""
    from tests import ops_emulator as EMU
    ops = EMU.install(monkeypatch)
    for name in MODULES:
        mod = importlib.import_module(name)
        assert hasattr(mod, "BF16"), f"{name} no longer binds BF16: drop it from tests/wide_arith.py"
        monkeypatch.setattr(mod, "BF16", dtype)
    return ops


def _binds(source: str) -> bool:
    """does this source bind the name BF16 at module level (assignment, tuple assignment or import)"""
    for line in source.splitlines():
        m = _ASSIGNS.match(line)
        if m and "BF16" in [n.strip() for n in m.group(1).split(",")]:
            return True
        m = _IMPORTS.match(line)
        if m and re.search(r"\bBF16\b", m.group(1)):
            return True
    return False


def modules_binding_the_constant(root: pathlib.Path):
    """dotted names of every module under simpletuner_amd/, every tests/*_ref.py and the emulator whose source binds `BF16` at module level"""
    files = sorted((root / "simpletuner_amd").rglob("*.py")) + sorted((root / "tests").glob("*_ref.py")) + [root / "tests" / "ops_emulator.py"]
    return [".".join(f.relative_to(root).with_suffix("").parts) for f in files if _binds(f.read_text())]

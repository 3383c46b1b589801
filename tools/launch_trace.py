"""Record the launch stream of the CPU engine tests, to show that a change to the host code did not change what a step launches.

    python tools/launch_trace.py OUT.txt [extra pytest arguments]

Runs the engine tests that execute against tests/ops_emulator.py (`-m "not gpu"`, the -k expression below) with every emulated `ops` wrapper wrapped, and
every stand-in that the feature reference modules (tests/*_ref.py: `STAND_INS`, LayerSync's two) install on top of them: before it runs, one line goes to OUT.txt — the wrapper's name and its arguments bound to the wrapper's signature (defaults filled in), tensors as dtype / shape /
stride, scalars by value.  An output the wrapper would allocate itself (`out=None`) is written as the tensor it returns, so who allocates a temporary does
not show; what the C entry point receives does.  `### <nodeid>` opens every test.  Run it at two commits and compare the files (`cmp`, `sha256sum`): the host
layer launches the same stream exactly when they are identical.  Worker processes a test spawns (the gloo replicas) are not traced; the single-process
reference run of the same step is.
"""
from __future__ import annotations

import functools
import inspect
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ENGINE_TESTS = "host_sequencing or host_loop or two_replicas or host_cpu or segments or finality"


def describe(v):
    if torch.is_tensor(v):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}/{list(v.stride())}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(describe(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {describe(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (bool, int, float, str, type(None))):
        return repr(v)
    if hasattr(v, "__dict__"):          # argument records (ops.qk_rope's namespace)
        return type(v).__name__ + describe(vars(v))
    return type(v).__name__


class LaunchTrace:
    def __init__(self, path):
        self.f = open(path, "w")

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def traced(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = dict(bound.arguments)
            late = [k for k in ("out",) if k in args and args[k] is None]
            if not late:
                self.f.write(f"{name} {describe(args)}\n")
                return fn(*a, **kw)
            res = fn(*a, **kw)
            for k in late:
                args[k] = res if torch.is_tensor(res) else None
            self.f.write(f"{name} {describe(args)}\n")
            return res

        return traced

    def pytest_configure(self, config):
        from tests import ops_emulator as EMU
        names, g = EMU._EMULATED, vars(EMU)

        def install(monkeypatch):
            from simpletuner_amd import ops
            for name in names:
                monkeypatch.setattr(ops, name, self.wrap(name, g[name]))
            return ops

        EMU.install = install
        # the features' stand-ins, installed on top of the emulator by their modules' own `install` (which read these at call time): wrapped in place
        from tests import diff2flow_ref, dora_ref, flow_dpo_ref, internal_guidance_ref, layersync_ref, lcm_ref, lora_dropout_ref, nextlat_ref, reflexflow_ref, self_flow_ref, tlora_ref, twinflow_ref
        for mod in (layersync_ref, nextlat_ref, internal_guidance_ref, lora_dropout_ref, dora_ref, reflexflow_ref, flow_dpo_ref, diff2flow_ref, tlora_ref, self_flow_ref, twinflow_ref, lcm_ref):
            table = getattr(mod, "STAND_INS", None) or {}
            for name, fn in table.items():
                if inspect.isfunction(fn):
                    table[name] = self.wrap(name, fn)
        for name in ("layersync_fwd", "layersync_inject"):
            setattr(layersync_ref, name, self.wrap(name, getattr(layersync_ref, name)))

    def pytest_runtest_setup(self, item):
        self.f.write(f"### {item.nodeid}\n")

    def pytest_unconfigure(self, config):
        self.f.close()


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(pytest.main([str(ROOT / "tests"), "-q", "-m", "not gpu", "-k", ENGINE_TESTS, "-p", "no:cacheprovider", *sys.argv[2:]],
                         plugins=[LaunchTrace(sys.argv[1])]))

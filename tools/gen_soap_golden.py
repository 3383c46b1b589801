#!/usr/bin/env python3
"""Generate tests/golden/soap_vectors.pt by EXECUTING THE REFERENCE'S SOAP (optimizers/soap/__init__.py, pure torch) on the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path.  Nothing of the reference is copied here; the tests read only the
recorded tensors, settings and state dicts.  Every run is recorded three times from the same inputs:
  traj          the class as it is (fp32 parameters, torch.linalg.eigh / qr in fp32)
  traj_f64dec   the same with eigh / qr routed through float64 (inputs cast up, results cast back) — the distance between the two is the
                reference's own sensitivity to its decompositions, and the tolerance of every test that compares against `traj`
  traj_signs    as `traj`, with the columns of every eigh / qr result multiplied by random signs
What is recorded (DESIGN.md §7 explains why it matters):
  one_sided_f3      [8, 40] and [40, 8], max_precond_dim=16 (the rank side only), precondition_frequency=3, 8 calls (two refreshes);
                    a state_dict() taken after call 4
  one_sided_f10     the same shapes, precondition_frequency=10, 22 calls (two refreshes)
  zero_first_grad   [8, 40] whose first gradient is exactly zero (lora_A while lora_B is still zero), with a [40, 8], frequency 3
  wd0, nobias, sb09 weight_decay=0, correct_bias=False, shampoo_beta=0.9
  two_sided         [8, 40] with the registry default max_precond_dim=10000: the 40 x 40 side has rank <= 8 * calls, its null-space basis is
                    arbitrary — the evidence for refusing that configuration
  default_settings  the registry entry (optimizer_param.py:415-431), read from the source with ast

    python tools/gen_soap_golden.py <SimpleTuner checkout>      (writes tests/golden/soap_vectors.pt)
"""
from __future__ import annotations

import ast
import copy
import importlib.util
import sys
from pathlib import Path

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "soap_vectors.pt"


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_soap", ref / "helpers/training/optimizers/soap/__init__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _default_settings(ref: Path) -> dict:
    tree = ast.parse((ref / "helpers/training/optimizer_param.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Dict):
            for k, v in zip(node.keys, node.values):
                if isinstance(k, ast.Constant) and k.value == "soap" and isinstance(v, ast.Dict):
                    for k2, v2 in zip(v.keys, v.values):
                        if isinstance(k2, ast.Constant) and k2.value == "default_settings":
                            return ast.literal_eval(v2)
    raise KeyError("optimizer_param.py: no 'soap' entry")


class _Decompositions:
    """torch.linalg.eigh / qr replaced for the duration of a run: through float64 and / or with random column signs"""

    def __init__(self, f64: bool, signs_seed=None):
        self.f64, self.gen = f64, None if signs_seed is None else torch.Generator().manual_seed(signs_seed)

    def _post(self, q, dtype):
        q = q.to(dtype)
        if self.gen is not None:
            q = q * (torch.randint(0, 2, (q.shape[1],), generator=self.gen).to(dtype) * 2 - 1)
        return q

    def __enter__(self):
        self.eigh, self.qr = torch.linalg.eigh, torch.linalg.qr

        def eigh(a, *args, **kw):
            lam, q = self.eigh(a.double() if self.f64 else a, *args, **kw)
            return lam.to(a.dtype), self._post(q, a.dtype)

        def qr(a, *args, **kw):
            q, r = self.qr(a.double() if self.f64 else a, *args, **kw)
            return self._post(q, a.dtype), r.to(a.dtype)

        torch.linalg.eigh, torch.linalg.qr = eigh, qr
        return self

    def __exit__(self, *exc):
        torch.linalg.eigh, torch.linalg.qr = self.eigh, self.qr


def _trajectory(mod, p0, grads, kw, dec, state_at=None):
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = mod.SOAP(ps, **kw)
    traj, sd = [], None
    with dec:
        for k, gs in enumerate(grads):
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            opt.step()
            traj.append([p.detach().clone() for p in ps])
            if state_at is not None and k == state_at:
                sd = copy.deepcopy(opt.state_dict())
    return traj, sd, copy.deepcopy(opt.state_dict())


def _run(mod, shapes, calls, seed, state_at=None, zero_first=(), **kw):
    g = torch.Generator().manual_seed(seed)
    p0 = [0.1 * torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (0.5 + 0.1 * k) for s in shapes] for k in range(calls)]
    for i in zero_first:
        grads[0][i].zero_()
    traj, sd, final = _trajectory(mod, p0, grads, kw, _Decompositions(False), state_at)
    t64, _, _ = _trajectory(mod, p0, grads, kw, _Decompositions(True))
    tsg, _, _ = _trajectory(mod, p0, grads, kw, _Decompositions(False, signs_seed=seed + 1000))
    dist = [[(a - b).abs().max().item() for a, b in zip(x, y)] for x, y in zip(traj, t64)]          # [call][matrix]
    move = max((a - b).abs().max().item() for a, b in zip(traj[1], p0))          # what the first update moves a parameter by
    return dict(shapes=shapes, p0=p0, grads=grads, traj=traj, traj_f64dec=t64, traj_signs=tsg, dist_f64dec=dist, one_step=move, settings=dict(kw),
                state_at=state_at, state_dict=sd, final_state_dict=final)


def main(ref: Path):
    mod = _load(ref)
    both = [(8, 40), (40, 8)]
    out = {}
    out["one_sided_f3"] = _run(mod, both, 8, 21, state_at=4, lr=1e-3, max_precond_dim=16, precondition_frequency=3)
    out["one_sided_f10"] = _run(mod, both, 22, 22, lr=1e-3, max_precond_dim=16, precondition_frequency=10)
    out["zero_first_grad"] = _run(mod, both, 8, 23, zero_first=(0,), lr=1e-3, max_precond_dim=16, precondition_frequency=3)
    out["wd0"] = _run(mod, both, 5, 24, lr=1e-3, max_precond_dim=16, precondition_frequency=3, weight_decay=0.0)
    out["nobias"] = _run(mod, both, 5, 25, lr=1e-3, max_precond_dim=16, precondition_frequency=3, correct_bias=False)
    out["sb09"] = _run(mod, both, 5, 26, lr=1e-3, max_precond_dim=16, precondition_frequency=3, shampoo_beta=0.9)
    out["two_sided"] = _run(mod, [(8, 40)], 14, 27, lr=1e-3, precondition_frequency=10)
    out["default_settings"] = _default_settings(ref)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    for k, v in out.items():
        if k != "default_settings":
            print(f"  {k}: one step moves {v['one_step']:.3e}; fp32 vs fp64-decomposition per call: " + " ".join(f"{max(d):.1e}" for d in v["dist_f64dec"]))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]) / "simpletuner")

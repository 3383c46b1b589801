#!/usr/bin/env python3
"""Time the Muon optimizer step over the Flux LoRA r32 adapter arenas ("all": 266 adapters, "all+ffs": 419) on one MI355X.

    python tools/muon_step_bench.py [--iters 20] [--rank 32]

Prints one JSON line per measurement: st355_muon_step over the whole arena (2 + 3 * ns_steps launches), the same step done matrix by matrix
with torch.mm (fp32, the reference's per-matrix loop without its aliasing; measured here only, never used by the product), and the fused
st355-adamw step over the same arena for comparison.  The adapter shapes are those flux/transformer.py's add_lora_adapter lays out
(A [r, in], B [out, r]) for the full-size model (D = 3072, 19 double + 38 single blocks)."""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

D, N_DOUBLE, N_SINGLE = 3072, 19, 38


def flux_adapter_shapes(target: str, r: int):
    """(in, out) of every adapted Linear, in arena order (flux/transformer.py add_lora_adapter)"""
    lin = []
    ffs = target == "all+ffs"
    for _ in range(N_DOUBLE):
        lin += [(D, D)] * 4                                     # to_q, to_k, to_v, to_out.0
        lin += [(D, D)] * 4                                     # add_q/k/v_proj, to_add_out
        if ffs:
            lin += [(D, 4 * D), (4 * D, D), (D, 4 * D), (4 * D, D)]   # ff.net.0.proj, ff.net.2, ff_context.net.0.proj, ff_context.net.2
    for _ in range(N_SINGLE):
        lin += [(D, D)] * 3                                     # to_q, to_k, to_v
        if ffs:
            lin += [(D, 4 * D), (5 * D, D)]                     # proj_mlp, proj_out
    if ffs:
        lin += [(D, 64)]                                        # the output projection proj_out
    shapes = []
    for k, n in lin:
        shapes += [(r, k), (n, r)]
    return shapes


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def torch_mm_step(mats, grads, moms, lr=2e-4, mu=0.95, wd=0.1, coeffs=(3.4445, -4.7750, 2.0315), steps=5):
    a, b, c = coeffs
    for p, g, m in zip(mats, grads, moms):
        m.lerp_(g, 1 - mu)
        X = m.T if m.shape[0] > m.shape[1] else m
        X = X / X.norm().clamp(min=1e-7)
        for _ in range(steps):
            A = torch.mm(X, X.T)
            B = torch.addmm(A, A, A, beta=b, alpha=c)
            X = torch.addmm(X, B, X, beta=a)
        O = (X.T if m.shape[0] > m.shape[1] else X) * (math.sqrt(max(m.shape)) * 0.2)
        p.add_(p, alpha=-lr * wd)
        p.add_(O, alpha=-lr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rank", type=int, default=32)
    args = ap.parse_args()
    from simpletuner_amd import ops
    from simpletuner_amd.training.optimizer import St355AdamW, St355Muon
    dev = torch.device("cuda:0")
    for target in ("all", "all+ffs"):
        shapes = flux_adapter_shapes(target, args.rank)
        n = sum(r * c for r, c in shapes)
        gen = torch.Generator(device=dev).manual_seed(0)
        flat = 1e-2 * torch.randn(n, device=dev, generator=gen)
        gflat = torch.randn(n, device=dev, generator=gen)
        ps, off = [], 0
        for r, c in shapes:
            p = torch.nn.Parameter(flat[off:off + r * c].view(r, c))
            p.grad = gflat[off:off + r * c].view(r, c)
            ps.append(p)
            off += r * c
        opt = St355Muon(ps, lr=2e-4)
        ms = _time(opt.step, args.iters)
        plan = opt._flat[0]["plan"]
        flops = sum(4.0 * ((min(s) + 31) // 32 * 32) ** 2 * max(s) * 5 for s in shapes)
        print(json.dumps({"target": target, "what": "st355_muon_step", "matrices": len(shapes), "params": n, "ms": round(ms, 4),
                          "launches": plan.launches(5), "workspace_MiB": round(plan.ws_floats * 4 / 2**20, 1),
                          "ns_gflop": round(flops / 1e9, 2), "ns_tflops": round(flops / ms / 1e9, 2)}), flush=True)
        adam = St355AdamW(ps, lr=2e-4)
        print(json.dumps({"target": target, "what": "st355-adamw step (same arena)", "ms": round(_time(adam.step, args.iters), 4)}), flush=True)
        if target == "all":
            mats = [p.detach() for p in ps]
            grads = [p.grad for p in ps]
            moms = [torch.zeros_like(m) for m in mats]
            t = _time(lambda: torch_mm_step(mats, grads, moms), max(2, args.iters // 4))
            print(json.dumps({"target": target, "what": "matrix by matrix, torch.mm fp32", "matrices": len(shapes), "ms": round(t, 3)}), flush=True)
        del opt, adam, ps, flat, gflat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

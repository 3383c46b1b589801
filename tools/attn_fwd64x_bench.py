#!/usr/bin/env python
"""Time the head_dim-64 attention forward under the two forward choices, on one MI355X, one JSON line per shape.

    python tools/attn_fwd64x_bench.py [--window 0.25] [--reps 5] [--out FILE.jsonl]

Shapes: SD3 joint attention (B 2, H 24, S 4096 + 231), SDXL self-attention with the rounding residual O_res (B 16: H 10 at S 4096, H 20 at S 1024) and SDXL
cross-attention against the 77 text keys (B 16, H 10, Sq 4096, with O_res as the UNet calls it).
  fwd64:  ops.attn_set_impl(fwd=64), the default: k_attn_fwd4<64> (32 queries per wave);
  fwd64x: ops.attn_set_impl(fwd=2): k_attn_fwd64x (64 queries per wave, csrc/attention_fwd64x.hip).
Each side runs the same ops.attn_fwd / ops.attn_cross_fwd call on the same operands; the choice is set once, outside the timed window.  A window is `iters`
back-to-back launches between two device events after a warm-up, with `iters` sized per shape from a first timing of the default side so that a window lasts
at least `--window` seconds (`--iters` fixes it instead); `reps` windows per side, the two sides alternated; the line carries the median and the min .. max of the reps, the FLOP rate the algorithm needs
(4 B H Sq Sk d) and the largest difference of the two sides' outputs."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
D = 64
SHAPES = (("sd3 joint S4327", 2, 24, 4327, 4327, False), ("sdxl self S4096 O_res", 16, 10, 4096, 4096, True), ("sdxl self S1024 O_res", 16, 20, 1024, 1024, True),
          ("sdxl cross Sq4096 Sk77 O_res", 16, 10, 4096, 77, True))
IMPL = {"fwd64": 64, "fwd64x": 2}


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=0, help="launches per timed window; 0: sized per shape from --window")
    ap.add_argument("--window", type=float, default=0.25, help="least length of a timed window in seconds")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    bf = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    lines = []
    prev = ops.attn_set_impl()
    try:
        for name, B, H, Sq, Sk, res in SHAPES:
            Skp, scale = (Sk + 63) // 64 * 64, 1.0 / math.sqrt(D)
            Q, K = bf(B, H, Sq, D), bf(B, H, Sk, D)
            Vt = torch.zeros(B, H, D, Skp, dtype=torch.bfloat16, device=dev)
            Vt[..., :Sk] = bf(B, H, D, Sk)
            out = {r: (torch.empty(B * Sq, H * D, dtype=torch.bfloat16, device=dev), torch.empty(B * Sq, H * D, dtype=torch.bfloat16, device=dev) if res else None,
                       torch.empty(B, H, Sq, dtype=torch.float32, device=dev)) for r in IMPL}

            def run(r):
                O, R, lse = out[r]
                if Sq == Sk:
                    ops.attn_fwd(Q, K, Vt, O, lse, B, H, Sk, Skp, D, scale, O_res=R)
                else:
                    ops.attn_cross_fwd(Q, K, Vt, O, lse, B, H, Sq, Sk, Skp, D, scale, O_res=R)

            plan = {}
            for r in IMPL:
                ops.attn_set_impl(fwd=IMPL[r])
                plan[r] = ops.attn_plan(B, H, Sq, Sk, D, O_res=res)["fwd"]
            ops.attn_set_impl(fwd=IMPL["fwd64"])
            iters = a.iters or max(20, math.ceil(a.window / timed(lambda: run("fwd64"), 20)))
            t = {r: [] for r in IMPL}
            for _ in range(a.reps):
                for r in IMPL:
                    ops.attn_set_impl(fwd=IMPL[r])
                    t[r].append(timed(lambda: run(r), iters))
            flops = 4.0 * B * H * Sq * Sk * D
            rec = {"shape": name, "B": B, "H": H, "Sq": Sq, "Sk": Sk, "d": D, "O_res": res, "iters": iters, "reps": a.reps, "kernels": plan,
                   "max_abs_dO": float((out["fwd64"][0].float() - out["fwd64x"][0].float()).abs().max()),
                   "max_abs_dlse2": float((out["fwd64"][2] - out["fwd64x"][2]).abs().max())}
            for r, ts in t.items():
                med = statistics.median(ts)
                rec[f"{r}_us"] = round(med * 1e6, 1)
                rec[f"{r}_us_min_max"] = [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]
                rec[f"{r}_tflops"] = round(flops / med / 1e12, 1)
            rec["speedup"] = round(rec["fwd64_us"] / rec["fwd64x_us"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    finally:
        ops.attn_set_impl(fwd=prev[0])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

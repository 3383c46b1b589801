#!/usr/bin/env python
"""Time the quantised attention forward (csrc/attention_sage.hip) against ops.attn_fwd on the same operands, on one MI355X, one JSON line per shape, and
measure its accuracy against exact fp64 attention on the bf16 operands.

    python tools/attn_sage_bench.py [--window 0.25] [--reps 5] [--out FILE.jsonl]

Shapes: Flux (B 1, H 24, S 4608, d 128), SD3 (B 2, H 24, S 4250, d 64) and one short one (B 2, H 24, S 333, d 64), Gaussian operands.
  quant:  ops.attn_sage_quantize (four launches);   main: st355_attn_sage_fwd alone on the workspace quantised once;   sum: ops.attn_sage_fwd (both);
  bf16:   ops.attn_fwd.
Each side is timed with device events over back-to-back runs after a warm-up; the number of runs is chosen per side from a first estimate so that one timed
window lasts about `window` seconds (0.25 s: 500 .. 25 000 runs), `reps` windows per side, the sides alternated; the line carries the median and the
min .. max of the windows.  TFLOP/s count 4 B H S^2 d for both.  Accuracy (rel-L1 and cosine of O against fp64 attention, first head of the first sample) is
given for both kernels."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
BF16, F32 = torch.bfloat16, torch.float32


def timed(fn, iters):
    for _ in range(3):
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
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back runs per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, B, H, S, d in (("flux", 1, 24, 4608, 128), ("sd3", 2, 24, 4250, 64), ("short", 2, 24, 333, 64)):
        Sp, scale = (S + 63) // 64 * 64, 1.0 / math.sqrt(d)
        Q, K, V = (torch.randn(B, H, S, d, device=dev, generator=g).to(BF16) for _ in range(3))
        Vt = torch.zeros(B, H, d, Sp, dtype=BF16, device=dev)
        Vt[..., :S] = V.transpose(2, 3)
        O, Ob = (torch.empty(B * S, H * d, dtype=BF16, device=dev) for _ in range(2))
        lse = torch.empty(B, H, S, dtype=F32, device=dev)
        L = lib.load()
        ws = ops._scratch("attn_sage", dev, L.st355_attn_sage_workspace(B, H, S, d))          # the buffer ops.attn_sage_quantize fills

        def main_only():
            lib.check(L.st355_attn_sage_fwd(torch.cuda.current_stream().cuda_stream, ws.data_ptr(), O.data_ptr(), O.stride(0), B, H, S, Sp, d, scale), "attn_sage_fwd")

        sides = {"quant": lambda: ops.attn_sage_quantize(Q, K, Vt, B, H, S, Sp, d), "main": main_only,
                 "sage": lambda: ops.attn_sage_fwd(Q, K, Vt, O, B, H, S, Sp, d, scale), "bf16": lambda: ops.attn_fwd(Q, K, Vt, Ob, lse, B, H, S, Sp, d, scale)}
        sides["quant"]()
        iters = {n: max(20, int(a.window / timed(fn, 20))) for n, fn in sides.items()}
        t = {n: [] for n in sides}
        for _ in range(a.reps):
            for n, fn in sides.items():
                t[n].append(timed(fn, iters[n]))
        rec = {"shape": name, "B": B, "H": H, "S": S, "d": d, "window_s": a.window, "iters": iters, "reps": a.reps}
        for n, ts in t.items():
            rec[f"{n}_us"] = round(statistics.median(ts) * 1e6, 1)
            rec[f"{n}_us_min_max"] = [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]
        flops = 4.0 * B * H * S * S * d
        rec["main_tflops"], rec["sage_tflops"], rec["bf16_tflops"] = (round(flops / (rec[k] * 1e-6) / 1e12, 1) for k in ("main_us", "sage_us", "bf16_us"))
        q, k, v = (x[0, 0].double() for x in (Q, K, V))
        ref = torch.softmax(q @ k.T * scale, -1) @ v
        for n, out in (("sage", O), ("bf16", Ob)):
            o = out[:S, :d].double()
            rec[f"{n}_rel_l1"] = float(f"{float((o - ref).abs().sum() / ref.abs().sum()):.3e}")
            rec[f"{n}_cosine"] = round(float(torch.cosine_similarity(o.flatten(), ref.flatten(), 0)), 6)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

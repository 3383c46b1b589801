#!/usr/bin/env python
"""Time the fused head_dim-512 attention (csrc/attention_d512.hip) against the launch sequence it replaces in the AutoencoderKL mid block, on one MI355X, one JSON
line per shape.

    python tools/attn_d512_bench.py [--repeats 5] [--shapes 4096:4,16384:4,65536:1] [--out FILE.jsonl]

Shapes S:B — the mid block at 512^2 (S 4096), 1024^2 (S 16384) and 2048^2 (S 65536) pixels.  Operands are the three 512-column thirds of one [B S, 1536] qkv
buffer, as the VAE passes them.  `fused`: one ops.attn_d512_fwd launch for all images.  `sequence`: per image, GEMM (q k^T -> [S, S] bf16), in-place row softmax,
transpose of V, GEMM (P V) — the kernels of the default route, on preallocated buffers.  The two alternate in one process, `repeats` timed windows each (device
events around `iters` back-to-back runs, iters sized to ~0.3 s, after a warm-up of both); the line carries the median and the min-max spread of the windows.
FLOPs are what the algorithm needs, 4 B S^2 512; bytes the operands and the result once.  Roofline: the larger of FLOPs / 2.5 PFLOP/s (dense bf16 MFMA peak) and
bytes / 8 TB/s — at these shapes always the FLOPs.  Also reports the largest |fused - sequence| output difference (the sequence rounds its scores to bf16)."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="4096:4,16384:4,65536:1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import ops
    dev, d = torch.device("cuda:0"), 512
    scale = 1.0 / math.sqrt(d)
    lines = []
    for S, B in (tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")):
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = torch.randn(B * S, 3 * d, device=dev, generator=g).to(torch.bfloat16)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        o_f, o_s = torch.empty(B * S, d, dtype=torch.bfloat16, device=dev), torch.empty(B * S, d, dtype=torch.bfloat16, device=dev)
        scores, vt = torch.empty(S, S, dtype=torch.bfloat16, device=dev), torch.empty(d, S, dtype=torch.bfloat16, device=dev)      # S % 64 == 0: no padding

        def fused():
            ops.attn_d512_fwd(q, k, v, o_f, None, B, 1, S, S, d, scale)

        def sequence():
            for b in range(B):
                r = slice(b * S, (b + 1) * S)
                ops.gemm(q[r], k[r], out=scores)
                ops.softmax_rows_(scores, scale)
                ops.transpose(v[r], out=vt)
                ops.gemm(scores, vt, out=o_s[r])

        t = {}
        for name, fn in (("fused", fused), ("sequence", sequence)):      # warm-up, and the size of a ~0.3 s window
            fn()
            torch.cuda.synchronize()
            t[name] = max(1, int(0.3 / window(fn, 2)))
        diff = float((o_f.float() - o_s.float()).abs().max())
        wins = {"fused": [], "sequence": []}
        for _ in range(a.repeats):
            for name, fn in (("fused", fused), ("sequence", sequence)):
                wins[name].append(window(fn, t[name]))
        fl, by = 4.0 * B * S * S * d, 2.0 * 4 * B * S * d
        roof = max(fl / PEAK_FLOPS, by / PEAK_BYTES)
        rec = {"S": S, "B": B, "d": d, "repeats": a.repeats, "roofline_ms": round(roof * 1e3, 3), "bound": "flops" if fl / PEAK_FLOPS >= by / PEAK_BYTES else "bytes",
               "max_abs_diff": diff}
        for name in ("fused", "sequence"):
            med = statistics.median(wins[name])
            rec.update({f"{name}_ms": round(med * 1e3, 3), f"{name}_min_ms": round(min(wins[name]) * 1e3, 3), f"{name}_max_ms": round(max(wins[name]) * 1e3, 3),
                        f"{name}_tflops": round(fl / med / 1e12, 1), f"{name}_iters": t[name]})
        rec["fused_share_of_peak"] = round(roof / statistics.median(wins["fused"]), 3)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del qkv, scores, vt, o_f, o_s
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

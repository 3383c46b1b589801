#!/usr/bin/env python
"""Time the three head_dim-160 attention kernels (csrc/attention_wide.hip) on one MI355X, one JSON line per shape.

    python tools/attn_wide_bench.py [--iters 50] [--out FILE.jsonl]

Shapes: SD 1.5 at 512 px, per-GPU batch 16, 8 heads: the 16^2 level's self-attention (S 256) and cross-attention (Sk 77), and the 8^2 mid block (S 64).  Operands are
column blocks of fused [B S, 3 D] / [B Sk, 2 D] projection buffers, as the UNet passes them.  Each kernel is timed with device events over `iters` back-to-back
launches after a warm-up; FLOPs are what the algorithm needs (forward 4 B H Sq Sk d; dq: 5 GEMMs = 10 B H Sq Sk d, its first pass recomputes S and dP; dk/dv:
4 GEMMs = 8 B H Sq Sk d), bytes the operands and results once.  The backward's two kernels are timed together (one entry point) and dq alone is not separable
from outside, so the line carries forward and backward.  Roofline: the larger of FLOPs / 2.5 PFLOP/s (dense bf16 MFMA peak) and bytes / 8 TB/s."""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def timed(fn, iters):
    for _ in range(5):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import ops
    dev, d, H, B = torch.device("cuda:0"), 160, 8, 16
    D = H * d
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, Sq, Sk in (("self S256", 256, 256), ("cross S256 Sk77", 256, 77), ("self S64 (mid block)", 64, 64)):
        self_attn = Sq == Sk
        qbuf = torch.randn(B * Sq, 3 * D if self_attn else D, device=dev, generator=g).to(torch.bfloat16)
        kvbuf = qbuf if self_attn else torch.randn(B * Sk, 2 * D, device=dev, generator=g).to(torch.bfloat16)
        q, k, v = (qbuf[:, :D], qbuf[:, D:2 * D], qbuf[:, 2 * D:]) if self_attn else (qbuf, kvbuf[:, :D], kvbuf[:, D:])
        dO = torch.randn(B * Sq, D, device=dev, generator=g).to(torch.bfloat16)
        O, lse = torch.empty_like(dO), torch.empty(B, H, Sq, device=dev)
        dqb, dkvb = torch.empty_like(qbuf), torch.empty_like(kvbuf)
        dq, dk, dv = (dqb[:, :D], dqb[:, D:2 * D], dqb[:, 2 * D:]) if self_attn else (dqb, dkvb[:, :D], dkvb[:, D:])
        scale = 1.0 / math.sqrt(d)
        t_f = timed(lambda: ops.attn_wide_fwd(q, k, v, O, lse, B, H, Sq, Sk, d, scale), a.iters)
        t_b = timed(lambda: ops.attn_wide_bwd(q, k, v, dO, lse, dq, dk, dv, B, H, Sq, Sk, d, scale), a.iters)
        unit = 2.0 * B * H * Sq * Sk * d
        rows = 2.0 * B * H * d
        fl_f, by_f = 2 * unit, rows * (2 * Sq + 2 * Sk)
        fl_b, by_b = 9 * unit, rows * (5 * Sq + 6 * Sk)          # dq reads q, dO, k, v and writes dq; dk/dv reads q, dO, k, v and writes dk, dv
        roof = lambda fl, by: max(fl / PEAK_FLOPS, by / PEAK_BYTES)
        rec = {"shape": name, "B": B, "H": H, "Sq": Sq, "Sk": Sk, "d": d, "iters": a.iters,
               "fwd_us": round(t_f * 1e6, 2), "fwd_tflops": round(fl_f / t_f / 1e12, 1), "fwd_roofline_us": round(roof(fl_f, by_f) * 1e6, 2),
               "bwd_us": round(t_b * 1e6, 2), "bwd_tflops": round(fl_b / t_b / 1e12, 1), "bwd_roofline_us": round(roof(fl_b, by_b) * 1e6, 2)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

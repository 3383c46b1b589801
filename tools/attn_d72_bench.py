#!/usr/bin/env python
"""Time the head_dim-72 attention kernels (csrc/attention_d72.hip) against the padded d-96 sequence they replace in a PixArt block, on one MI355X, one JSON
line per shape.

    python tools/attn_d72_bench.py [--iters 10] [--reps 5] [--out FILE.jsonl] [--only self|cross]

Shapes: PixArt-Sigma, 16 heads of 72 channels at head pitch 96: self-attention at S 4096 (B 2) and S 16384 (B 1), cross-attention of both against 300 caption
keys with a key bias (-10000 on the last third of the keys).  Operands are the column blocks of qkv [B S, 3 Dp] / q2 [B S, Dp] / kv [B Sk, 2 Dp], as
PixArtTransformer2DModel._block_fwd / _block_bwd pass them.
  d72:    ops.attn_d72_fwd and ops.attn_d72_bwd (two kernels, one entry point), writing dq / dk / dv into the column blocks of dqkv / dq2 / dkv.
  padded: what the per-kernel sequencing runs with the switch off — forward: head_split x 3, attn_fwd / attn_cross_fwd at d 96; backward: attn_bwd /
          attn_cross_bwd at d 96, head_merge x 2.
Each side is timed with device events over `iters` back-to-back runs after a warm-up, `reps` times, the two sides alternated; the line carries the median and
the min .. max of the reps.  FLOPs are what the algorithm needs at d 72 (forward 4 B H Sq Sk d; backward 14 B H Sq Sk d)."""
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
H, D, HP = 16, 72, 96


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


def routes(ops, qsrc, kvsrc, B, S, Sk, kbias, dO):
    """{route: (forward, backward)} on the same projection buffers"""
    Dp, dev, self_attn, scale = H * HP, qsrc.device, qsrc is kvsrc, 1.0 / math.sqrt(D)
    q = qsrc[:, :Dp]
    k, v = (kvsrc[:, Dp:2 * Dp], kvsrc[:, 2 * Dp:]) if self_attn else (kvsrc[:, :Dp], kvsrc[:, Dp:])
    blocks = lambda dq_src, dkv_src: (dq_src[:, :Dp],) + ((dkv_src[:, Dp:2 * Dp], dkv_src[:, 2 * Dp:]) if self_attn else (dkv_src[:, :Dp], dkv_src[:, Dp:]))
    new = lambda: (torch.empty(B * S, Dp, dtype=BF16, device=dev), torch.empty(B, H, S, dtype=F32, device=dev))
    st, sp = {}, {}

    def d72_fwd():
        st["O"], st["lse"] = new()
        ops.attn_d72_fwd(q, k, v, st["O"], st["lse"], B, H, S, Sk, D, scale, pitch=HP, key_bias=kbias)

    def d72_bwd():
        dq_src = torch.empty_like(qsrc)
        dq, dk, dv = blocks(dq_src, dq_src if self_attn else torch.empty_like(kvsrc))
        ops.attn_d72_bwd(q, k, v, st["O"], dO, st["lse"], dq, dk, dv, B, H, S, Sk, D, scale, pitch=HP, key_bias=kbias)

    def pad_fwd():
        Q, Qt, Sp = ops.head_split(q, B, H, HP, S, want_xt=not ops.ATTN_TR)
        K, Kt, Skp = ops.head_split(k, B, H, HP, Sk, want_xt=not ops.ATTN_TR)
        _, Vt, _ = ops.head_split(v, B, H, HP, Sk, want_x=False)
        O, lse = new()
        if self_attn:
            ops.attn_fwd(Q, K, Vt, O, lse, B, H, S, Sp, HP, scale)
        else:
            ops.attn_cross_fwd(Q, K, Vt, O, lse, B, H, S, Sk, Skp, HP, scale, key_bias=kbias)
        sp.update(Q=Q, Qt=Qt, K=K, Kt=Kt, Sp=Sp, Skp=Skp, O=O, lse=lse)

    def pad_bwd():
        dq_src = torch.empty_like(qsrc)
        dq, dk, dv = blocks(dq_src, dq_src if self_attn else torch.empty_like(kvsrc))
        dQ, dK = torch.empty_like(sp["Q"]), torch.empty_like(sp["K"])
        if self_attn:
            ops.attn_bwd(sp["Q"], sp["K"], sp["Qt"], sp["Kt"], v, sp["O"], dO, sp["lse"], dQ, dK, dv, B, H, S, sp["Sp"], HP, scale)
        else:
            ops.attn_cross_bwd(sp["Q"], sp["K"], sp["Qt"], sp["Kt"], v, sp["O"], dO, sp["lse"], dQ, dK, dv, B, H, S, sp["Sp"], Sk, sp["Skp"], HP, scale,
                               key_bias=kbias)
        ops.head_merge(dQ, dq, B, H, HP, S)
        ops.head_merge(dK, dk, B, H, HP, Sk)

    return {"d72": (d72_fwd, d72_bwd), "padded": (pad_fwd, pad_bwd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("self", "cross"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import ops
    dev, Dp = torch.device("cuda:0"), H * HP
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []

    def padded(rows, n):          # n head-padded projections side by side: zero pad lanes, as the padded weights produce them
        t = torch.zeros(rows, n * H, HP, dtype=BF16, device=dev)
        t[:, :, :D] = torch.randn(rows, n * H, D, device=dev, generator=g).to(BF16)
        return t.view(rows, n * Dp)

    for name, B, Sq, Sk in (("self S4096", 2, 4096, 4096), ("self S16384", 1, 16384, 16384), ("cross S4096 Sk300", 2, 4096, 300), ("cross S16384 Sk300", 1, 16384, 300)):
        self_attn = Sq == Sk
        if a.only and (a.only == "self") != self_attn:
            continue
        qbuf = padded(B * Sq, 3 if self_attn else 1)
        kvbuf = qbuf if self_attn else padded(B * Sk, 2)
        dO = padded(B * Sq, 1)
        kbias = None
        if not self_attn:
            kbias = torch.zeros(B, Sk, dtype=F32, device=dev)
            kbias[:, 2 * Sk // 3:] = -10000.0
        rt = routes(ops, qbuf, kvbuf, B, Sq, Sk, kbias, dO)
        t = {(r, p): [] for r in rt for p in ("fwd", "bwd")}
        for _ in range(a.reps):
            for r, (fwd, bwd) in rt.items():
                t[r, "fwd"].append(timed(fwd, a.iters))
                t[r, "bwd"].append(timed(bwd, a.iters))
        unit = 2.0 * B * H * Sq * Sk * D
        rec = {"shape": name, "B": B, "H": H, "Sq": Sq, "Sk": Sk, "d": D, "pitch": HP, "iters": a.iters, "reps": a.reps}
        for (r, p), ts in t.items():
            med = statistics.median(ts)
            rec[f"{r}_{p}_us"] = round(med * 1e6, 1)
            rec[f"{r}_{p}_us_min_max"] = [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]
            if r == "d72":
                rec[f"{r}_{p}_tflops"] = round((2 if p == "fwd" else 7) * unit / med / 1e12, 1)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

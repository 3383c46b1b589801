#!/usr/bin/env python
"""Time the head_dim-40 / 80 attention kernels (csrc/attention_narrow.hip) against the zero-padded route they replace, on one MI355X, one JSON line per shape.

    python tools/attn_narrow_bench.py [--iters 20] [--reps 5] [--out FILE.jsonl]

Shapes: SD 1.5 at 512 px, per-GPU batch 16, 8 heads: self-attention at the 64^2 level (S 4096, d 40) and the 32^2 level (S 1024, d 80), and the cross-attention
of both (Sk 77).  Operands are column blocks of fused [B S, 3 D] / [B Sk, 2 D] projection buffers, as the UNet passes them.
  narrow: ops.attn_narrow_fwd (with o_res in the self cases, as under a recording tape) and ops.attn_narrow_bwd (two kernels, one entry point).
  padded: what UNet2DConditionModel._attention runs for the same attention with the switch off — forward: head_split x 3, attn_fwd / attn_cross_fwd (O_res in the
          self cases), the slice copy of O out of the padded heads; backward: the zero-padded copies of V and dO, attn_bwd / attn_cross_bwd, the slice copy of dV,
          head_merge x 2.
Each side is timed with device events over `iters` back-to-back runs after a warm-up, `reps` times, the two sides alternated; the line carries the median and
the min .. max of the reps.  FLOPs are what the algorithm needs at the real d (forward 4 B H Sq Sk d; backward 14 B H Sq Sk d: 3 GEMMs in dq, 4 in dk / dv)."""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
BF16 = torch.bfloat16


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


def padded_route(ops, qsrc, kvsrc, qo, ko, vo, C_, B, S, Sk, H, dO):
    """the forward and backward closures of the padded route, statement for statement those of UNet2DConditionModel._attention under a recording tape"""
    hd = C_ // H
    hp = 64 if hd <= 64 else 96
    scale, dev, self_attn = 1.0 / math.sqrt(hd), qsrc.device, qsrc is kvsrc
    M, Mk, Cp = B * S, B * Sk, H * hp
    st = {}

    def pad_cols(t2d, rows):
        o = torch.zeros(rows, H, hp, dtype=BF16, device=dev)
        o[:, :, :hd] = t2d.reshape(rows, H, hd)
        return o.view(rows, Cp)

    def fwd():
        Q, Qt, Sp = ops.head_split(qsrc[:, qo:qo + C_], B, H, hp, S, d_src=hd, want_xt=not ops.ATTN_TR)
        K, Kt, Skp = ops.head_split(kvsrc[:, ko:ko + C_], B, H, hp, Sk, d_src=hd, want_xt=not ops.ATTN_TR)
        _, Vt, _ = ops.head_split(kvsrc[:, vo:vo + C_], B, H, hp, Sk, want_x=False, d_src=hd)
        Op = torch.empty(M, Cp, dtype=BF16, device=dev)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        Ores = torch.empty_like(Op) if self_attn else None
        if self_attn:
            ops.attn_fwd(Q, K, Vt, Op, lse, B, H, S, Sp, hp, scale, O_res=Ores)
        else:
            ops.attn_cross_fwd(Q, K, Vt, Op, lse, B, H, S, Sk, Skp, hp, scale, O_res=Ores)
        O = Op.view(M, H, hp)[:, :, :hd].reshape(M, C_)
        st.update(Q=Q, K=K, Qt=Qt, Kt=Kt, Sp=Sp, Skp=Skp, Op=Op, lse=lse, Ores=Ores, O=O)

    def bwd():
        Q, K = st["Q"], st["K"]
        dq_src = torch.empty_like(qsrc)
        dkv_src = dq_src if self_attn else torch.empty_like(kvsrc)
        dQ, dK = torch.empty_like(Q), torch.empty_like(K)
        v_rows, dOp = pad_cols(kvsrc[:, vo:vo + C_], Mk), pad_cols(dO, M)
        dv_rows = torch.empty(Mk, Cp, dtype=BF16, device=dev)
        if self_attn:
            ops.attn_bwd(Q, K, st["Qt"], st["Kt"], v_rows, st["Op"], dOp, st["lse"], dQ, dK, dv_rows, B, H, S, st["Sp"], hp, scale, O_res=st["Ores"])
        else:
            ops.attn_cross_bwd(Q, K, st["Qt"], st["Kt"], v_rows, st["Op"], dOp, st["lse"], dQ, dK, dv_rows, B, H, S, st["Sp"], Sk, st["Skp"], hp, scale,
                               O_res=st["Ores"])
        dkv_src[:, vo:vo + C_] = dv_rows.view(Mk, H, hp)[:, :, :hd].reshape(Mk, C_)
        ops.head_merge(dQ, dq_src[:, qo:qo + C_], B, H, hp, S, d_src=hd)
        ops.head_merge(dK, dkv_src[:, ko:ko + C_], B, H, hp, Sk, d_src=hd)

    return fwd, bwd


def narrow_route(ops, qsrc, kvsrc, qo, ko, vo, C_, B, S, Sk, H, dO):
    hd = C_ // H
    scale, dev, self_attn = 1.0 / math.sqrt(hd), qsrc.device, qsrc is kvsrc
    q, k, v = qsrc[:, qo:qo + C_], kvsrc[:, ko:ko + C_], kvsrc[:, vo:vo + C_]
    st = {}

    def fwd():
        O = torch.empty(B * S, C_, dtype=BF16, device=dev)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        Ores = torch.empty_like(O) if self_attn else None
        ops.attn_narrow_fwd(q, k, v, O, lse, B, H, S, Sk, hd, scale, o_res=Ores)
        st.update(O=O, lse=lse, Ores=Ores)

    def bwd():
        dq_src = torch.empty_like(qsrc)
        dkv_src = dq_src if self_attn else torch.empty_like(kvsrc)
        ops.attn_narrow_bwd(q, k, v, st["O"], dO, st["lse"], dq_src[:, qo:qo + C_], dkv_src[:, ko:ko + C_], dkv_src[:, vo:vo + C_], B, H, S, Sk, hd, scale,
                            o_res=st["Ores"])

    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from simpletuner_amd import ops
    dev, H, B = torch.device("cuda:0"), 8, 16
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, Sq, Sk, d in (("self S4096 d40", 4096, 4096, 40), ("self S1024 d80", 1024, 1024, 80), ("cross S4096 Sk77 d40", 4096, 77, 40),
                            ("cross S1024 Sk77 d80", 1024, 77, 80)):
        D, self_attn = H * d, Sq == Sk
        qbuf = torch.randn(B * Sq, 3 * D if self_attn else D, device=dev, generator=g).to(BF16)
        kvbuf = qbuf if self_attn else torch.randn(B * Sk, 2 * D, device=dev, generator=g).to(BF16)
        dO = torch.randn(B * Sq, D, device=dev, generator=g).to(BF16)
        offs = (0, D, 2 * D) if self_attn else (0, 0, D)
        routes = {"narrow": narrow_route(ops, qbuf, kvbuf, *offs, D, B, Sq, Sk, H, dO), "padded": padded_route(ops, qbuf, kvbuf, *offs, D, B, Sq, Sk, H, dO)}
        t = {(r, p): [] for r in routes for p in ("fwd", "bwd")}
        for _ in range(a.reps):
            for r, (fwd, bwd) in routes.items():
                t[r, "fwd"].append(timed(fwd, a.iters))
                t[r, "bwd"].append(timed(bwd, a.iters))
        unit = 2.0 * B * H * Sq * Sk * d
        rec = {"shape": name, "B": B, "H": H, "Sq": Sq, "Sk": Sk, "d": d, "iters": a.iters, "reps": a.reps}
        for (r, p), ts in t.items():
            med = statistics.median(ts)
            rec[f"{r}_{p}_us"] = round(med * 1e6, 1)
            rec[f"{r}_{p}_us_min_max"] = [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]
            if r == "narrow":
                rec[f"{r}_{p}_tflops"] = round((2 if p == "fwd" else 7) * unit / med / 1e12, 1)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

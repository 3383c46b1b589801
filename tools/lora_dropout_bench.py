#!/usr/bin/env python3
"""LoRA dropout: the three masked kernels against the unmasked routes they replace and against a materialising baseline, and the SD3-Medium LoRA step at
p = 0.1 against p = 0.

    python tools/lora_dropout_bench.py [--part kernels|step|both] [--batch 4] [--steps 6] [--iters 20]

Kernel shapes: SD3-Medium's adapted Linears at 1024^2 — M = batch * 4096 image rows, K = 1536, rank 32; the q / k / v group (G = 3, K2 = 128) and to_out (G = 1,
K2 = 64).  Per shape, medians over --iters launches timed with device events after 3 warm-up launches:
  fwd   ops.gemm(x, A_cat)                        | lora_down_drop            | mask export (uint8) -> x * mask per target -> ops.gemm per target
  dA    skinny_tn_multi / skinny_tn               | skinny_tn_drop[_multi]    | the same materialised x per target -> skinny_tn per target
  dx    ops.gemm(dy, W^T, a2 = U, b2 = A_cat_T)   | ops.gemm(dy, W^T) + lora_dx_drop | ops.gemm(dy, W^T) + per target: gemm(U_g, A_g^T) * mask, added
(the materialising baseline leaves the scale out: it would be one more pass).  One JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARCH = dict(num_layers=24, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536, pooled_projection_dim=2048,
            pos_embed_max_size=192, sample_size=128)
BF16, F32 = torch.bfloat16, torch.float32


def _median_ms(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def kernels(batch: int, iters: int):
    from simpletuner_amd import ops
    from simpletuner_amd.engine import LoraDropout
    dev = torch.device("cuda:0")
    M, K, rank, r_pad = batch * 4096, 1536, 32, 32
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(BF16)
    drop = LoraDropout(0.1, 5, 0, dev, calls=1)
    x, dy1, dy3 = rnd(M, K), rnd(M, K), rnd(M, 3 * K)
    for G, dy, N in ((3, dy3, 3 * K), (1, dy1, K)):
        K2 = (G * r_pad + 63) // 64 * 64
        streams = list(range(G))
        A_cat = torch.zeros(K2, K, dtype=BF16, device=dev)
        A_cat[:G * r_pad] = rnd(G * r_pad, K) * 0.03
        A_cat_T = A_cat.t().contiguous()
        U = rnd(M, K2)
        wT = rnd(K, N) * 0.03
        gA = [torch.zeros(rank, K, dtype=F32, device=dev) for _ in range(G)]
        T = torch.empty(M, K2, dtype=BF16, device=dev)
        dx = torch.empty(M, K, dtype=BF16, device=dev)
        xm = torch.empty(M, K, dtype=BF16, device=dev)
        tmp = torch.empty(M, K, dtype=BF16, device=dev)
        # the materialising baseline's per-target operands, padded to the GEMM's 64-wide granule once, outside the timed region
        A64 = [torch.zeros(64, K, dtype=BF16, device=dev) for _ in range(G)]
        U64 = [torch.zeros(M, 64, dtype=BF16, device=dev) for _ in range(G)]
        for gi in range(G):
            A64[gi][:r_pad] = A_cat[gi * r_pad:(gi + 1) * r_pad]
            U64[gi][:, :r_pad] = U[:, gi * r_pad:(gi + 1) * r_pad]
        A64T = [a.t().contiguous() for a in A64]

        def materialise(gi):
            torch.mul(x, ops.lora_dropout_mask(M, K, drop, streams[gi]), out=xm)
            return xm

        def fwd_mat():
            for gi in range(G):
                ops.gemm(materialise(gi), A64[gi])

        def dA_plain():
            if G > 1:
                ops.skinny_tn_multi(x, U, gA, 1, K, rank)
            else:
                ops.skinny_tn(x, U[:, :r_pad], gA[0], 1, K, rank)

        def dA_drop():
            if G > 1:
                ops.skinny_tn_drop_multi(x, U, gA, 1, K, rank, streams, drop)
            else:
                ops.skinny_tn_drop(x, U[:, :r_pad], gA[0], 1, K, rank, streams[0], drop)

        def dA_mat():
            for gi in range(G):
                ops.skinny_tn(materialise(gi), U[:, gi * r_pad:(gi + 1) * r_pad], gA[gi], 1, K, rank)

        def dx_drop():
            ops.gemm(dy, wT, out=dx)
            ops.lora_dx_drop(dx, U, A_cat_T, r_pad, streams, drop)

        def dx_mat():
            ops.gemm(dy, wT, out=dx)
            for gi in range(G):
                ops.gemm(U64[gi], A64T[gi], out=tmp)
                tmp.mul_(ops.lora_dropout_mask(M, K, drop, streams[gi]))
                dx.add_(tmp)

        rec = {"measurement": "lora_dropout_kernels", "shape": f"M {M} K {K} G {G} rank {rank} K2 {K2} N {N}", "iters": iters,
               "fwd_ms": {"unmasked_gemm": _median_ms(lambda: ops.gemm(x, A_cat, out=T), iters), "lora_down_drop": _median_ms(lambda: ops.lora_down_drop(x, A_cat, r_pad, streams, drop, out=T), iters),
                          "materialised": _median_ms(fwd_mat, iters)},
               "dA_ms": {"unmasked": _median_ms(dA_plain, iters), "skinny_tn_drop": _median_ms(dA_drop, iters), "materialised": _median_ms(dA_mat, iters)},
               "dx_ms": {"k_extended_gemm": _median_ms(lambda: ops.gemm(dy, wT, out=dx, a2=U, b2=A_cat_T), iters), "gemm_plus_lora_dx_drop": _median_ms(dx_drop, iters),
                         "plain_gemm": _median_ms(lambda: ops.gemm(dy, wT, out=dx), iters), "materialised": _median_ms(dx_mat, iters)}}
        rec = {k: ({a: round(b, 4) for a, b in v.items()} if isinstance(v, dict) else v) for k, v in rec.items()}
        print(json.dumps(rec), flush=True)


def _trainer(p: float, batch: int):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4, lora_dropout=p)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return Trainer(cfg, plugin, acc)


def step(batch: int, steps: int):
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    runs = {p: _trainer(p, batch) for p in (0.0, 0.1)}
    _, devt = PU.make_inputs(batch, 128, 128, 231, 4096, 2048, dev, seed=5)
    b = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    times = {p: [] for p in runs}
    for i in range(2 + steps):
        for p in runs:          # alternating, same process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[p].train_step(dict(b))
            torch.cuda.synchronize()
            if i >= 2:
                times[p].append(time.perf_counter() - t0)
    med = {p: sorted(v)[len(v) // 2] for p, v in times.items()}
    print(json.dumps({"measurement": "sd3_lora_step", "arch": f"SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch {batch}, 4096 + 231 tokens, eager", "steps": steps,
                      "step_ms_p0": round(med[0.0] * 1e3, 2), "step_ms_p0.1": round(med[0.1] * 1e3, 2), "delta_ms": round((med[0.1] - med[0.0]) * 1e3, 2),
                      "spread_ms_p0": round((max(times[0.0]) - min(times[0.0])) * 1e3, 2), "spread_ms_p0.1": round((max(times[0.1]) - min(times[0.1])) * 1e3, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_dropout_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.batch, args.iters)
    if args.part in ("step", "both"):
        step(args.batch, args.steps)


if __name__ == "__main__":
    main()

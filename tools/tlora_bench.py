#!/usr/bin/env python3
"""T-LoRA: the rank-mask kernel at SD3-Medium shapes beside an in-place elementwise kernel over the same operand, and the SD3-Medium T-LoRA step against the same
adapter with the mask launches stubbed out.

    python tools/tlora_bench.py [--part kernels|step|both] [--batch 16] [--step-batch 4] [--steps 6] [--iters 50]

Kernel shapes: the rank-space operands of SD3-Medium's adapted Linears at 1024^2 — M = batch * 4096 image rows, rank 64 (r_pad 64), the q / k / v group (G = 3,
K2 = 192) and a single Linear (G = 1, K2 = 64); timesteps drawn uniformly from [0, 1000), Rmin 1, alpha 1.  Per shape, the median over --iters launches timed
with device events after 3 warm-up launches:
  tlora_mask            ops.tlora_mask in place on T [M, K2]
  scale_cols_in_place   ops.scale_cols(T, gate, 4096, out=T): the project's per-sample in-place bf16 elementwise kernel over the same operand (reads and writes
                        every element) — the yardstick, not a threshold
and the bytes the mask actually writes (every dead column of [0, rank), 2 bytes each, counted on the host from the drawn timesteps) over that time.  Kernel times
proper come from `rocprofv3 --kernel-trace --stats -- python tools/tlora_bench.py --part kernels` in a run of its own (kernel k_tlora_mask).
Step: Attention + FeedForward sites, rank 64, eager; the two variants alternate step by step in one process (the stub swaps `ops.tlora_mask` for the identity).
One JSON line per measurement."""
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
    from simpletuner_amd.engine import TLora
    dev = torch.device("cuda:0")
    rows, rank, r_pad = 4096, 64, 64
    M = batch * rows
    g = torch.Generator(device=dev).manual_seed(1)
    state = TLora(rank, 1, 1.0, 1000, dev)
    ts = torch.rand(batch, generator=g, device=dev) * 1000.0
    ranks = [state.ranks[int(t)] for t in ts.tolist()]
    for G in (3, 1):
        K2 = (G * r_pad + 63) // 64 * 64
        T = torch.randn(M, K2, generator=g, device=dev).to(BF16)
        gate = torch.randn(batch, K2, generator=g, device=dev).to(BF16)
        written = sum(rows * G * (rank - r) * 2 for r in ranks)
        mask_ms = _median_ms(lambda: ops.tlora_mask(T, r_pad, rank, G, rows, state.table, ts), iters)
        yard_ms = _median_ms(lambda: ops.scale_cols(T, gate, rows, out=T), iters)
        print(json.dumps({"measurement": "tlora_mask_kernel", "shape": f"M {M} K2 {K2} G {G} rank {rank} batch {batch}", "iters": iters,
                          "tlora_mask_ms": round(mask_ms, 4), "bytes_written": written, "written_GBps": round(written / (mask_ms * 1e-3) / 1e9, 1),
                          "scale_cols_in_place_ms": round(yard_ms, 4), "scale_cols_bytes_moved": 4 * M * K2,
                          "scale_cols_GBps": round(4 * M * K2 / (yard_ms * 1e-3) / 1e9, 1), "mean_active_rank": round(sum(ranks) / len(ranks), 1)}), flush=True)


def step(batch: int, steps: int):
    from simpletuner_amd import ops
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", lora_rank=64, train_batch_size=batch, seed=5, learning_rate=1e-4)
    cfg.lora_type = "lycoris"
    cfg.lycoris_config = {"algo": "tlora", "multiplier": 1.0, "linear_dim": 64, "linear_alpha": 64, "apply_preset": {"target_module": ["Attention", "FeedForward"]}}
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(batch, 128, 128, 231, 4096, 2048, dev, seed=5)
    b = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    real, calls = ops.tlora_mask, [0]

    def counted(t, *a, **k):
        calls[0] += 1
        return real(t, *a, **k)

    variants = {"masked": counted, "stubbed": lambda t, *a, **k: t}
    times = {k: [] for k in variants}
    try:
        for i in range(2 + steps):
            for name, fn in variants.items():          # alternating, same process
                ops.tlora_mask = fn
                calls[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                trainer.train_step(dict(b))
                torch.cuda.synchronize()
                if i >= 2:
                    times[name].append(time.perf_counter() - t0)
                if name == "masked":
                    per_step = calls[0]
    finally:
        ops.tlora_mask = real
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"measurement": "sd3_tlora_step", "arch": f"SD3-Medium, 24 joint blocks, D 1536, T-LoRA Attention + FeedForward r64, batch {batch}, 4096 + 231 tokens, eager",
                      "steps": steps, "mask_launches_per_step": per_step, "step_ms_masked": round(med["masked"] * 1e3, 2), "step_ms_stubbed": round(med["stubbed"] * 1e3, 2),
                      "delta_ms": round((med["masked"] - med["stubbed"]) * 1e3, 2), "spread_ms_masked": round((max(times["masked"]) - min(times["masked"])) * 1e3, 2),
                      "spread_ms_stubbed": round((max(times["stubbed"]) - min(times["stubbed"])) * 1e3, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--step-batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tlora_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.batch, args.iters)
    if args.part in ("step", "both"):
        step(args.step_batch, args.steps)


if __name__ == "__main__":
    main()

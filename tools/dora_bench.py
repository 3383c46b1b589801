#!/usr/bin/env python3
"""DoRA: the fold kernel and the dm pass at SD3-Medium's adapted Linears, and the SD3-Medium LoRA step with and without `use_dora`.

    python tools/dora_bench.py [--part kernels|step|both] [--batch 4] [--steps 6] [--iters 20] [--out profiles/dora_kernel_stats.md]

Kernels (medians over --iters launches timed with device events after 3 warm-up launches):
  fold   ops.dora_fold at [4608, 1536] (q / k / v, 3 targets) and [1536, 1536] (to_out, 1 target), rank 32 and 128: time, achieved bytes/s over the bytes the kernel
         must move (W read twice, B_blk read twice, A_cat_T once, W' / W'^T / B_blk' / B_blk'^T written), against the time of reading W twice at the streaming rate
         this device reaches on a bf16 copy of the same matrix (read + write counted)
  dmag   ops.dora_dmag over M = batch * 4096 rows at N = 4608 and 1536, and the y0 recompute GEMM in front of it
Step: the eager SD3-Medium LoRA r32 step (synthetic weights), alternating between a trainer without and one with DoRA in one process; the device memory each adapter
adds (torch.cuda.memory_allocated around add_lora_adapter).  One JSON line per measurement; --out also writes them as a markdown list."""
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
RECORDS = []


def emit(rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


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
    dev = torch.device("cuda:0")
    K = 1536
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    for G in (3, 1):
        N = G * K
        W = (rnd(N, K) / K ** 0.5).to(BF16)
        tmp = torch.empty_like(W)
        copy_ms = _median_ms(lambda: tmp.copy_(W), iters)
        stream_rate = 2 * W.numel() * 2 / (copy_ms * 1e-3)          # bytes / s, read + write
        for rank in (32, 128):
            r_pad = 32 if rank <= 32 else (rank + 63) // 64 * 64
            K2 = (G * r_pad + 63) // 64 * 64
            z = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
            A_cat, A_cat_T, B_blk, B_blk_T = z(K2, K), z(K, K2), z(N, K2), z(K2, N)
            for i in range(G):
                ops.lora_pack(rnd(rank, K) / K ** 0.5, 0.02 * rnd(K, rank), 1.0, A_cat, A_cat_T, B_blk, B_blk_T, k2_off=i * r_pad, n_off=i * K)
            m, inv, gg = torch.ones(N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
            Wf, WfT, Bf, BfT = torch.empty_like(W), z(K, N), torch.empty_like(B_blk), z(K2, N)
            targets = [(i * K, K) for i in range(G)]
            ms = _median_ms(lambda: ops.dora_fold(W, A_cat_T, B_blk, m, targets, r_pad, inv, gg, Wf, WfT, Bf, BfT), iters)
            moved = 2 * (4 * N * K + 4 * N * K2 + K * K2)
            emit({"measurement": "dora_fold", "shape": f"W [{N}, {K}] G {G} rank {rank} K2 {K2}", "iters": iters, "fold_ms": round(ms, 4),
                  "bytes_moved": moved, "achieved_GBps": round(moved / (ms * 1e-3) / 1e9, 1), "bf16_copy_of_W_ms": round(copy_ms, 4),
                  "streaming_GBps": round(stream_rate / 1e9, 1), "reading_W_twice_at_streaming_rate_ms": round(2 * W.numel() * 2 / stream_rate * 1e3, 4)})
        M = batch * 4096
        x, dy = rnd(M, K).to(BF16), rnd(M, N).to(BF16)
        T = rnd(M, K2).to(BF16)
        dm = torch.zeros(N, device=dev)
        y0 = ops.dora_y0_scratch(dev, M, N)
        emit({"measurement": "dora_dmag", "shape": f"M {M} N {N} K {K} K2 {K2}", "iters": iters,
              "y0_recompute_gemm_ms": round(_median_ms(lambda: ops.gemm(x, W, a2=T, b2=B_blk, out=y0), iters), 4),
              "dmag_ms": round(_median_ms(lambda: ops.dora_dmag(dy, y0, inv, dm, accumulate=True), iters), 4), "dmag_bytes": 4 * M * N})


def _trainer(dora: bool, batch: int):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4)
    cfg.use_dora = dora
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.get_trained_component().init_synthetic(3)          # (DoRA divides by the row norm of W + s B A: the weights must not be the arena's zeros)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    plugin.add_lora_adapter()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated() - before
    plugin.post_model_load_setup()
    return Trainer(cfg, plugin, acc), mem


def step(batch: int, steps: int):
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    runs, mem = {}, {}
    for d in (False, True):
        runs[d], mem[d] = _trainer(d, batch)
    _, devt = PU.make_inputs(batch, 128, 128, 231, 4096, 2048, dev, seed=5)
    b = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    times = {d: [] for d in runs}
    for i in range(2 + steps):
        for d in runs:          # alternating, same process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[d].train_step(dict(b))
            torch.cuda.synchronize()
            if i >= 2:
                times[d].append(time.perf_counter() - t0)
    med = {d: sorted(v)[len(v) // 2] for d, v in times.items()}
    emit({"measurement": "sd3_lora_step", "arch": f"SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch {batch}, 4096 + 231 tokens, eager, synthetic weights", "steps": steps,
          "step_ms_lora": round(med[False] * 1e3, 2), "step_ms_dora": round(med[True] * 1e3, 2), "delta_ms": round((med[True] - med[False]) * 1e3, 2),
          "spread_ms_lora": round((max(times[False]) - min(times[False])) * 1e3, 2), "spread_ms_dora": round((max(times[True]) - min(times[True])) * 1e3, 2),
          "adapter_bytes_lora": mem[False], "adapter_bytes_dora": mem[True], "extra_device_bytes_dora": mem[True] - mem[False]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dora_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.batch, args.iters)
    if args.part in ("step", "both"):
        step(args.batch, args.steps)
    if args.out:
        lines = ["# DoRA kernel and step measurements (tools/dora_bench.py, one MI355X)", "",
                 f"`python tools/dora_bench.py --part {args.part} --batch {args.batch} --steps {args.steps} --iters {args.iters}`", ""]
        for rec in RECORDS:
            lines.append(f"- **{rec['measurement']}** " + ", ".join(f"{k}: {v}" for k, v in rec.items() if k != "measurement"))
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

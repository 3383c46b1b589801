#!/usr/bin/env python3
"""Scheduled sampling with ReflexFlow: the loss kernels at the 1024^2 latent shape of BASELINE.json's Flux and SD3 configs, and the SD3-Medium LoRA step with a rollout.

    python tools/reflexflow_bench.py [--part kernels|step|both] [--batch 4] [--steps 6] [--iters 20] [--out profiles/reflexflow_kernel_stats.md]

Kernels (medians over --iters launches timed with device events after 3 warm-up launches), at latents [B, 16, 128, 128] (Flux.1-dev and SD3-Medium at 1024^2 share
the shape), B = --batch and 8, in one run:
  fused   ops.reflexflow_stats + ops.reflexflow_loss (l2, cached predictions, defaults alpha 1 / beta1 10 / beta2 1, gradient written)
  cond    ops.cond_loss on the same shape: it reads a third of the operands, a lower bound, not a target
  eager   the same expression composed from torch operations on the device in bf16, with autograd for d(loss)/d(pred): what would ship without the kernels
each as time and as GB/s over the bytes it must move (fused: stats 5 reads + loss 6 reads + 1 write = 12 x 2 B per element; cond: 2 reads + 1 write; eager: the same
12 x 2 B as a floor — it moves far more).
Step: the eager SD3-Medium LoRA r32 step (synthetic weights) alternating between a plain trainer and one with scheduled_sampling_max_step_offset = 4, probability 1
and an injected plan of offset 4 for every sample, in one process; the added cost itemised: number of batch-1 forwards, the time of the rollout, the loss kernels.
One JSON line per measurement; --out also writes them as a markdown list."""
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


def eager_loss(pred, target, noisy, latents, clean, biased, alpha=1.0, beta1=10.0, beta2=1.0):
    """the expression of the loss in torch operations on bf16 device tensors (float casts where the reference casts)"""
    p = pred.detach().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(p.float(), target.float(), reduction="none")
    e = (clean - biased).detach()
    loss = loss * (1.0 + alpha * e / e.abs().sum(dim=(1, 2, 3), keepdim=True).clamp_min(1e-6))
    if beta2 != 1.0:
        loss = loss * beta2
    tv = (noisy - latents).reshape(p.shape[0], -1)
    fp = p.reshape(p.shape[0], -1)
    adr = (fp / torch.norm(fp, dim=1, keepdim=True).clamp_min(1e-6) - tv / torch.norm(tv, dim=1, keepdim=True).clamp_min(1e-6)).pow(2).sum(dim=1)
    total = (loss.mean(dim=(1, 2, 3)) + beta1 * adr.float()).mean()
    total.backward()
    return total, p.grad


def kernels(batch: int, iters: int):
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    for B in sorted({batch, 8}):
        shape = (B, 16, 128, 128)
        n = B * 16 * 128 * 128
        pred, target, noisy, latents, clean, biased = (torch.randn(*shape, generator=g, device=dev).to(BF16) for _ in range(6))
        tmp = torch.empty_like(pred)
        copy_ms = _median_ms(lambda: tmp.copy_(pred), iters)

        def fused():
            st = ops.reflexflow_stats(pred, noisy, latents, clean, biased)
            return ops.reflexflow_loss(pred, target, noisy, latents, st, "l2", clean=clean, biased=biased)
        stats_ms = _median_ms(lambda: ops.reflexflow_stats(pred, noisy, latents, clean, biased), iters)
        fused_ms = _median_ms(fused, iters)
        cond_ms = _median_ms(lambda: ops.cond_loss(pred, target, "l2"), iters)
        eager_ms = _median_ms(lambda: eager_loss(pred, target, noisy, latents, clean, biased), iters)
        f_loss = fused()[0].item()
        e_loss = eager_loss(pred, target, noisy, latents, clean, biased)[0].item()
        gbps = lambda elems_x2, ms: round(elems_x2 * 2 * n / (ms * 1e-3) / 1e9, 1)
        emit({"measurement": "reflexflow_loss_kernels", "shape": list(shape), "iters": iters, "stats_ms": round(stats_ms, 4), "stats_plus_loss_ms": round(fused_ms, 4),
              "fused_bytes": 24 * n, "fused_GBps": gbps(12, fused_ms), "cond_loss_ms": round(cond_ms, 4), "cond_loss_bytes": 6 * n, "cond_loss_GBps": gbps(3, cond_ms),
              "torch_eager_bf16_ms": round(eager_ms, 4), "torch_eager_GBps_over_the_fused_bytes": gbps(12, eager_ms), "eager_over_fused": round(eager_ms / fused_ms, 2),
              "bf16_copy_ms": round(copy_ms, 4), "bf16_copy_GBps": gbps(2, copy_ms), "loss_fused": round(f_loss, 5), "loss_eager": round(e_loss, 5)})


def _trainer(offset: int, batch: int):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    extra = dict(scheduled_sampling_max_step_offset=offset, scheduled_sampling_probability=1.0) if offset else {}
    cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4, **extra)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return Trainer(cfg, plugin, acc)


def step(batch: int, steps: int, offset: int = 4):
    from simpletuner_amd.scheduled_sampling import ScheduledSamplingPlan
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    runs = {0: _trainer(0, batch), offset: _trainer(offset, batch)}
    _, devt = PU.make_inputs(batch, 128, 128, 231, 4096, 2048, dev, seed=5)
    sig = devt["sigmas"]
    for tr in runs.values():
        tr.model.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    base = (sig * 1000.0).long()
    off = torch.full_like(base, offset)
    b = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    roll = runs[offset].model
    stamp = {"forwards": 0, "rollout_s": []}
    predict, apply = roll.model_predict, roll.apply_scheduled_sampling_rollout

    def counted(pb):
        stamp["forwards"] += int(pb["noisy_latents"].shape[0] == 1 and not torch.is_grad_enabled())
        return predict(pb)

    def timed(pb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = apply(pb)
        torch.cuda.synchronize()
        stamp["rollout_s"].append(time.perf_counter() - t0)
        return out
    roll.model_predict, roll.apply_scheduled_sampling_rollout = counted, timed
    times = {d: [] for d in runs}
    for i in range(2 + steps):
        for d, tr in runs.items():          # alternating, same process
            bb = dict(b)
            if d:
                bb["scheduled_sampling_plan"] = ScheduledSamplingPlan(target_timesteps=base, source_timesteps=torch.clamp(base + off, max=999), rollout_steps=off)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_step(bb)
            torch.cuda.synchronize()
            if i >= 2:
                times[d].append(time.perf_counter() - t0)
    med = {d: sorted(v)[len(v) // 2] for d, v in times.items()}
    rs = sorted(stamp["rollout_s"][2:])
    emit({"measurement": "sd3_lora_step_with_rollout", "arch": f"SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch {batch}, 4096 + 231 tokens, eager, synthetic weights",
          "steps": steps, "max_step_offset": offset, "probability": 1.0, "step_ms_plain": round(med[0] * 1e3, 2), "step_ms_rollout": round(med[offset] * 1e3, 2),
          "delta_ms": round((med[offset] - med[0]) * 1e3, 2), "batch1_forwards_per_step": stamp["forwards"] // (2 + steps),
          "rollout_ms_per_step": round(rs[len(rs) // 2] * 1e3, 2), "rollout_ms_per_forward": round(rs[len(rs) // 2] * 1e3 / max(stamp["forwards"] // (2 + steps), 1), 2),
          "spread_ms_plain": round((max(times[0]) - min(times[0])) * 1e3, 2), "spread_ms_rollout": round((max(times[offset]) - min(times[offset])) * 1e3, 2),
          "logs": runs[offset].last_aux_logs})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reflexflow_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.batch, args.iters)
    if args.part in ("step", "both"):
        step(args.batch, args.steps)
    if args.out:
        lines = ["# ReflexFlow kernel and step measurements (tools/reflexflow_bench.py, one MI355X)", "",
                 f"`python tools/reflexflow_bench.py --part {args.part} --batch {args.batch} --steps {args.steps} --iters {args.iters}`", ""]
        for rec in RECORDS:
            lines.append(f"- **{rec['measurement']}** " + ", ".join(f"{k}: {v}" for k, v in rec.items() if k != "measurement"))
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

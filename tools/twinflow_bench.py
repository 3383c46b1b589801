#!/usr/bin/env python3
"""TwinFlow at SD3-Medium shapes on the MI355X: the three kernels against a bf16 copy of the bytes they must move and against the torch-eager composition they
replace, and the step of SD3-Medium LoRA r32 with the flag on (order 2, ratio 0 and 0.5) beside the flag-off step.

    python tools/twinflow_bench.py [--steps 4] [--batch 4] [--only kernels|step]

One JSON line per measurement, device events around windows that end in a synchronise.  Kernels: REPS launches per window (a single launch is a few microseconds:
one window then measures the launch path REPS times, which is what the step pays too), medians over the windows behind warm-up windows, the compared things
alternating.  Algorithmic bytes (bf16 2, fp32 4) per element: rcgm_step 2 + 2 + 2 (x in / out, fc) + 4 (acc out) [+ 4 acc in unless first]; loss 2 + 2 + 4 (pred,
target, acc) [+ 4 cond / uncond] + 2 (dpred); ucgm_step 2 + 2 + 2 [+ 2 noise].  The copy moves the same number of bytes (half read, half written).
  step      Trainer.train_step through the SD3 plugin (24 joint blocks, D 1536, LoRA r32, latents [B, 16, 128, 128], 154 text tokens), EMA on in all three runs."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARCH = dict(num_layers=24, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536, pooled_projection_dim=2048,
            pos_embed_max_size=192, sample_size=128)
BF16, F32 = torch.bfloat16, torch.float32
REPS = 50


def timed(fns: dict, steps: int, warm: int = 2, reps: int = 1):
    """{name: callable} run alternately; -> {name: (median ms per call, spread ms)} from device events"""
    times = {k: [] for k in fns}
    for i in range(warm + steps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times[k].append(a.elapsed_time(b) / reps)
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in times.items()}


def bench_kernels(dev, B: int, steps: int):
    from simpletuner_amd import ops
    shape = (B, 16, 128, 128)
    n = B * 16 * 128 * 128
    g = torch.Generator(device=dev).manual_seed(1)
    rb = lambda: torch.randn(shape, generator=g, device=dev).to(BF16)
    x, fc, pred, target, cond, uncond, noise = (rb() for _ in range(7))
    acc = torch.randn(shape, generator=g, device=dev)
    tp, tn = torch.rand(B, generator=g, device=dev) * 0.5 + 0.5, torch.rand(B, generator=g, device=dev) * 0.5
    h4 = (tn - tp).view(B, 1, 1, 1)

    def copy_of(nbytes):
        src = torch.empty(nbytes // 4, dtype=BF16, device=dev).normal_()          # nbytes / 2 read + nbytes / 2 written
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    def eager_rcgm():
        f = fc.float()
        acc.add_(f * -h4)
        x.copy_((x.float() + h4 * f).to(BF16))

    def eager_loss(pair):
        t = target.float() + (0.5 * (cond.float() - uncond.float()) if pair else 0.0)
        p = pred.float()
        d = p - t
        rc = (d - acc).clamp(-1.0, 1.0)
        return torch.stack([(rc * rc).mean(), (d * d).mean()]), ((2.0 / n) * (rc + d)).to(BF16)

    def eager_ucgm():
        xs, f = x.float(), fc.float()
        x.copy_(((1 - 0.25) * (xs - 0.6 * f) + 0.25 * ((xs + 0.4 * f) * 0.0 + noise.float() * 1.0)).to(BF16))

    cases = {
        "rcgm_step_first": (lambda: ops.twinflow_rcgm_step(x, acc, fc, tp, tn, True), 10 * n, eager_rcgm),
        "rcgm_step": (lambda: ops.twinflow_rcgm_step(x, acc, fc, tp, tn, False), 14 * n, eager_rcgm),
        "loss": (lambda: ops.twinflow_loss(pred, target, acc, None, None, 0.0, 1.0), 10 * n, lambda: eager_loss(False)),
        "loss_cfg": (lambda: ops.twinflow_loss(pred, target, acc, cond, uncond, 0.5, 1.0), 14 * n, lambda: eager_loss(True)),
        "ucgm_step": (lambda: ops.twinflow_ucgm_step(x, fc, 0.6, 0.25, 1.0, noise), 8 * n, eager_ucgm),
    }
    for name, (kernel, nbytes, eager) in cases.items():
        r = timed({"kernel": kernel, "copy": copy_of(nbytes), "eager": eager}, max(steps, 10), warm=3, reps=REPS)
        print(json.dumps({"measurement": f"twinflow_{name}", "shape": list(shape), "kernel_us": round(r["kernel"][0] * 1e3, 2), "kernel_spread_us": round(r["kernel"][1] * 1e3, 2),
                          "copy_same_bytes_us": round(r["copy"][0] * 1e3, 2), "copy_spread_us": round(r["copy"][1] * 1e3, 2), "torch_eager_us": round(r["eager"][0] * 1e3, 2),
                          "eager_spread_us": round(r["eager"][1] * 1e3, 2), "algorithmic_bytes": nbytes, "kernel_TBps": round(nbytes / (r["kernel"][0] * 1e-3) / 1e12, 3),
                          "launches_per_window": REPS}), flush=True)


def build_trainer(dev, B: int, **flags):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    cfg = default_config(model_family="sd3", train_batch_size=B, seed=5, lora_rank=32, lora_init_b_std=0.02, learning_rate=1e-4, use_ema=True, **flags)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(B, 128, 128, 154, 4096, 2048, dev, seed=5)
    g = torch.Generator().manual_seed(9)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"],
             "negative_prompt_embeds": torch.randn(devt["prompt"].shape, generator=g).to(BF16).to(dev)}
    return trainer, batch


def bench_step(dev, B: int, steps: int):
    runs = {"flag_off": {}, "order2_ratio0": dict(twinflow_enabled=True, twinflow_estimate_order=2, twinflow_enhanced_ratio=0.0),
            "order2_ratio0.5": dict(twinflow_enabled=True, twinflow_estimate_order=2, twinflow_enhanced_ratio=0.5)}
    out = {}
    for name, flags in runs.items():          # one model at a time on the device
        trainer, batch = build_trainer(dev, B, **flags)
        r = timed({name: lambda: trainer.train_step(dict(batch))}, steps)
        out[name] = r[name]
        del trainer, batch
        torch.cuda.empty_cache()
    base = out["flag_off"][0]
    print(json.dumps({"measurement": "sd3_medium_lora_r32_train_step", "batch": B, "latents": [B, 16, 128, 128],
                      **{f"{k}_ms": round(v[0], 2) for k, v in out.items()}, **{f"{k}_spread_ms": round(v[1], 2) for k, v in out.items()},
                      **{f"{k}_over_flag_off": round(v[0] / base, 3) for k, v in out.items() if k != "flag_off"}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--only", choices=("kernels", "step"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("twinflow_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    dev = torch.device("cuda:0")
    if args.only in (None, "kernels"):
        for B in (4, 8):
            bench_kernels(dev, B, args.steps)
    if args.only in (None, "step"):
        bench_step(dev, args.batch, args.steps)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""SD3-Medium-shaped LoRA train steps with NextLat on or off, for a kernel-trace pass and for the step-time delta.

    python tools/nextlat_bench.py --nextlat on|off|both [--steps 6] [--batch 4]
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/nextlat_bench.py --nextlat on --steps 3        (no counters in the same run)

SD3-Medium: 24 joint blocks, D 1536, LoRA r32, 1024^2 (4096 image + 231 text tokens), AdamW, eager, through the plugin and the trainer.  `both` alternates the two
configurations in one process and reports the medians and the spread of the off runs.  One JSON line per result.  With NextLat on, M = batch * 4095 predictor rows:
the streaming kernels' algorithmic bytes are printed with it (bf16 2 bytes, fp32 parameters 4): gelu_fwd 8 M D, gelu_bwd 12 M D, loss 6 M D, ln_bwd_add 8 M D,
fold 32 D^2 (two fp32 matrices of 2 D^2 elements in, each as two bf16 images out), wgrad_up 20 D^2, wgrad_down 12 D^2."""
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


def _trainer(on: bool, batch: int):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4, nextlat_enabled=on, nextlat_weight=0.1 if on else None)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return Trainer(cfg, plugin, acc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nextlat", choices=("on", "off", "both"), default="both")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nextlat_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    modes = {"on": (True,), "off": (False,), "both": (False, True)}[args.nextlat]
    runs = {on: _trainer(on, args.batch) for on in modes}
    _, devt = PU.make_inputs(args.batch, 128, 128, 231, 4096, 2048, dev, seed=5)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    times = {on: [] for on in modes}
    for i in range(2 + args.steps):
        for on in modes:          # alternating, same process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[on].train_step(dict(batch))
            torch.cuda.synchronize()
            if i >= 2:
                times[on].append(time.perf_counter() - t0)
    med = {on: sorted(v)[len(v) // 2] for on, v in times.items()}
    M, D = args.batch * 4095, 1536
    rec = {"measurement": "sd3_lora_step", "arch": f"SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch {args.batch}, 4096 + 231 tokens, eager", "steps": args.steps,
           **{f"step_ms_nextlat_{'on' if on else 'off'}": round(med[on] * 1e3, 2) for on in modes},
           **{f"spread_ms_{'on' if on else 'off'}": round((max(times[on]) - min(times[on])) * 1e3, 3) for on in modes}}
    if len(modes) == 2:
        rec["delta_ms"] = round((med[True] - med[False]) * 1e3, 3)
    if True in modes:
        rec["algorithmic_bytes"] = {"gelu_fwd": 8 * M * D, "gelu_bwd": 12 * M * D, "loss": 6 * M * D, "ln_bwd_add": 8 * M * D, "fold": 32 * D * D, "wgrad_up": 20 * D * D, "wgrad_down": 12 * D * D}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

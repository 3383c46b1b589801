#!/usr/bin/env python3
"""Time the two LayerSync entry points (st355_layersync_fwd, st355_layersync_inject) on one MI355X at the shapes the trained models give them.

    python tools/layersync_bench.py [--iters 200] [--step-time] [--steps 6]

One JSON line per measurement.  Shapes: Flux.1 at batch 8 (rows = 4096 image tokens of a 4608-row joint [txt || img] sequence, D = 3072: the teacher / the
gradient are strided views starting 512 rows into each sample) and SD3-Medium at batch 8 (4096 compact image-stream rows, D = 1536).  Times are device events
around `iters` back-to-back calls after a warm-up; bytes are the algorithm's (forward: read student + teacher, write G = 3 * B * rows * D bf16, plus the
cosines; inject: read dx + G, write dx), the rate is bytes / time against the 8 TB/s HBM3E peak DESIGN.md §5 uses.  Both kernels are bandwidth-bound.
--step-time also measures a Flux LoRA train step (reduced depth, full width: 2 double + 4 single blocks, batch 2, 1024^2) through the plugin and the trainer with
LayerSync off and on, alternating, on the same process."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_PEAK = 8.0e12
SHAPES = {"flux_b8": dict(B=8, rows=4096, St=512, D=3072), "sd3_b8": dict(B=8, rows=4096, St=0, D=1536)}


def _time(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e-3


def kernels(iters):
    from simpletuner_amd import ops
    from simpletuner_amd.engine import rows_of
    dev = torch.device("cuda:0")
    for name, sh in SHAPES.items():
        B, rows, St, D = sh["B"], sh["rows"], sh["St"], sh["D"]
        S = St + rows
        g = torch.Generator(device=dev).manual_seed(1)
        joint_t = torch.randn(B * S, D, generator=g, device=dev, dtype=torch.bfloat16)
        joint_dx = torch.randn(B * S, D, generator=g, device=dev, dtype=torch.bfloat16)
        student = torch.randn(B * rows, D, generator=g, device=dev, dtype=torch.bfloat16)
        G = torch.empty_like(student)
        cos, sim = torch.empty(B * rows, dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.zeros((), dtype=torch.float32, device=dev)          # (scale 0: dx keeps its values over the iterations; the pass is the same)
        t_view, dx_view, s_view = rows_of(joint_t, St, rows, B, S), rows_of(joint_dx, St, rows, B, S), student.view(B, rows, D)
        n = B * rows * D
        t_f = _time(lambda: ops.layersync_fwd(s_view, t_view, G, cos, sim), iters)
        t_i = _time(lambda: ops.layersync_inject(dx_view, G, scale), iters)
        for what, t, nbytes in (("layersync_fwd", t_f, 3 * 2 * n + 4 * B * rows), ("layersync_inject", t_i, 3 * 2 * n)):
            print(json.dumps({"kernel": what, "shape": name, **sh, "time_us": round(t * 1e6, 2), "bytes": nbytes, "GBps": round(nbytes / t / 1e9, 1),
                              "share_of_hbm_peak": round(nbytes / t / HBM_PEAK, 3), "bound": "HBM"}))


def step_time(steps):
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    arch = dict(num_layers=2, num_single_layers=4, num_attention_heads=24, attention_head_dim=128, joint_attention_dim=4096, pooled_projection_dim=768, guidance_embeds=True,
                in_channels=64)
    runs = {}
    for on in (False, True):
        cfg = default_config(lora_rank=16, train_batch_size=2, seed=5, learning_rate=1e-4, layersync_enabled=on, layersync_student_block=2, layersync_teacher_block=5)
        acc = St355Accelerator(dev)
        plugin = Flux(cfg, acc)
        plugin.load_model(**arch)
        plugin.add_lora_adapter()
        plugin.post_model_load_setup()
        runs[on] = (plugin, Trainer(cfg, plugin, acc))
    _, devt = PU.make_inputs(2, 128, 128, 512, 4096, 768, dev, seed=5)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    times = {False: [], True: []}
    for i in range(2 + steps):
        for on in (False, True):          # alternating, same process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[on][1].train_step(dict(batch))
            torch.cuda.synchronize()
            if i >= 2:
                times[on].append(time.perf_counter() - t0)
    med = {on: sorted(v)[len(v) // 2] for on, v in times.items()}
    print(json.dumps({"measurement": "flux_lora_step_reduced_depth", "arch": "2 double + 4 single blocks, D 3072, batch 2, 4096 + 512 tokens", "steps": steps,
                      "step_ms_layersync_off": round(med[False] * 1e3, 2), "step_ms_layersync_on": round(med[True] * 1e3, 2),
                      "delta_ms": round((med[True] - med[False]) * 1e3, 3), "spread_ms_off": round((max(times[False]) - min(times[False])) * 1e3, 3),
                      "note": "layersync on includes the two host reads of auxiliary_loss's logs"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-time", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("layersync_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    kernels(args.iters)
    if args.step_time:
        step_time(args.steps)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The evaluation loss on the MI355X: the two kernels of csrc/eval_loss.hip at training shapes, and the wall time of one eval pass (eval_timesteps 28, 4 eval
batches) for SD3-Medium LoRA r128 batch 3 and Flux.1-dev LoRA r32 batch 8 over eval_timestep_stack in {1, 2, 4, 7, 14, 28}, beside the training step of the same
configuration.

    python tools/eval_loss_bench.py --only kernels
    python tools/eval_loss_bench.py --only pass --family sd3 [--stacks 1,2,4,7,14,28] [--repeats 3]
    python tools/eval_loss_bench.py --only pass --family sd3 --baseline          # runs on a tree without the feature, too

One JSON line per measurement.  Kernels: device events around windows of REPS launches that end in a synchronise (a single launch is a few microseconds: a
window measures the call as the pass pays it), medians over the windows behind warm-up windows, beside a bf16 copy of the same number of bytes.  Algorithmic bytes
per element of [B, n]: views 2 + 2 read, 2 K written; loss 2 K (pred) + 2 (target: one slab, whatever K) read.
Pass: a host clock around `Trainer.evaluate()`, which ends in the pass's one host read; the stack sizes alternate inside every repeat, so the spread of one size
is the run-to-run spread under the same neighbours.  A size whose forward does not fit is reported as skipped with the allocator's message.
`--baseline`: the same pass with only the ops a tree without the feature has — per timestep ops.flow_noise_mix (all rows at the timestep's sigma), model_predict
under no_grad, ops.mse_loss(want_grad=False) — the losses kept on the device and read once: the comparison is against that tree, not against the code under test."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BF16, F32 = torch.bfloat16, torch.float32
REPS = 50
SD3_ARCH = dict(sample_size=128, num_layers=24, num_attention_heads=24, attention_head_dim=64, caption_projection_dim=1536, pooled_projection_dim=2048,
                pos_embed_max_size=192)
CONFIGS = {"sd3": dict(rank=128, batch=3, S_txt=154, txt_dim=4096, pooled=2048, what="SD3-Medium LoRA r128 batch 3, latents [3, 16, 128, 128], 154 text tokens"),
           "flux": dict(rank=32, batch=8, S_txt=512, txt_dim=4096, pooled=768, what="Flux.1-dev LoRA r32 batch 8, latents [8, 16, 128, 128], 512 text tokens")}
T, EVAL_BATCHES = 28, 4


def timed(fns: dict, steps: int, warm: int = 3, reps: int = 1):
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


def bench_kernels(dev, steps: int):
    from simpletuner_amd import ops
    for B in (3, 4, 8):
        for K in (1, 7):
            shape = (B, 16, 128, 128)
            n = B * 16 * 128 * 128
            g = torch.Generator(device=dev).manual_seed(1)
            lat, noise, target = (torch.randn(shape, generator=g, device=dev).to(BF16) for _ in range(3))
            pred = torch.randn((K,) + shape, generator=g, device=dev).to(BF16)
            sig = torch.rand(K, generator=g, device=dev)
            out = torch.empty((K,) + shape, dtype=BF16, device=dev)
            table = torch.zeros(4, 28, device=dev)
            c = torch.full((K * B,), 0.1, device=dev)

            def copy_of(nbytes):
                src = torch.empty(nbytes // 4, dtype=BF16, device=dev).normal_()          # nbytes / 2 read + nbytes / 2 written
                dst = torch.empty_like(src)
                return lambda: dst.copy_(src)

            cases = {"views": (lambda: ops.eval_flow_views(lat, noise, sig, out=out), (4 + 2 * K) * n),
                     "loss_l2": (lambda: ops.eval_loss(pred, target, "l2", loss_out=table[1, :K]), (2 * K + 2) * n),
                     "loss_huber": (lambda: ops.eval_loss(pred, target, "huber", c, loss_out=table[1, :K]), (2 * K + 2) * n)}
            for name, (kernel, nbytes) in cases.items():
                r = timed({"kernel": kernel, "copy": copy_of(nbytes)}, max(steps, 10), reps=REPS)
                print(json.dumps({"measurement": f"eval_{name}", "latents": list(shape), "K": K, "call_us": round(r["kernel"][0] * 1e3, 2),
                                  "call_spread_us": round(r["kernel"][1] * 1e3, 2), "copy_same_bytes_us": round(r["copy"][0] * 1e3, 2),
                                  "copy_spread_us": round(r["copy"][1] * 1e3, 2), "algorithmic_bytes": nbytes,
                                  "call_TBps": round(nbytes / (r["kernel"][0] * 1e-3) / 1e12, 3), "launches_per_window": REPS}), flush=True)


def build(dev, family: str, eval_sets=None, **flags):
    """(plugin, trainer or None, training batch, eval batches)"""
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    c = CONFIGS[family]
    B = c["batch"]
    cfg = default_config(model_family=family, train_batch_size=B, seed=42, lora_rank=c["rank"], lora_init_b_std=1e-3, learning_rate=1e-4, **flags)
    acc = St355Accelerator(dev)
    if family == "flux":
        from simpletuner_amd.flux.model import Flux
        plugin = Flux(cfg, acc)
        plugin.load_model(num_layers=19, num_single_layers=38, guidance_embeds=True)
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, acc)
        plugin.load_model(**SD3_ARCH)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    gen = torch.Generator(device=dev).manual_seed(42)

    def make_batch():
        return {"latent_batch": torch.randn(B, 16, 128, 128, device=dev, generator=gen).to(BF16),
                "prompt_embeds": torch.randn(B, c["S_txt"], c["txt_dim"], device=dev, generator=gen).to(BF16),
                "add_text_embeds": torch.randn(B, c["pooled"], device=dev, generator=gen).to(BF16)}
    train_batch = make_batch()
    evals = [make_batch() for _ in range(EVAL_BATCHES)]
    trainer = None
    if eval_sets is not False:
        trainer = Trainer(cfg, plugin, acc, **({"eval_sets": {"val": evals}} if eval_sets else {}))
    return plugin, trainer, train_batch, evals


def grid_of(plugin):
    """the 28-step grid of the training schedule and its dtype chain (grid value -> bf16 -> sigma = bf16(t / 1000) -> model timestep = bf16(sigma 1000))"""
    import copy
    if plugin.noise_schedule is None:
        plugin.setup_training_noise_schedule()
    sched = copy.copy(plugin.noise_schedule)
    sched.set_timesteps(T)
    t = sched.timesteps.to(BF16)
    sigma = (t / 1000.0).clamp(0.0, 1.0)
    return sigma.float(), (sigma * 1000.0).float()


def baseline_pass(plugin, evals, dev):
    from simpletuner_amd import ops
    sigma, ts = grid_of(plugin)
    sigma, ts = sigma.to(dev), ts.to(dev)
    table = torch.zeros(len(evals), T, device=dev)
    with torch.no_grad():
        for row, raw in enumerate(evals):
            prepared = plugin.prepare_batch(dict(raw), {"global_step": 0})
            lat, noise, target = prepared["latents"], prepared["input_noise"], prepared["flow_target"]
            B = lat.shape[0]
            for j in range(T):
                batch = dict(prepared)
                batch["noisy_latents"] = ops.flow_noise_mix(lat, sigma[j].expand(B).contiguous(), noise=noise, want_target=False)[0]
                batch["timesteps"] = ts[j].expand(B)
                pred = plugin.model_predict(batch)["model_prediction"]
                table[row, j:j + 1].copy_(ops.mse_loss(pred, target, want_grad=False)[0])
    return table.cpu()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_pass(dev, family: str, stacks, repeats: int, baseline: bool, train_steps: int):
    what = CONFIGS[family]["what"]
    if baseline:
        plugin, _, _, evals = build(dev, family, eval_sets=False)
        baseline_pass(plugin, evals[:1], dev)          # warm-up
        times, means = [], []
        for _ in range(repeats):
            ms, table = wall(lambda: baseline_pass(plugin, evals, dev))
            times.append(ms)
            means.append(float(table.mean()))
            print(f"[eval_loss_bench] {family} baseline ops: {ms:.1f} ms", file=sys.stderr, flush=True)
        print(json.dumps({"measurement": "eval_pass_baseline_ops", "config": what, "eval_timesteps": T, "eval_batches": EVAL_BATCHES, "pass_ms": [round(t, 1) for t in times],
                          "median_ms": round(sorted(times)[len(times) // 2], 1), "spread_ms": round(max(times) - min(times), 1), "mean_loss": means[0]}), flush=True)
        return
    plugin, trainer, train_batch, evals = build(dev, family, eval_sets=True, eval_steps_interval=1, eval_timesteps=T)
    r = timed({"train_step": lambda: trainer.train_step(dict(train_batch))}, train_steps, warm=2)
    step_ms = r["train_step"][0]
    print(json.dumps({"measurement": "train_step_eager", "config": what, "median_ms": round(step_ms, 2), "spread_ms": round(r["train_step"][1], 2)}), flush=True)
    trainer.optimizer.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()
    times, means, skipped = {k: [] for k in stacks}, {}, {}
    for rep in range(repeats + 1):          # the first round is the warm-up of every size (one eval batch: every shape of the pass is launched once)
        plugin.config.num_eval_images = None if rep else 1
        for k in stacks:
            if k in skipped:
                continue
            plugin.config.eval_timestep_stack = k
            try:
                ms, logs = wall(trainer.evaluate)
            except torch.OutOfMemoryError as e:
                skipped[k] = str(e).split("\n")[0][:160]
                torch.cuda.empty_cache()
                continue
            if rep:
                times[k].append(ms)
            means[k] = logs["loss/val/val"]
            print(f"[eval_loss_bench] {family} round {rep} stack {k}: {ms:.1f} ms", file=sys.stderr, flush=True)
    for k in stacks:
        if k in skipped:
            print(json.dumps({"measurement": "eval_pass", "config": what, "eval_timestep_stack": k, "skipped": skipped[k]}), flush=True)
            continue
        v = times[k]
        med = sorted(v)[len(v) // 2]
        print(json.dumps({"measurement": "eval_pass", "config": what, "eval_timesteps": T, "eval_batches": EVAL_BATCHES, "eval_timestep_stack": k,
                          "pass_ms": [round(t, 1) for t in v], "median_ms": round(med, 1), "spread_ms": round(max(v) - min(v), 1),
                          "over_train_step": round(med / step_ms, 2), "mean_loss": means[k], "peak_hbm_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernels", "pass"), default=None)
    ap.add_argument("--family", choices=("sd3", "flux", "both"), default="both")
    ap.add_argument("--stacks", default="1,2,4,7,14,28")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="timed windows of the kernel measurement")
    ap.add_argument("--train-steps", type=int, default=4)
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_loss_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    dev = torch.device("cuda:0")
    if args.only in (None, "kernels") and not args.baseline:
        bench_kernels(dev, args.steps)
    if args.only in (None, "pass"):
        for family in (("sd3", "flux") if args.family == "both" else (args.family,)):
            bench_pass(dev, family, [int(s) for s in args.stacks.split(",")], args.repeats, args.baseline, args.train_steps)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

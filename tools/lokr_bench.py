#!/usr/bin/env python3
"""LoKr: the fold, mix, dw2, P and dw1 launches at SD3-Medium's adapted Linears under the documented LyCORIS config (factor 10 on Attention: 8 x 192, factor 4 on
FeedForward: 4 x 384 / 4 x 1536), and the SD3-Medium step with LoKr beside the plain LoRA r32 step.

    python tools/lokr_bench.py [--part kernels|step|both] [--batch 4] [--steps 6] [--iters 20] [--out profiles/lokr_kernel_stats.md]

Kernels (medians over --iters launches timed with device events after 3 warm-up launches), M = batch * 4096 rows:
  fold   ops.lokr_fold of one fused projection: bytes the kernel must move = W read, Wf and WfT written (+ the factors), achieved bytes / s
  mix    ops.lokr_mix: dy slab read, dP written
  dw2    ops.lokr_dw2: dP and x read once per output tile row / column; FLOPs 2 M im ok in
  P      ops.gemm(x.view(M im, in), w2b): FLOPs 2 M im ok in
  dw1    ops.lokr_dw1: dy slab and P read; FLOPs 2 M ol im ok
Step: the eager SD3-Medium step (synthetic weights), alternating between a trainer with LoRA r32 and one with LoKr in one process; the device memory each adapter
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
LYCORIS = {"algo": "lokr", "multiplier": 1.0, "linear_dim": 10000, "linear_alpha": 1, "factor": 10,
           "apply_preset": {"target_module": ["Attention", "FeedForward"], "module_algo_map": {"Attention": {"factor": 10}, "FeedForward": {"factor": 4}}}}
BF16, F32 = torch.bfloat16, torch.float32
RECORDS = []
# (site, targets G, N per target, K, factor)
SITES = [("attn q/k/v", 3, 1536, 1536, 10), ("attn to_out", 1, 1536, 1536, 10), ("ff.net.0.proj", 1, 6144, 1536, 4), ("ff.net.2", 1, 1536, 6144, 4)]


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
    from simpletuner_amd.engine import lokr_factorization
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    M = batch * 4096
    rate = lambda n, ms: round(n / (ms * 1e-3) / 1e9, 1)
    for (site, G, N, K, f) in SITES:
        (ol, ok), (im, in_) = lokr_factorization(N, f), lokr_factorization(K, f)
        Nt = G * N
        W = (rnd(Nt, K) / K ** 0.5).to(BF16)
        Wf, WfT = torch.empty_like(W), torch.empty(K, Nt, dtype=BF16, device=dev)
        facs = [(rnd(ol, im), 0.02 * rnd(ok, in_), torch.empty(ok, in_, dtype=BF16, device=dev)) for _ in range(G)]
        targets = [(i * N, N, w1, w2, w2b) for i, (w1, w2, w2b) in enumerate(facs)]
        ms = _median_ms(lambda: ops.lokr_fold(W, targets, 1.0, Wf, WfT), iters)
        moved = 6 * Nt * K + G * 6 * ok * in_
        emit({"measurement": "lokr_fold", "site": site, "shape": f"W [{Nt}, {K}] G {G} w1 [{ol}, {im}] w2 [{ok}, {in_}]", "ms": round(ms, 4), "bytes": moved,
              "achieved_GBps": rate(moved, ms)})
        x, dy = rnd(M, K).to(BF16), rnd(M, Nt).to(BF16)
        w1, w2, w2b = facs[-1]
        n_off = (G - 1) * N
        dP, P = ops.lokr_scratch("dp", dev, M, im * ok), ops.lokr_scratch("p", dev, M, im * ok)
        g1, g2 = torch.zeros(ol, im, device=dev), torch.zeros(ok, in_, device=dev)
        ms = _median_ms(lambda: ops.lokr_mix(dy, n_off, w1, ok, dP), iters)
        moved = 2 * M * (ol + im) * ok
        emit({"measurement": "lokr_mix", "site": site, "shape": f"M {M} w1 [{ol}, {im}] ok {ok} (per target)", "ms": round(ms, 4), "bytes": moved, "achieved_GBps": rate(moved, ms)})
        ms = _median_ms(lambda: ops.lokr_dw2(dP, x, im, g2, alpha=1.0, accumulate=True), iters)
        flops, moved = 2 * M * im * ok * in_, 2 * M * im * (ok + in_)
        emit({"measurement": "lokr_dw2", "site": site, "shape": f"L [{M * im}, {ok}]^T R [{M * im}, {in_}] (per target)", "ms": round(ms, 4), "flops": flops,
              "achieved_TFLOPs": round(flops / (ms * 1e-3) / 1e12, 1), "bytes_once": moved, "GBps_if_read_once": rate(moved, ms)})
        ms = _median_ms(lambda: ops.gemm(x.view(M * im, in_), w2b, out=P.view(M * im, ok)), iters)
        emit({"measurement": "lokr_P_gemm", "site": site, "shape": f"[{M * im}, {in_}] x [{ok}, {in_}]^T (per target)", "ms": round(ms, 4), "flops": flops,
              "achieved_TFLOPs": round(flops / (ms * 1e-3) / 1e12, 1), "bytes_once": moved, "GBps_if_read_once": rate(moved, ms)})
        ms = _median_ms(lambda: ops.lokr_dw1(dy, n_off, P, g1, ok, alpha=1.0, accumulate=True), iters)
        flops, moved = 2 * M * ol * im * ok, 2 * M * (ol + im) * ok
        emit({"measurement": "lokr_dw1", "site": site, "shape": f"M {M} w1 [{ol}, {im}] ok {ok} (per target)", "ms": round(ms, 4), "flops": flops, "bytes": moved,
              "achieved_GBps": rate(moved, ms), "achieved_TFLOPs": round(flops / (ms * 1e-3) / 1e12, 2)})
        del W, Wf, WfT, x, dy


def _trainer(lokr: bool, batch: int):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4)
    if lokr:
        cfg.lora_type, cfg.lycoris_config = "lycoris", dict(LYCORIS)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(**ARCH)
    plugin.get_trained_component().init_synthetic(3)
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
    emit({"measurement": "sd3_step", "arch": f"SD3-Medium, 24 joint blocks, D 1536, batch {batch}, 4096 + 231 tokens, eager, synthetic weights; LoRA r32 on to_q/k/v/out.0 vs "
                                             "LoKr factor 10 on Attention + factor 4 on FeedForward", "steps": steps,
          "step_ms_lora_r32": round(med[False] * 1e3, 2), "step_ms_lokr": round(med[True] * 1e3, 2), "delta_ms": round((med[True] - med[False]) * 1e3, 2),
          "spread_ms_lora": round((max(times[False]) - min(times[False])) * 1e3, 2), "spread_ms_lokr": round((max(times[True]) - min(times[True])) * 1e3, 2),
          "adapter_bytes_lora": mem[False], "adapter_bytes_lokr": mem[True], "peak_device_bytes": torch.cuda.max_memory_allocated()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lokr_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.batch, args.iters)
    if args.part in ("step", "both"):
        step(args.batch, args.steps)
    if args.out:
        lines = ["# LoKr kernel and step measurements (tools/lokr_bench.py, one MI355X)", "",
                 f"`python tools/lokr_bench.py --part {args.part} --batch {args.batch} --steps {args.steps} --iters {args.iters}`", ""]
        for rec in RECORDS:
            lines.append(f"- **{rec['measurement']}** " + ", ".join(f"{k}: {v}" for k, v in rec.items() if k != "measurement"))
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

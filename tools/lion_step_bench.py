#!/usr/bin/env python3
"""Time the Lion launch (st355_lion_step*) next to the AdamW launch (st355_adamw_ema_step*) at the same n, in one process on one MI355X.

    python tools/lion_step_bench.py [--iters 20] [--rounds 5] [--rank 32]

Two arenas, each with and without the fused EMA: the Flux LoRA adapter arena ("all" targets, rank 32, fp32) and an SD3-Medium-sized bf16 full-fine-tune arena
(2.0 B parameters, Lion with its Kahan compensation buffer).  The two kernels alternate launch by launch; every launch is timed with its own pair of device events;
one "median" is the median of --iters timed launches after warm-up, and --rounds medians are taken so that the run-to-run spread stands next to the number.
Prints one JSON line per measurement: bytes per parameter as read off the operand lists (lion.hip / optim.hip), GB/s = those bytes over the median of the medians,
and that rate as a fraction of the HBM figure DESIGN.md uses (8 TB/s)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.muon_step_bench import flux_adapter_shapes  # noqa: E402

HBM_BYTES_PER_S = 8e12          # HBM3E 8 TB/s
SD3_MEDIUM_PARAMS = 2_000_000_000


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    return t0, t1


def measure(fns, iters, rounds, warmup=3):
    """fns: {name: callable}.  Alternates the callables launch by launch.  Returns {name: [median ms of each round]}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        ev = {k: [] for k in fns}
        for _ in range(iters):
            for k, fn in fns.items():
                ev[k].append(_timed(fn))
        torch.cuda.synchronize()
        for k in fns:
            out[k].append(statistics.median(a.elapsed_time(b) for a, b in ev[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--full-params", type=int, default=SD3_MEDIUM_PARAMS)
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20 timed launches per median")
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    n_lora = sum(r * c for r, c in flux_adapter_shapes("all", args.rank))
    arenas = [("flux lora r%d adapter arena (fp32)" % args.rank, torch.float32, n_lora),
              ("sd3-medium full fine-tune arena (bf16)", torch.bfloat16, args.full_params // 8 * 8)]
    for name, dtype, n in arenas:
        bf = dtype == torch.bfloat16
        rnd = lambda scale, dt=dtype: torch.empty(n, dtype=dt, device=dev).normal_(0.0, scale)
        p, g, ema = rnd(0.05), rnd(1e-2), rnd(0.05)
        lion_m = torch.zeros(n, dtype=dtype, device=dev)
        comp = torch.zeros(n, dtype=dtype, device=dev) if bf else None
        adam_m, adam_v = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        step = [0]

        def adam(e):
            step[0] += 1
            ops.adamw_ema_step(p, g, adam_m, adam_v, step[0], 1e-5, 0.9, 0.999, 1e-8, 1e-2, ema=e, ema_decay=0.999)

        for with_ema in (False, True):
            e = ema if with_ema else None
            fns = {"st355_lion_step" + ("_bf16" if bf else ""): lambda: ops.lion_step(p, g, lion_m, 1e-5, 0.9, 0.99, 1e-2, comp=comp, ema=e, ema_decay=0.999),
                   "st355_adamw_ema_step" + ("_bf16" if bf else ""): lambda: adam(e)}
            per_param = {"st355_lion_step": 20 + (8 if with_ema else 0), "st355_lion_step_bf16": 14 + (4 if with_ema else 0),
                         "st355_adamw_ema_step": 28 + (8 if with_ema else 0), "st355_adamw_ema_step_bf16": 22 + (4 if with_ema else 0)}
            res = measure(fns, args.iters, args.rounds)
            for k, meds in res.items():
                ms = statistics.median(meds)
                rate = per_param[k] * n / (ms * 1e-3)
                print(json.dumps({"arena": name, "params": n, "ema": with_ema, "what": k, "bytes_per_param": per_param[k], "ms": round(ms, 5),
                                  "ms_medians_min": round(min(meds), 5), "ms_medians_max": round(max(meds), 5), "rounds": args.rounds, "iters": args.iters,
                                  "GB_per_s": round(rate / 1e9, 1), "fraction_of_hbm_8TBps": round(rate / HBM_BYTES_PER_S, 4)}), flush=True)
        del p, g, ema, lion_m, comp, adam_m, adam_v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

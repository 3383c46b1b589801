#!/usr/bin/env python3
"""Time the 8-bit block-wise AdamW launch (st355_adamw8bit_step) next to the fp32-moment AdamW launch (st355_adamw_ema_step*) on the same arena, in one process
on one MI355X.

    python tools/adamw8bit_bench.py [--iters 20] [--rounds 5] [--rank 32] [--full-params 2000000000] [--counters]

Two arenas, each as fp32 and as bf16: the Flux LoRA adapter arena ("all" targets, rank 32: the tensors of the bench's step) and an SD3-Medium-sized full
fine-tune arena (1536 x 1536 matrices, each followed by a 1536-element vector that keeps fp32 moments).  The two kernels alternate launch by launch, every launch
timed with its own pair of device events; a "median" is the median of --iters launches after warm-up and --rounds medians give the spread.  One JSON line per
measurement: bytes per parameter read off the operand lists, GB/s over the median of the medians, the state bytes per parameter as allocated.
--counters: a handful of launches of the 8-bit kernel only, for a counter run of its own (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.lion_step_bench import HBM_BYTES_PER_S, SD3_MEDIUM_PARAMS, measure  # noqa: E402
from tools.muon_step_bench import flux_adapter_shapes  # noqa: E402


def arenas(rank, full_params):
    lora = [r * c for r, c in flux_adapter_shapes("all", rank)]
    full = []
    while sum(full) + 1536 * 1537 <= full_params:
        full += [1536 * 1536, 1536]
    return [(f"flux lora r{rank} adapter arena", lora), ("sd3-medium-sized full fine-tune arena", full)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--full-params", type=int, default=SD3_MEDIUM_PARAMS)
    ap.add_argument("--counters", action="store_true")
    args = ap.parse_args()
    if args.iters < 20 and not args.counters:
        raise SystemExit("--iters must be at least 20 timed launches per median")
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    books = ops.adamw8bit_books().to(dev)
    for name, numels in arenas(args.rank, args.full_params):
        offs = [0]
        for k in numels[:-1]:
            offs.append(offs[-1] + k)
        plan = ops.Adamw8bitPlan(offs, numels, dev)
        n = plan.end
        for dtype in (torch.float32, torch.bfloat16):
            bf = dtype == torch.bfloat16
            p = torch.empty(n, dtype=dtype, device=dev).normal_(0.0, 0.05)
            g = torch.empty(n, dtype=dtype, device=dev).normal_(0.0, 1e-2)
            st = [torch.full((plan.n_codes,), 127, dtype=torch.uint8, device=dev), torch.zeros(plan.n_codes, dtype=torch.uint8, device=dev),
                  torch.zeros(plan.n_scales, device=dev), torch.zeros(plan.n_scales, device=dev), torch.zeros(plan.n_plain, device=dev), torch.zeros(plan.n_plain, device=dev)]
            step = [0, 0]

            def a8():
                step[0] += 1
                ops.adamw8bit_step(plan, p, g, *st, books, step[0], 1e-5, 0.9, 0.999, 1e-6, 1e-2)

            if args.counters:
                for _ in range(3):
                    a8()
                torch.cuda.synchronize()
                continue
            adam_m, adam_v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)

            def adam():
                step[1] += 1
                ops.adamw_ema_step(p, g, adam_m, adam_v, step[1], 1e-5, 0.9, 0.999, 1e-6, 1e-2)

            esz = p.element_size()
            state_bytes = sum(t.numel() * t.element_size() for t in st)
            moved8 = 3 * esz * n + 4 * plan.n_codes + 16 * plan.n_scales + 16 * plan.n_plain       # p read + written, g read; codes, scales, plain moments read + written
            per = {"st355_adamw8bit_step": moved8 / n, "st355_adamw_ema_step" + ("_bf16" if bf else ""): 3 * esz + 16.0}
            res = measure({"st355_adamw8bit_step": a8, "st355_adamw_ema_step" + ("_bf16" if bf else ""): adam}, args.iters, args.rounds)
            for k, meds in res.items():
                ms = statistics.median(meds)
                rate = per[k] * n / (ms * 1e-3)
                print(json.dumps({"arena": name, "dtype": str(dtype), "params": n, "tensors": plan.n, "quantised_share": round(plan.n_codes / n, 4), "what": k,
                                  "bytes_per_param": round(per[k], 3), "state_bytes_per_param": round((state_bytes if "8bit" in k else 8 * n) / n, 4),
                                  "ms": round(ms, 5), "ms_medians_min": round(min(meds), 5), "ms_medians_max": round(max(meds), 5), "rounds": args.rounds,
                                  "iters": args.iters, "GB_per_s": round(rate / 1e9, 1), "fraction_of_hbm_8TBps": round(rate / HBM_BYTES_PER_S, 4)}), flush=True)
            del adam_m, adam_v
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

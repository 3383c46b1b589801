#!/usr/bin/env python3
"""Time the SOAP optimizer step over the Flux LoRA r32 adapter arenas ("all": 266 adapters, "all+ffs": 419) on one MI355X.

    python tools/soap_step_bench.py [--iters 20] [--rank 32]

Prints one JSON line per measurement: the plain st355_soap_step (no refresh), the step of a call that refreshes the eigenbasis, the first call
(Gram + eigensolver), and — on the same arena in the same run — the fused st355-adamw step, the Muon step and a device-to-device copy of the
arena (max_precond_dim = the rank: "all+ffs" holds a [64, r] adapter, whose long side bounds it; the measured copy bandwidth the achieved fraction is stated against: the step streams 7 x 4 B per parameter — p, g, m, v read, p, m, v
written).  The adapter shapes are those of tools/muon_step_bench.py."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.muon_step_bench import _time, flux_adapter_shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rank", type=int, default=32)
    args = ap.parse_args()
    from simpletuner_amd.training.optimizer import St355AdamW, St355Muon, St355Soap
    dev = torch.device("cuda:0")
    for target in ("all", "all+ffs"):
        shapes = flux_adapter_shapes(target, args.rank)
        n = sum(r * c for r, c in shapes)
        gen = torch.Generator(device=dev).manual_seed(0)
        flat = 1e-2 * torch.randn(n, device=dev, generator=gen)
        gflat = torch.randn(n, device=dev, generator=gen)
        ps, off = [], 0
        for r, c in shapes:
            p = torch.nn.Parameter(flat[off:off + r * c].view(r, c))
            p.grad = gflat[off:off + r * c].view(r, c)
            ps.append(p)
            off += r * c
        dst = torch.empty_like(flat)
        copy_ms = _time(lambda: dst.copy_(flat), args.iters)
        copy_gbs = 2 * 4 * n / copy_ms / 1e6
        print(json.dumps({"target": target, "what": "device copy of the arena", "params": n, "ms": round(copy_ms, 4), "GB_per_s": round(copy_gbs, 1)}), flush=True)
        base = dict(target=target, matrices=len(shapes), params=n)
        first = St355Soap(ps, lr=1e-3, max_precond_dim=args.rank)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record(); first.step(); t1.record()
        torch.cuda.synchronize()
        print(json.dumps({**base, "what": "st355_soap_step, first call (Gram, fold, eigensolver; includes one-time setup)", "ms": round(t0.elapsed_time(t1), 4),
                          "launches": first._flat[0]["plan"].launches(first=True)}), flush=True)
        del first
        for what, freq in (("st355_soap_step", 10 ** 9), ("st355_soap_step with refresh", 1)):
            opt = St355Soap(ps, lr=1e-3, max_precond_dim=args.rank, precondition_frequency=freq)
            opt.step()
            ms = _time(opt.step, args.iters)
            plan = opt._flat[0]["plan"]
            stream = 7 * 4 * n
            print(json.dumps({**base, "what": what, "ms": round(ms, 4), "launches": plan.launches(refresh=freq == 1),
                              "workspace_MiB": round(plan.ws_floats * 4 / 2**20, 1), "stream_GB": round(stream / 1e9, 3),
                              "GB_per_s": round(stream / ms / 1e6, 1), "fraction_of_copy_bandwidth": round(stream / ms / 1e6 / copy_gbs, 3)}), flush=True)
            del opt
        adam = St355AdamW(ps, lr=2e-4)
        print(json.dumps({"target": target, "what": "st355-adamw step (same arena)", "ms": round(_time(adam.step, args.iters), 4)}), flush=True)
        muon = St355Muon(ps, lr=2e-4)
        print(json.dumps({"target": target, "what": "st355_muon_step (same arena)", "ms": round(_time(muon.step, args.iters), 4)}), flush=True)
        del adam, muon, ps, flat, gflat, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

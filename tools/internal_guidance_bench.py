#!/usr/bin/env python3
"""Time the Internal Guidance head's entry points on one MI355X against the composition of existing ops that computes the same thing, in the same process.

    python tools/internal_guidance_bench.py [--iters 100] [--repeats 5] [--step-time] [--steps 6] [--markdown profiles/internal_guidance_kernel_stats.md]

Shapes [B * S_img, D]: [16 * 4096, 1536] (SD3-Medium) and [8 * 4096, 3072].  Per shape, `repeats` timings of `iters` back-to-back calls each (device events, after a
warm-up); reported: the median and the run-to-run spread (max - min over the repeats).

  ig_head_fwd   st355_ig_head_fwd (xhat, rstd) + the thin GEMM on xhat            vs  ln_modulate_fwd(scale = gamma - 1, shift = beta) + gemm
  ig_head_bwd   st355_ig_head_bwd (g = dy W' on the MFMA, never stored)           vs  gemm (dn [M, D]) + ln_modulate_bwd_stats + a layersync_inject-style add
  ig_wgrad      skinny_tn (dy^T xhat) + colsum + st355_ig_wgrad                   vs  gemm_tn (dy^T n) + colsum_prod

Bytes are the algorithm's (what the fused form must move); the rate is set against a device-to-device copy of the same size measured in this process.
--step-time also measures an SD3 LoRA train step at `bench.py --model sd3`'s shape (SD3-Medium: 24 joint blocks, D 1536, LoRA r32, batch 8, 1024^2, 4096 + 231 tokens,
AdamW, eager) through the plugin and the trainer with the regulariser off and on, alternating."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = {"sd3_b16": dict(B=16, rows=4096, D=1536), "d3072_b8": dict(B=8, rows=4096, D=3072)}
BF16, F32 = torch.bfloat16, torch.float32


def _time(fn, iters, repeats):
    for _ in range(5):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / iters * 1e-3)
    out.sort()
    return out[len(out) // 2], out[-1] - out[0]


def kernels(iters, repeats):
    from simpletuner_amd import ops
    from simpletuner_amd.engine import pad64
    dev = torch.device("cuda:0")
    rows_out = []
    for name, sh in SHAPES.items():
        B, rows, D = sh["B"], sh["rows"], sh["D"]
        M, N = B * rows, ops.IG_N
        g = torch.Generator(device=dev).manual_seed(1)
        rn = lambda *s: torch.randn(*s, generator=g, device=dev)
        h = rn(M, D).to(BF16)
        dxb = rn(M, D).to(BF16)
        dy = (rn(M, N) / 64).to(BF16)
        gamma, beta, W, b = 1.0 + 0.25 * rn(D), 0.1 * rn(D), rn(N, D) / D ** 0.5, 0.05 * rn(N)
        Wf, WfT, c = torch.empty(N, D, dtype=BF16, device=dev), torch.empty(D, N, dtype=BF16, device=dev), torch.empty(N, dtype=BF16, device=dev)
        xhat, rstd, y = torch.empty(M, D, dtype=BF16, device=dev), torch.empty(M, dtype=F32, device=dev), torch.empty(M, N, dtype=BF16, device=dev)
        grads = [torch.zeros_like(t) for t in (gamma, beta, W, b)]
        ops.ig_fold(gamma, beta, W, b, Wf, WfT, c)
        hv, dxv = h.view(B, rows, D), dxb.view(B, rows, D)
        # the composition's operands
        sc, sf = (gamma - 1.0).to(BF16).view(1, D), beta.to(BF16).view(1, D)
        W16, b16, WT16 = W.to(BF16), b.to(BF16), W.to(BF16).t().contiguous()
        n_out, dn, dsh, dscl = torch.empty(M, D, dtype=BF16, device=dev), torch.empty(M, D, dtype=BF16, device=dev), torch.zeros(1, D, device=dev), torch.zeros(1, D, device=dev)
        one = torch.ones((), device=dev)
        gw, gb = torch.empty(N, D, dtype=BF16, device=dev), torch.empty(1, N, device=dev)
        src, dst = torch.empty(M * D, dtype=BF16, device=dev), torch.empty(M * D, dtype=BF16, device=dev)
        t_copy, _ = _time(lambda: dst.copy_(src), iters, repeats)
        copy_bw = 2 * 2 * M * D / t_copy                                             # bytes read + written per second

        def comp_fwd():
            ops.ln_modulate_fwd(h, sc, sf, M, out=n_out)
            ops.gemm(n_out, W16, bias=b16, out=y)

        def comp_bwd():
            ops.gemm(dy, WT16, out=dn)
            dx_, _ = ops.ln_modulate_bwd_stats(dn, h, sc, M, dsh, dscl)
            ops.layersync_inject(dxv, dx_, one)

        def comp_wgrad():
            ops.gemm_tn(pad64(dy), pad64(n_out), out=gw)
            ops.colsum_prod(dy, gb)

        cases = (("ig_head_fwd", lambda: ops.ig_head_fwd(hv, Wf, c, xhat, rstd, y), comp_fwd, 2 * 2 * M * D + 2 * M * N),
                 ("ig_head_bwd", lambda: ops.ig_head_bwd(xhat, rstd, dy, WfT, dxv), comp_bwd, 3 * 2 * M * D + 2 * M * N),
                 ("ig_wgrad", lambda: ops.ig_wgrad(xhat, dy, gamma, beta, W, *grads), comp_wgrad, 2 * M * D + 2 * M * N))
        ops.ig_head_fwd(hv, Wf, c, xhat, rstd, y)
        comp_fwd()
        for what, fused, comp, nbytes in cases:
            tf, sf_ = _time(fused, iters, repeats)
            tc, sc_ = _time(comp, iters, repeats)
            rec = {"kernel": what, "shape": name, **sh, "fused_us": round(tf * 1e6, 1), "fused_spread_us": round(sf_ * 1e6, 1), "composition_us": round(tc * 1e6, 1),
                   "composition_spread_us": round(sc_ * 1e6, 1), "bytes": nbytes, "share_of_copy_bandwidth": round(nbytes / tf / copy_bw, 3),
                   "copy_GBps": round(copy_bw / 1e9, 1), "no_slower_than_composition": bool(tf <= tc + max(sf_, sc_))}
            print(json.dumps(rec), flush=True)
            rows_out.append(rec)
    return rows_out


def step_time(steps):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    arch = dict(num_layers=24, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536, pooled_projection_dim=2048,
                pos_embed_max_size=192, sample_size=128)
    runs = {}
    for on in (False, True):
        cfg = default_config(model_family="sd3", lora_rank=32, train_batch_size=8, seed=5, learning_rate=1e-4, internal_guidance_enabled=on)
        acc = St355Accelerator(dev)
        plugin = SD3(cfg, acc)
        plugin.load_model(**arch)
        plugin.add_lora_adapter()
        plugin.post_model_load_setup()
        runs[on] = (plugin, Trainer(cfg, plugin, acc))
    _, devt = PU.make_inputs(8, 128, 128, 231, 4096, 2048, dev, seed=5)
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
    rec = {"measurement": "sd3_lora_step_bench_shape", "arch": "SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch 8, 4096 + 231 tokens, eager", "steps": steps,
           "step_ms_internal_guidance_off": round(med[False] * 1e3, 2), "step_ms_internal_guidance_on": round(med[True] * 1e3, 2),
           "delta_ms": round((med[True] - med[False]) * 1e3, 3), "spread_ms_off": round((max(times[False]) - min(times[False])) * 1e3, 3),
           "note": "on includes the head's loss pass and the two host reads of auxiliary_loss's logs"}
    print(json.dumps(rec), flush=True)
    return rec


def markdown(path, rows, step):
    lines = ["# Internal Guidance head: fused entry points against the composition of existing ops", "",
             "Written by `tools/internal_guidance_bench.py` on one MI355X; times are medians of repeated timings, spread = max - min over the repeats.", "",
             "| entry | shape [M, D] | fused us | spread | composition us | spread | bytes moved | share of copy bandwidth | no slower |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['kernel']} | [{r['B'] * r['rows']}, {r['D']}] | {r['fused_us']} | {r['fused_spread_us']} | {r['composition_us']} | {r['composition_spread_us']} | "
                     f"{r['bytes']} | {r['share_of_copy_bandwidth']} (copy: {r['copy_GBps']} GB/s) | {'yes' if r['no_slower_than_composition'] else 'NO'} |")
    if step:
        lines += ["", f"SD3 LoRA step ({step['arch']}): {step['step_ms_internal_guidance_off']} ms off, {step['step_ms_internal_guidance_on']} ms on "
                      f"(delta {step['delta_ms']} ms, spread of the off runs {step['spread_ms_off']} ms; {step['note']})."]
    Path(path).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-time", action="store_true")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("internal_guidance_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    rows = kernels(args.iters, args.repeats)
    step = step_time(args.steps) if args.step_time else None
    if args.markdown:
        markdown(args.markdown, rows, step)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measure the Flow-DPO kernels and the Flow-DPO step on one MI355X.

    python tools/flow_dpo_bench.py [--part kernels|step|both] [--pairs 4] [--steps 6] [--iters 20] [--family sd3|flux] [--out profiles/flow_dpo_kernel_stats.md]

kernels   ops.flow_dpo_stats + flow_dpo_head + flow_dpo_grad at latents [pairs, 16, 128, 128] and [8, 16, 128, 128] (pairs) by device events, against
  copy    a bf16 copy of the bytes the kernels must move (the lower bound), and
  eager   the reference's formula as torch operations on bf16 device tensors with autograd (four per-sample errors, the margin as their differences);
          also what that margin loses to cancellation against fp64, with policy = reference + 1e-3 (LoRA initialisation).
step      the SD3-Medium (or Flux.1-dev-width) LoRA r32 step with `pairs` pairs under distillation_method=flow_dpo, alternating in one process with the plain step
          at batch 2 pairs and a no-grad forward at batch 2 pairs.  The expectation — to be confirmed or refuted here, not asserted anywhere — is
          DPO step ~ plain step at batch 2 pairs + no-grad forward at batch 2 pairs + the kernel time above.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SD3_ARCH = dict(num_layers=24, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536, pooled_projection_dim=2048,
                pos_embed_max_size=192, sample_size=128)
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
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


def eager_loss(policy, ref, tw, tl, beta=0.02, anchor_alpha=0.0):
    """the reference's expression in torch operations on bf16 device tensors (float casts where the reference casts), with autograd"""
    B = tw.shape[0]
    p = policy.detach().requires_grad_(True)
    dims = tuple(range(1, p.dim()))
    err = lambda x, t: (x.float() - t.float()).pow(2).sum(dim=dims)
    margin = (err(ref[:B], tw) - err(p[:B], tw)) + (err(p[B:], tl) - err(ref[B:], tl))
    loss = -torch.nn.functional.logsigmoid(0.5 * beta * margin.float()).mean()
    if anchor_alpha != 0.0:
        loss = loss + 0.5 * anchor_alpha * (torch.nn.functional.mse_loss(p[:B].float(), ref[:B].float()) + torch.nn.functional.mse_loss(p[B:].float(), ref[B:].float()))
    loss.backward()
    return loss, p.grad, margin.detach()


def kernels(pairs: int, iters: int):
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    for B in sorted({pairs, 8}):
        shape = (B, 16, 128, 128)
        n = B * 16 * 128 * 128
        rn = lambda rows: torch.randn(rows, 16, 128, 128, generator=g, device=dev)
        ref32, tw, tl = rn(2 * B), rn(B).to(BF16), rn(B).to(BF16)
        ref = ref32.to(BF16)
        policy = (ref32 + 0.1 * rn(2 * B)).to(BF16)
        for anchor in (0.0, 0.5):
            def fused():
                st = ops.flow_dpo_stats(policy, ref, tw, tl)
                loss, pair, logs = ops.flow_dpo_head(st, n // B, beta=0.02, anchor_alpha=anchor)
                return loss, ops.flow_dpo_grad(policy, ref, tw, tl, pair, anchor_alpha=anchor), pair
            stats_ms = _median_ms(lambda: ops.flow_dpo_stats(policy, ref, tw, tl), iters)
            fused_ms = _median_ms(fused, iters)
            eager_ms = _median_ms(lambda: eager_loss(policy, ref, tw, tl, 0.02, anchor), iters)
            # the bytes the kernels must move: stats reads policy + ref (2 x 2n) and both targets (2 x n); grad reads policy (2n) [+ ref (2n)] and the targets, writes 2n
            elems = (4 + 2) + (2 + (2 if anchor else 0) + 2 + 2)
            src = torch.empty(elems * n // 2, dtype=BF16, device=dev)
            dst = torch.empty_like(src)
            copy_ms = _median_ms(lambda: dst.copy_(src), iters)          # reads and writes elems n / 2 each: elems n elements moved
            f_loss, f_grad, pair = fused()
            e_loss, e_grad, e_margin = eager_loss(policy, ref, tw, tl, 0.02, anchor)
            emit({"measurement": "flow_dpo_kernels", "pairs_shape": list(shape), "anchor_alpha": anchor, "iters": iters, "stats_ms": round(stats_ms, 4),
                  "stats_head_grad_ms": round(fused_ms, 4), "bytes_moved": 2 * elems * n, "fused_GBps": round(2 * elems * n / (fused_ms * 1e-3) / 1e9, 1),
                  "bf16_copy_of_those_bytes_ms": round(copy_ms, 4), "copy_GBps": round(2 * elems * n / (copy_ms * 1e-3) / 1e9, 1),
                  "fused_over_copy": round(fused_ms / copy_ms, 2), "torch_eager_bf16_ms": round(eager_ms, 4), "eager_over_fused": round(eager_ms / fused_ms, 2),
                  "loss_fused": round(f_loss.item(), 6), "loss_eager": round(e_loss.item(), 6),
                  "grad_rel_l2_eager_vs_fused": round(((e_grad.float() - f_grad.float()).norm() / f_grad.float().norm()).item(), 5)})
        # cancellation: policy = reference + 1e-3 (bf16 operands), the margin of both forms against fp64 on the same operands
        near = (ref.float() + 1e-3).to(BF16)
        st = ops.flow_dpo_stats(near, ref, tw, tl)
        fused_margin = (st[:, 7] + st[:, 8]).double().cpu()
        _, _, e_margin = eager_loss(near, ref, tw, tl)
        d = lambda t: t.double().cpu().reshape(t.shape[0], -1)
        p64, r64, a64, b64 = d(near), d(ref), d(tw), d(tl)
        want = ((r64[:B] - p64[:B]) * (r64[:B] + p64[:B] - 2 * a64)).sum(1) + ((p64[B:] - r64[B:]) * (p64[B:] + r64[B:] - 2 * b64)).sum(1)
        emit({"measurement": "flow_dpo_margin_cancellation", "pairs_shape": list(shape), "policy": "reference + 1e-3, rounded to bf16",
              "fp64_margin": [round(v, 4) for v in want.tolist()], "element_wise_fp32_abs_error_max": float((fused_margin - want).abs().max()),
              "four_sum_eager_abs_error_max": float((e_margin.double().cpu() - want).abs().max()),
              "per_sample_error_sum_magnitude": round(float(((r64[:B] - a64) ** 2).sum(1).mean()), 1)})


def _trainer(family: str, batch: int, dpo: bool):
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    extra = dict(distillation_method="flow_dpo") if dpo else {}
    cfg = default_config(model_family=family, lora_rank=32, train_batch_size=batch, seed=5, learning_rate=1e-4, **extra)
    acc = St355Accelerator(dev)
    if family == "sd3":
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, acc)
        plugin.load_model(**SD3_ARCH)
    else:
        from simpletuner_amd.flux.model import Flux
        plugin = Flux(cfg, acc)
        plugin.load_model()
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return Trainer(cfg, plugin, acc)


def step(family: str, pairs: int, steps: int):
    from tests import parity_utils as PU
    dev = torch.device("cuda:0")
    dims = dict(sd3=(231, 4096, 2048), flux=(512, 4096, 768))[family]
    _, d2 = PU.make_inputs(2 * pairs, 128, 128, dims[0], dims[1], dims[2], dev, seed=5)
    plain, dpo = _trainer(family, 2 * pairs, False), _trainer(family, pairs, True)
    sig2 = d2["sigmas"]
    plain.model.sample_flow_sigmas = lambda batch, state: (sig2, sig2 * 1000.0)
    dpo.model.sample_flow_sigmas = lambda batch, state: (sig2[:pairs], sig2[:pairs] * 1000.0)
    b_plain = {"latent_batch": d2["latents"], "prompt_embeds": d2["prompt"], "add_text_embeds": d2["pooled"], "noise": d2["noise"]}
    b_dpo = {"latent_batch": d2["latents"][:pairs], "prompt_embeds": d2["prompt"][:pairs], "add_text_embeds": d2["pooled"][:pairs], "noise": d2["noise"][:pairs],
             "conditioning_latents": d2["latents"][pairs:], "conditioning_type": "reference_strict"}

    def nograd_forward():
        pb = plain.model.prepare_batch(dict(b_plain), plain.state)
        with torch.no_grad():
            plain.model.model_predict(pb)

    runs = {"plain_step_at_2x": lambda: plain.train_step(dict(b_plain)), "nograd_forward_at_2x": nograd_forward, "dpo_step": lambda: dpo.train_step(dict(b_dpo))}
    times = {k: [] for k in runs}
    for i in range(2 + steps):
        for k, fn in runs.items():          # alternating, same process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 2:
                times[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    spread = {k: (max(v) - min(v)) * 1e3 for k, v in times.items()}
    emit({"measurement": f"{family}_lora_flow_dpo_step", "arch": f"{family}, LoRA r32, {pairs} pairs (forwards at batch {2 * pairs}), 128 x 128 latents, eager, synthetic weights",
          "steps": steps, "dpo_step_ms": round(med["dpo_step"], 2), "plain_step_at_batch_2x_ms": round(med["plain_step_at_2x"], 2),
          "nograd_forward_at_batch_2x_ms": round(med["nograd_forward_at_2x"], 2),
          "dpo_minus_plain_minus_forward_ms": round(med["dpo_step"] - med["plain_step_at_2x"] - med["nograd_forward_at_2x"], 2),
          "spread_ms": {k: round(v, 2) for k, v in spread.items()}, "logs": dpo.last_aux_logs})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "both"), default="both")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--family", choices=("sd3", "flux"), default="sd3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("flow_dpo_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    if args.part in ("kernels", "both"):
        kernels(args.pairs, args.iters)
    if args.part in ("step", "both"):
        step(args.family, args.pairs, args.steps)
    if args.out:
        lines = ["# Flow-DPO kernel and step measurements (tools/flow_dpo_bench.py, one MI355X)", "",
                 f"`python tools/flow_dpo_bench.py --part {args.part} --pairs {args.pairs} --steps {args.steps} --iters {args.iters} --family {args.family}`", ""]
        for rec in RECORDS:
            lines.append(f"- **{rec['measurement']}** " + ", ".join(f"{k}: {v}" for k, v in rec.items() if k != "measurement"))
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measure the Diff2Flow loss kernel and the SDXL-LoRA step under the flags on one MI355X.

    python tools/diff2flow_bench.py [--part kernels|step|both] [--iters 30] [--batch 4] [--steps 6] [--out FILE.jsonl]

kernels   at latents [16, 4, 128, 128], [32, 4, 128, 128] (SDXL at 1024^2, the bench line's batches) and [16, 4, 64, 64], by device events around warmed calls,
          launches included, the variants alternating:
  fused   ops.diff2flow_loss with gradient (reads pred, noisy, tau; writes dpred),
  cond    ops.cond_loss (l2, with gradient): the loss these families run without the flags (reads pred, target; writes dpred) — one operand fewer,
  masked  the fused call with a [B, H * W] element mask (the conditioning-mask losses),
  eager   the reference's formula as torch operations on bf16 device tensors with bf16 tables (what `bridge.to(dtype=weight_dtype)` leaves) and autograd;
          and the value each path computes.  Each variant is timed twice: as eager calls (host launch cost included: at these sizes the host is the limit) and as
          20 calls captured into one hipGraph and replayed (the device time of one call: what a captured step pays).
step      the SDXL-LoRA r16 step at 1024^2 with and without the flags, alternating in one process.  The expected difference is the kernel difference.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BF16, F32 = torch.bfloat16, torch.float32
RECORDS = []


def emit(rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def _alternate_ms(fns: dict, iters: int) -> dict:
    """median device-event time of every variant, one call of each per round so that clock and cache state are shared"""
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def _graph_ms(fns: dict, iters: int, calls: int = 20) -> dict:
    """device time of one call: `calls` calls captured into one graph, replayed, the variants alternating"""
    graphs = {}
    side = torch.cuda.Stream()
    for k, f in fns.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            f()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(calls):
                f()
        graphs[k] = g
    ms = _alternate_ms({k: g.replay for k, g in graphs.items()}, iters)
    return {k: v / calls for k, v in ms.items()}


def eager_loss(bridge16, pred, noisy, tau, t):
    """common.py:6238-6248 + 6426-6429 with the bridge's tables in bf16, as torch operations with autograd"""
    p = pred.detach().requires_grad_(True)
    ra, rm = bridge16[0][t].view(-1, 1, 1, 1), bridge16[1][t].view(-1, 1, 1, 1)
    pf, xf = p.float(), noisy.float()
    flow = pf - (ra * xf - rm * pf)
    loss = torch.nn.functional.mse_loss(flow.float(), tau.float(), reduction="none").mean(dim=(1, 2, 3)).mean()
    loss.backward()
    return loss, p.grad


def kernels(iters: int):
    from simpletuner_amd import ops
    from simpletuner_amd.diff2flow import Diff2FlowBridge
    from simpletuner_amd.foundation import DDPMSchedule
    dev = torch.device("cuda:0")
    br = Diff2FlowBridge(DDPMSchedule().alphas_cumprod, device=dev)
    table = br.table("epsilon")
    b16 = (br.sqrt_recip_alphas_cumprod.to(BF16), br.sqrt_recipm1_alphas_cumprod.to(BF16))
    g = torch.Generator(device=dev).manual_seed(1)
    for shape in ((16, 4, 128, 128), (32, 4, 128, 128), (16, 4, 64, 64)):
        B = shape[0]
        n = 1
        for s in shape:
            n *= s
        rn = lambda: torch.randn(*shape, generator=g, device=dev)
        lat, noise = rn(), rn()
        t = torch.linspace(5, 994, B, device=dev).long()
        a = DDPMSchedule().alphas_cumprod.to(dev)[t].view(-1, 1, 1, 1)
        noisy = (a.sqrt() * lat + (1 - a).sqrt() * noise).to(BF16)
        pred = (noise + 0.1 * rn()).to(BF16)
        tau = (noise.to(BF16) - lat.to(BF16))
        target = noise.to(BF16)
        emask = torch.rand(B, shape[2] * shape[3], generator=g, device=dev)
        fns = {"fused": lambda: ops.diff2flow_loss(pred, noisy, tau, t, table, "epsilon"),
               "masked": lambda: ops.diff2flow_loss(pred, noisy, tau, t, table, "epsilon", emask=emask),
               "cond": lambda: ops.cond_loss(pred, target, "l2")}
        ms = _alternate_ms(dict(fns, eager=lambda: eager_loss(b16, pred, noisy, tau, t)), iters)
        dev_ms = _graph_ms(fns, iters)
        f_loss, _, f_grad = ops.diff2flow_loss(pred, noisy, tau, t, table, "epsilon")
        c_loss, _, _ = ops.cond_loss(pred, target, "l2")
        e_loss, e_grad = eager_loss(b16, pred, noisy, tau, t)
        emit({"measurement": "diff2flow_kernel", "shape": list(shape), "iters": iters, "fused_ms": round(ms["fused"], 4), "cond_loss_l2_ms": round(ms["cond"], 4),
              "fused_masked_ms": round(ms["masked"], 4), "torch_eager_bf16_tables_ms": round(ms["eager"], 4), "fused_over_cond": round(ms["fused"] / ms["cond"], 3),
              "captured_fused_ms": round(dev_ms["fused"], 5), "captured_fused_masked_ms": round(dev_ms["masked"], 5), "captured_cond_loss_l2_ms": round(dev_ms["cond"], 5),
              "captured_fused_over_cond": round(dev_ms["fused"] / dev_ms["cond"], 3), "captured_fused_GBps": round(8 * n / (dev_ms["fused"] * 1e-3) / 1e9, 1),
              "captured_cond_GBps": round(6 * n / (dev_ms["cond"] * 1e-3) / 1e9, 1),
              "eager_over_fused": round(ms["eager"] / ms["fused"], 2), "fused_bytes": 8 * n, "fused_GBps": round(8 * n / (ms["fused"] * 1e-3) / 1e9, 1),
              "cond_bytes": 6 * n, "cond_GBps": round(6 * n / (ms["cond"] * 1e-3) / 1e9, 1), "loss_fused_fp32_tables": round(f_loss.item(), 6),
              "loss_eager_bf16_tables": round(e_loss.item(), 6), "loss_plain_epsilon_mse": round(c_loss.item(), 6),
              "grad_rel_l2_eager_vs_fused": round(((e_grad.float() - f_grad.float()).norm() / f_grad.float().norm()).item(), 5)})


def step(batch: int, steps: int):
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")

    def trainer(**over):
        cfg = default_config(model_family="sdxl", model_type="lora", lora_rank=16, train_batch_size=batch, seed=5, learning_rate=1e-4, **over)
        acc = St355Accelerator(dev)
        pl = SDXL(cfg, acc)
        pl.load_model()
        pl.add_lora_adapter()
        return Trainer(cfg, pl, acc)

    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g, device=dev).to(BF16)
    b = {"latent_batch": r(batch, 4, 128, 128), "prompt_embeds": r(batch, 77, 2048), "add_text_embeds": r(batch, 1280),
         "batch_time_ids": torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * batch, device=dev, dtype=BF16), "noise": r(batch, 4, 128, 128),
         "timesteps": torch.linspace(5, 994, batch).long()}
    plain, d2f = trainer(), trainer(diff2flow_enabled=True, diff2flow_loss=True)
    runs = {"plain_step": lambda: plain.train_step(dict(b)), "diff2flow_step": lambda: d2f.train_step(dict(b))}
    ms = _alternate_ms(runs, steps)
    emit({"measurement": "sdxl_lora_r16_step", "batch": batch, "res": 1024, "steps": steps, "plain_step_ms": round(ms["plain_step"], 3),
          "diff2flow_step_ms": round(ms["diff2flow_step"], 3), "difference_ms": round(ms["diff2flow_step"] - ms["plain_step"], 3),
          "loss_plain": round(float(plain.last_loss), 6), "loss_diff2flow": round(float(d2f.last_loss), 6)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["kernels", "step", "both"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.part in ("kernels", "both"):
        kernels(a.iters)
    if a.part in ("step", "both"):
        step(a.batch, a.steps)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in RECORDS))


if __name__ == "__main__":
    main()

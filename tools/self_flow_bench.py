#!/usr/bin/env python3
"""Self-Flow at SD3-Medium shapes on the MI355X: the views kernel against the launches it replaces, the teacher forward, the alignment path and the step.

    python tools/self_flow_bench.py [--steps 4] [--batch 4] [--student 8] [--teacher 20] [--only views|teacher|align|step]
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/self_flow_bench.py --only step --steps 2        (no counters in the same run)

SD3-Medium: 24 joint blocks, D 1536, LoRA r32, 1024^2 (latents [B, 16, 128, 128], 4096 image + 231 text tokens), eager, through the component.  One JSON line per
measurement, device events around windows that end in a synchronise, medians over `--steps` windows behind two warm-up windows, alternating where two things are compared:

  views     st355_self_flow_views at batch 16 against the parent commit's equivalent — two ops.flow_noise_mix launches (the base and the alternate view) and the
            torch elementwise ops for the mask, the token timesteps, the minima and the two selections.  Algorithmic bytes: 4 tensors of B C H W bf16 (2 in, 2 out).
  teacher   the capture forward inside teacher_values(shadow) (ends behind the teacher block, packs from the shadow, re-packs on exit) against a plain no-grad forward.
  align     SelfFlowTap.tap and .backward alone at M = batch * 4096 rows: fold, rows, projection, cosine; colsum, P, wgrad, g, LayerNorm backward.  Algorithmic
            bytes per launch are printed with it (bf16 2 bytes, fp32 4): fold 12 D^2, rows 4 M D, cosine 6 M D, ln_bwd_add 8 M D, wgrad 10 D^2.
  step      teacher forward + tokenwise training forward with the tap + backward, against the plain tokenwise LoRA forward + backward (no optimizer in either)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ARCH = dict(num_layers=24, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536, pooled_projection_dim=2048,
            pos_embed_max_size=192, sample_size=128)
BF16, F32 = torch.bfloat16, torch.float32


def timed(fns: dict, steps: int, warm: int = 2):
    """{name: callable} run alternately; -> {name: (median ms, spread ms)} from device events"""
    times = {k: [] for k in fns}
    for i in range(warm + steps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            if i >= warm:
                times[k].append(a.elapsed_time(b))
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in times.items()}


def bench_views(dev, steps: int):
    from simpletuner_amd import ops
    B, C, H, W, p, ratio = 16, 16, 128, 128, 2, 0.25
    g = torch.Generator(device=dev).manual_seed(1)
    lat, noise = torch.randn(B, C, H, W, generator=g, device=dev).to(BF16), torch.randn(B, C, H, W, generator=g, device=dev).to(BF16)
    sig, alt, u = torch.rand(B, generator=g, device=dev), torch.rand(B, generator=g, device=dev), torch.rand(B, H // p, W // p, generator=g, device=dev)
    t0, t1 = sig * 1000, alt * 1000

    def fused():
        return ops.self_flow_views(lat, noise, sig, alt, t0, t1, u, ratio, p)

    def parent():
        base, _, _ = ops.flow_noise_mix(lat, sig, noise=noise, want_target=False)
        other, _, _ = ops.flow_noise_mix(lat, alt, noise=noise, want_target=False)
        mask = u < ratio
        tok = torch.where(mask, t1.view(B, 1, 1), t0.view(B, 1, 1)).flatten(1)
        grid = mask.repeat_interleave(p, dim=1).repeat_interleave(p, dim=2)[:, None]
        student = torch.where(grid, other, base)
        teacher = torch.where((alt < sig).view(B, 1, 1, 1), other, base)
        return student, teacher, tok, torch.minimum(sig, alt), torch.minimum(t0, t1)

    a, b = fused(), parent()
    same = bool(torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and (a[0].float() - b[0].float()).abs().max() <= 2.0 ** -6 * a[0].float().abs().max())
    r = timed({"fused": fused, "parent": parent}, max(steps, 20), warm=5)
    nbytes = 4 * B * C * H * W * 2
    print(json.dumps({"measurement": "self_flow_views", "shape": [B, C, H, W], "ratio": ratio, "fused_us": round(r["fused"][0] * 1e3, 2), "fused_spread_us": round(r["fused"][1] * 1e3, 2),
                      "parent_equivalent_us": round(r["parent"][0] * 1e3, 2), "parent_spread_us": round(r["parent"][1] * 1e3, 2), "algorithmic_bytes": nbytes,
                      "fused_TBps": round(nbytes / (r["fused"][0] * 1e-3) / 1e12, 3), "outputs_agree": same}), flush=True)


def build(dev, student: int, teacher: int, tap: bool):
    from simpletuner_amd.sd3.transformer import SD3Transformer2DModel
    m = SD3Transformer2DModel(device=dev, **ARCH)
    m.init_synthetic(5)
    if tap:
        m.set_self_flow(student, teacher)
    m.add_lora_adapter(rank=32, seed=12, init_b_std=0.02)
    m.prepare_for_training()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--student", type=int, default=8)
    ap.add_argument("--teacher", type=int, default=20)
    ap.add_argument("--only", choices=("views", "teacher", "align", "step"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("self_flow_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    dev = torch.device("cuda:0")
    want = lambda k: args.only in (None, k)
    if want("views"):
        bench_views(dev, args.steps)
    if args.only == "views":
        return
    from simpletuner_amd.engine import SelfFlowTap
    from tests import parity_utils as PU
    B, Si, D = args.batch, 4096, 1536
    _, devt = PU.make_inputs(B, 128, 128, 231, 4096, 2048, dev, seed=5)
    lat, prompt, pooled = devt["latents"], devt["prompt"], devt["pooled"]
    g = torch.Generator(device=dev).manual_seed(2)
    base, alt = torch.rand(B, 1, generator=g, device=dev) * 800 + 100, torch.rand(B, 1, generator=g, device=dev) * 800 + 100
    tok = torch.where(torch.rand(B, Si, generator=g, device=dev) < 0.25, alt, base).contiguous()
    t_T = torch.minimum(base, alt).reshape(B)
    target = torch.randn(lat.shape, generator=g, device=dev).to(BF16)
    model = build(dev, args.student, args.teacher, tap=True)
    shadow = model.lora_flat.clone() + 1e-3 * torch.randn(model.lora_flat.shape, generator=g, device=dev)
    fwd = dict(hidden_states=lat, encoder_hidden_states=prompt, pooled_projections=pooled)

    def teacher_fwd():
        with torch.no_grad(), model.teacher_values(shadow):
            return model(timestep=t_T, crepa_capture_block_index=args.teacher, **fwd).crepa_hidden_states

    def plain_fwd():
        with torch.no_grad():
            return model(timestep=t_T, **fwd).sample

    arch = f"SD3-Medium, 24 joint blocks, D 1536, LoRA r32, batch {B}, 4096 + 231 tokens, eager"
    if want("teacher"):
        r = timed({"teacher": teacher_fwd, "plain": plain_fwd}, args.steps)
        print(json.dumps({"measurement": "teacher_forward", "arch": arch, "teacher_block": args.teacher, "teacher_ms": round(r["teacher"][0], 2), "teacher_spread_ms": round(r["teacher"][1], 2),
                          "plain_no_grad_forward_ms": round(r["plain"][0], 2), "plain_spread_ms": round(r["plain"][1], 2)}), flush=True)
    if want("align"):
        M = B * Si
        h = torch.randn(B, Si, D, generator=g, device=dev).to(BF16)
        feats = torch.randn(B, Si, D, generator=g, device=dev).to(BF16)
        dx = torch.zeros(B, Si, D, dtype=BF16, device=dev)
        dsim = torch.tensor(-0.5, device=dev)
        taps = []

        def tap_fwd():
            t = SelfFlowTap(model._sf, feats)
            t.tap(model._sf.block, h)
            taps.append(t)

        def tap_bwd():
            taps.pop().backward(dsim, dx)

        r = timed({"tap": tap_fwd, "backward": tap_bwd}, args.steps)
        print(json.dumps({"measurement": "align_path", "M": M, "D": D, "tap_ms": round(r["tap"][0], 3), "tap_spread_ms": round(r["tap"][1], 3), "backward_ms": round(r["backward"][0], 3),
                          "backward_spread_ms": round(r["backward"][1], 3),
                          "algorithmic_bytes": {"fold": 12 * D * D, "rows": 4 * M * D, "projection_gemm": 4 * M * D + 2 * D * D, "cosine": 6 * M * D, "colsum": 2 * M * D,
                                                "P_gemm_tn": 4 * M * D + 2 * D * D, "wgrad": 10 * D * D, "g_gemm": 4 * M * D + 2 * D * D, "ln_bwd_add": 8 * M * D}}), flush=True)
    if want("step"):
        plain = build(dev, args.student, args.teacher, tap=False)

        def step_self_flow():
            for q in model._lora_params:
                q.grad = None
            feats = teacher_fwd()
            res = model(timestep=tok, crepa_teacher_features=feats, **fwd)
            (((res.sample.float() - target.float()) ** 2).mean() - 0.5 * res.crepa_similarity).backward()

        def step_plain():
            for q in plain._lora_params:
                q.grad = None
            ((plain(timestep=tok, **fwd).sample.float() - target.float()) ** 2).mean().backward()

        r = timed({"self_flow": step_self_flow, "plain": step_plain}, args.steps)
        print(json.dumps({"measurement": "sd3_lora_forward_backward", "arch": arch, "student_block": args.student, "teacher_block": args.teacher,
                          "self_flow_ms": round(r["self_flow"][0], 2), "self_flow_spread_ms": round(r["self_flow"][1], 2), "plain_tokenwise_ms": round(r["plain"][0], 2),
                          "plain_spread_ms": round(r["plain"][1], 2), "delta_ms": round(r["self_flow"][0] - r["plain"][0], 2)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Self-Transcendence at SD3-Medium shapes on the MI355X: the four kernels of csrc/self_transcendence.hip, the tap, and the step of both stages.

    python tools/self_transcendence_bench.py [--steps 4] [--batch 3] [--student 8] [--teacher 20] [--hidden 2048] [--only kernels|tap|step]
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python tools/self_transcendence_bench.py --only tap --steps 2        (no counters in the same run)

SD3-Medium: 24 joint blocks, D 1536, LoRA r128, 1024^2 (latents [B, 16, 128, 128], 4096 image + 231 text tokens), projector_hidden_dim 2048, eager, through the
component.  One JSON line per measurement, device events around windows that end in a synchronise, medians over `--steps` windows behind warm-up windows,
alternating where two things are compared:

  kernels   st_fold (both stages), st_vae_loss, st_cfg_loss, st_wgrad (the largest Linear), st_dx_add, each alone, with its algorithmic bytes (bf16 2 bytes, fp32 4)
            and the rate they give:  fold 8 (Hp D + Hp^2 + P3 Hp);  vae_loss 6 M P (pred read and written, the target read);  cfg_loss 8 M D (pred read and
            written, c and u read);  wgrad 6 R Cc;  dx_add 6 M D.
  tap       SelfTranscendenceTap.tap and .backward alone at M = batch * 4096 rows, both stages.
  step      stage `vae`: training forward with the tap + backward;  stage `self`: the teacher's ONE no-grad forward at batch 2B ending behind the teacher block, then
            the same;  against the plain LoRA forward + backward (no optimizer in any of the three)."""
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
TMIN, TMAX, CFG = 0.4, 0.7, 30.0


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


def bench_kernels(dev, B: int, Hp: int, steps: int):
    from simpletuner_amd import ops
    D, S, P, reps = 1536, 4096, 64, 20          # each window runs the kernel `reps` times: a single launch of a few microseconds measures the clock
    M = B * S
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s, dt=BF16: torch.randn(*s, generator=g, device=dev).to(dt)
    params = [rn(Hp, D, dt=F32), rn(Hp, dt=F32), rn(Hp, Hp, dt=F32), rn(Hp, dt=F32), rn(D, Hp, dt=F32), rn(D, dt=F32)]
    e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)
    outs = {P3: [e(Hp, D), e(D, Hp), e(Hp), e(Hp, Hp), e(Hp, Hp), e(Hp), e(D, Hp), e(Hp, P3), e(D)] for P3 in (P, D)}
    sig = torch.tensor([0.55, 0.9, 0.6][:B] + [0.5] * max(0, B - 3), device=dev)
    per, st, s = torch.empty(B, dtype=F32, device=dev), torch.empty(3, dtype=F32, device=dev), torch.tensor([0.37], device=dev)
    pred_v, target = rn(M, P), rn(B, 16, 128, 128)
    pred_c, cap = rn(M, D), rn(2 * B, S, D)
    Pm, db, gW, gb = rn(Hp, Hp), rn(Hp, dt=F32), torch.zeros(Hp, Hp, dtype=F32, device=dev), torch.zeros(Hp, dtype=F32, device=dev)
    addend, dx = rn(M, D), torch.zeros(B, S, D, dtype=BF16, device=dev)
    loop = lambda fn: (lambda: [fn() for _ in range(reps)])
    fns = {"st_fold_vae": loop(lambda: ops.st_fold(*params, *outs[P])), "st_fold_self": loop(lambda: ops.st_fold(*params, *outs[D])),
           "st_vae_loss": loop(lambda: ops.st_vae_loss(pred_v, target, (64, 64), sig, TMIN, TMAX, per, st)),
           "st_cfg_loss": loop(lambda: ops.st_cfg_loss(pred_c, cap, CFG, sig, TMIN, TMAX, per, st)),
           "st_wgrad": loop(lambda: ops.st_wgrad(Pm, db, s, gW, gb)), "st_dx_add": loop(lambda: ops.st_dx_add(addend, s, dx))}
    nbytes = {"st_fold_vae": 8 * (Hp * D + Hp * Hp + P * Hp), "st_fold_self": 8 * (Hp * D + Hp * Hp + D * Hp), "st_vae_loss": 6 * M * P, "st_cfg_loss": 8 * M * D,
              "st_wgrad": 6 * Hp * Hp, "st_dx_add": 6 * M * D}
    r = timed(fns, max(steps, 10), warm=3)
    for k in fns:
        us = r[k][0] * 1e3 / reps
        print(json.dumps({"measurement": k, "batch": B, "M": M, "D": D, "Hp": Hp, "P": P, "us_per_launch": round(us, 2), "spread_us": round(r[k][1] * 1e3 / reps, 2),
                          "algorithmic_bytes": nbytes[k], "TBps": round(nbytes[k] / (us * 1e-6) / 1e12, 3), "launches_per_window": reps}), flush=True)


def build(dev, stage, student: int, teacher: int, Hp: int):
    from simpletuner_amd.sd3.transformer import SD3Transformer2DModel
    m = SD3Transformer2DModel(device=dev, **ARCH)
    m.init_synthetic(5)
    if stage is not None:
        m.set_self_transcendence(stage, student, teacher if stage == "self" else None, Hp, TMIN, TMAX, CFG)
    m.add_lora_adapter(rank=128, seed=12, init_b_std=0.02)
    m.prepare_for_training()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--student", type=int, default=8)
    ap.add_argument("--teacher", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--only", choices=("kernels", "tap", "step"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("self_transcendence_bench: needs an MI355X (no CPU path, nothing is measured without the device)")
    dev = torch.device("cuda:0")
    want = lambda k: args.only in (None, k)
    B, Si, D, Hp = args.batch, 4096, 1536, args.hidden
    if want("kernels"):
        bench_kernels(dev, B, Hp, args.steps)
    if args.only == "kernels":
        return
    from simpletuner_amd.engine import SelfTranscendenceTap
    from tests import parity_utils as PU
    _, devt = PU.make_inputs(B, 128, 128, 231, 4096, 2048, dev, seed=5)
    lat, prompt, pooled = devt["latents"], devt["prompt"], devt["pooled"]
    g = torch.Generator(device=dev).manual_seed(2)
    t = torch.rand(B, generator=g, device=dev) * 300 + 400
    sig = t / 1000.0
    target = torch.randn(lat.shape, generator=g, device=dev).to(BF16)
    neg_prompt, neg_pooled = torch.zeros_like(prompt), torch.zeros_like(pooled)
    fwd = dict(hidden_states=lat, encoder_hidden_states=prompt, pooled_projections=pooled)
    arch = f"SD3-Medium, 24 joint blocks, D 1536, LoRA r128, batch {B}, 4096 + 231 tokens, projector_hidden_dim {Hp}, eager"
    models = {stage: build(dev, stage, args.student, args.teacher, Hp) for stage in ("vae", "self")}
    snapshot = models["self"].lora_flat.clone()

    def teacher_fwd():
        m = models["self"]
        two = lambda a, b: torch.cat([a, b], dim=0)
        with torch.no_grad(), m.teacher_values(snapshot):
            return m(hidden_states=two(lat, lat), encoder_hidden_states=two(prompt, neg_prompt), pooled_projections=two(pooled, neg_pooled), timestep=two(t, t),
                     crepa_capture_block_index=args.teacher).crepa_hidden_states

    if want("tap"):
        h = torch.randn(B, Si, D, generator=g, device=dev).to(BF16)
        cap = torch.randn(2 * B, Si, D, generator=g, device=dev).to(BF16)
        dx = torch.zeros(B, Si, D, dtype=BF16, device=dev)
        dg = torch.tensor(0.5, device=dev)
        for stage, tgt in (("vae", target), ("self", cap)):
            head, taps = models[stage]._st, []

            def tap_fwd():
                tp = SelfTranscendenceTap(head, stage, tgt, sig, TMIN, TMAX, CFG)
                tp.tap(head.block, h)
                taps.append(tp)

            def tap_bwd():
                taps.pop().backward(dg, dx)

            r = timed({"tap": tap_fwd, "backward": tap_bwd}, args.steps)
            print(json.dumps({"measurement": "tap_path", "stage": stage, "M": B * Si, "D": D, "Hp": Hp, "tap_ms": round(r["tap"][0], 3), "tap_spread_ms": round(r["tap"][1], 3),
                              "backward_ms": round(r["backward"][0], 3), "backward_spread_ms": round(r["backward"][1], 3)}), flush=True)
    if want("step"):
        plain = build(dev, None, args.student, args.teacher, Hp)

        def step(stage):
            m = models[stage]

            def run():
                for q in m._lora_params:
                    q.grad = None
                tgt = target if stage == "vae" else teacher_fwd()
                res = m(timestep=t, self_transcendence_target=tgt, self_transcendence_sigmas=sig, **fwd)
                (((res.sample.float() - target.float()) ** 2).mean() + 0.5 * res.self_transcendence_guide_loss).backward()
            return run

        def step_plain():
            for q in plain._lora_params:
                q.grad = None
            ((plain(timestep=t, **fwd).sample.float() - target.float()) ** 2).mean().backward()

        r = timed({"vae": step("vae"), "self": step("self"), "plain": step_plain, "teacher_2B": teacher_fwd}, args.steps)
        print(json.dumps({"measurement": "sd3_lora_forward_backward", "arch": arch, "student_block": args.student, "teacher_block": args.teacher,
                          **{f"{k}_ms": round(v[0], 2) for k, v in r.items()}, **{f"{k}_spread_ms": round(v[1], 2) for k, v in r.items()},
                          "vae_delta_ms": round(r["vae"][0] - r["plain"][0], 2), "self_delta_ms": round(r["self"][0] - r["plain"][0], 2)}), flush=True)


if __name__ == "__main__":
    main()

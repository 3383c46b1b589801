#!/usr/bin/env python3
"""Time one Adafactor step (st355_adafactor_step: stats, factors, unorm, coef, apply) on a synthetic arena through the C ABI, next to the AdamW launch
(st355_adamw_ema_step*, no EMA) and — on bf16 arenas — the AdamWBF16 launch (st355_adamw_bf16_sr_step), in one process on one MI355X.

    python tools/adafactor_bench.py [--arena sd3-full|flux-full|flux-lora|all] [--iters 10] [--rounds 3] [--rank 32] [--memory]
    python tools/adafactor_bench.py --sd3-step-memory torch-adafactor|adamw_bf16 [--batch 8]

Three arenas, each with the tensor shapes of the model's checkpoint (weights, biases, norm weights, the 2 x 2 patch embedding), 16-byte aligned starts:
the SD3-Medium full fine-tune arena (bf16), the Flux.1-dev full-rank arena (bf16) and the Flux LoRA rank-32 adapter arena (fp32).  The optimizers
alternate call by call; every call is timed with its own pair of device events; one "median" is the median of --iters timed calls after warm-up and
--rounds medians are taken, so the run-to-run spread stands next to the number.  One JSON line per measurement: bytes per parameter as read off the
operand lists (adafactor.hip: 6 arena elements per parameter, i.e. 12 B bf16 / 24 B fp32; optim.hip), GB/s = those bytes over the median of the
medians, and the state bytes each optimizer keeps.  --memory adds torch.cuda.max_memory_allocated of one optimizer step per optimizer (state included).
--sd3-step-memory builds the SD3-Medium full fine-tune + EMA of `bench.py --model sd3 --full-finetune` (24 joint blocks, 1024^2, the benchmark batch) under the named
optimizer, runs two train steps and prints torch.cuda.max_memory_allocated: one process per optimizer, so the peaks do not mix."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.lion_step_bench import HBM_BYTES_PER_S, measure  # noqa: E402
from tools.muon_step_bench import flux_adapter_shapes  # noqa: E402


def _linear(out_f, in_f, bias=True):
    return [(out_f, in_f)] + ([(out_f,)] if bias else [])


def sd3_medium_shapes(D=1536, layers=24, ctx=4096, pooled=2048, latent_c=16, heads_dim=64):
    """the tensors of an SD3-Medium transformer checkpoint (diffusers SD3Transformer2DModel), fused buffers as the separate tensors it saves"""
    s = [(D, latent_c, 2, 2), (D,)] + _linear(D, ctx)                                     # pos_embed.proj, context_embedder
    s += _linear(D, 256) + _linear(D, D) + _linear(D, pooled) + _linear(D, D)              # time_text_embed
    for i in range(layers):
        last = i == layers - 1
        s += _linear(6 * D, D) + _linear((2 if last else 6) * D, D)                        # norm1.linear, norm1_context.linear
        s += _linear(D, D) * 3 + _linear(D, D) * 3 + _linear(D, D)                         # to_q/k/v, add_q/k/v_proj, to_out.0
        s += _linear(4 * D, D) + _linear(D, 4 * D)                                         # ff
        if not last:
            s += _linear(D, D) + _linear(4 * D, D) + _linear(D, 4 * D)                     # to_add_out, ff_context
    return s + _linear(2 * D, D) + _linear(4 * latent_c, D)                                # norm_out.linear, proj_out


def flux_dev_shapes(D=3072, double=19, single=38, ctx=4096, pooled=768, hd=128):
    """the tensors of a Flux.1-dev transformer checkpoint (diffusers FluxTransformer2DModel)"""
    s = _linear(D, 64) + _linear(D, ctx)                                                   # x_embedder, context_embedder
    s += (_linear(D, 256) + _linear(D, D)) * 2 + _linear(D, pooled) + _linear(D, D)        # timestep, guidance, text embedders
    for _ in range(double):
        s += _linear(6 * D, D) * 2 + _linear(D, D) * 8 + [(hd,)] * 4                       # norm1 / norm1_context, q k v out + added, the four RMSNorm weights
        s += (_linear(4 * D, D) + _linear(D, 4 * D)) * 2                                   # ff, ff_context
    for _ in range(single):
        s += _linear(3 * D, D) + _linear(4 * D, D) + _linear(D, 5 * D) + _linear(D, D) * 3 + [(hd,)] * 2
    return s + _linear(2 * D, D) + _linear(64, D)


def numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


def offsets_of(shapes, elem_bytes):
    per16 = 16 // elem_bytes
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        off += (numel(s) + per16 - 1) // per16 * per16
    return offs, off


def sd3_step_memory(optimizer, batch):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    dev = torch.device("cuda:0")
    cfg = default_config(model_family="sd3", train_batch_size=batch, seed=42, model_type="full", use_ema=True, optimizer=optimizer, learning_rate=1e-5)
    acc = St355Accelerator(dev)
    plugin = SD3(cfg, acc)
    plugin.load_model(sample_size=128, num_layers=24, num_attention_heads=24, attention_head_dim=64, caption_projection_dim=1536, pooled_projection_dim=2048,
                      pos_embed_max_size=192)
    plugin.enable_full_finetune()
    trainer = Trainer(cfg, plugin, acc)
    gen = torch.Generator(device=dev).manual_seed(42)
    b = {"latent_batch": torch.randn(batch, 16, 128, 128, device=dev, generator=gen).to(torch.bfloat16),
         "prompt_embeds": torch.randn(batch, 231, 4096, device=dev, generator=gen).to(torch.bfloat16),
         "add_text_embeds": torch.randn(batch, 2048, device=dev, generator=gen).to(torch.bfloat16)}
    torch.cuda.reset_peak_memory_stats()
    for _ in range(2):
        trainer.train_step(dict(b))
    torch.cuda.synchronize()
    n = sum(p.numel() for p in trainer.params)
    opt_state = sum(t.numel() * t.element_size() for st in trainer.optimizer._flat.values() for t in st.values() if torch.is_tensor(t) and t.is_cuda)
    print(json.dumps({"what": "sd3-medium full fine-tune + EMA, one train step", "optimizer": optimizer, "batch": batch, "params": n,
                      "max_memory_allocated_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "memory_allocated_after_GiB": round(torch.cuda.memory_allocated() / 2 ** 30, 3),
                      "optimizer_state_GiB": round(opt_state / 2 ** 30, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sd3-step-memory", default=None, choices=("torch-adafactor", "adamw_bf16"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--arena", default="all", choices=("sd3-full", "flux-full", "flux-lora", "all"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--memory", action="store_true")
    args = ap.parse_args()
    if args.sd3_step_memory:
        return sd3_step_memory(args.sd3_step_memory, args.batch)
    from simpletuner_amd import ops
    dev = torch.device("cuda:0")
    arenas = {"sd3-full": ("sd3-medium full fine-tune arena (bf16)", torch.bfloat16, sd3_medium_shapes()),
              "flux-full": ("flux.1-dev full-rank arena (bf16)", torch.bfloat16, flux_dev_shapes()),
              "flux-lora": ("flux lora r%d adapter arena (fp32)" % args.rank, torch.float32, flux_adapter_shapes("all", args.rank))}
    for key, (name, dtype, shapes) in arenas.items():
        if args.arena not in ("all", key):
            continue
        bf = dtype == torch.bfloat16
        esz = 2 if bf else 4
        offs, n = offsets_of(shapes, esz)
        n = (n + 7) // 8 * 8
        params = sum(numel(s) for s in shapes)
        torch.cuda.reset_peak_memory_stats()
        p = torch.empty(n, dtype=dtype, device=dev).normal_(0.0, 0.05)
        g = torch.empty(n, dtype=dtype, device=dev).normal_(0.0, 1e-2)
        base = torch.cuda.max_memory_allocated()
        plan = ops.AdafactorPlan(offs, shapes, dev)
        rv, cv, var = (torch.zeros(k, dtype=torch.float32, device=dev) for k in (plan.rv_len, plan.cv_len, plan.var_len))
        step = [0]

        def adafactor():
            step[0] += 1
            ops.adafactor_step(plan, p, g, rv, cv, var, step[0], 1e-5, weight_decay=1e-2)

        adafactor()
        torch.cuda.synchronize()
        fns = {"st355_adafactor_step": adafactor}
        state = {"st355_adafactor_step": 4 * (plan.rv_len + plan.cv_len + plan.var_len) + 4 * plan.ws_floats}
        per_param = {"st355_adafactor_step": 6 * esz}
        peak = {"st355_adafactor_step": torch.cuda.max_memory_allocated() - base}
        adam_m = adam_v = None
        try:
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            adam_m, adam_v = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
            astep = [0]

            def adam():
                astep[0] += 1
                ops.adamw_ema_step(p, g, adam_m, adam_v, astep[0], 1e-5, 0.9, 0.999, 1e-8, 1e-2)

            adam()
            torch.cuda.synchronize()
            nm = "st355_adamw_ema_step" + ("_bf16" if bf else "")
            fns[nm], state[nm], per_param[nm], peak[nm] = adam, 8 * n, 22 if bf else 28, torch.cuda.max_memory_allocated() - before
        except torch.OutOfMemoryError:
            print(json.dumps({"arena": name, "what": "st355_adamw_ema_step", "skipped": "fp32 moments do not fit next to the arena"}), flush=True)
        res = measure(fns, args.iters, args.rounds)
        del adam_m, adam_v
        fns = {}
        if bf:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            m16, v16, shift = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(3))
            seg_end = torch.tensor([n], dtype=torch.int64, device=dev)
            seg_decay = torch.zeros(1, dtype=torch.float32, device=dev)
            bstep = [0]

            def adam16():
                bstep[0] += 1
                ops.adamw_bf16_sr_step(p, g, m16, v16, shift, bstep[0], 1e-5, 0.9, 0.999, 1e-6, seg_end=seg_end, seg_decay=seg_decay, seed=0, offset=4 * n * bstep[0])

            adam16()
            torch.cuda.synchronize()
            nm = "st355_adamw_bf16_sr_step"
            state[nm], per_param[nm], peak[nm] = 6 * n, 16, torch.cuda.max_memory_allocated() - before
            res.update(measure({nm: adam16, "st355_adafactor_step (beside adamw_bf16)": adafactor}, args.iters, args.rounds))
            per_param["st355_adafactor_step (beside adamw_bf16)"] = 6 * esz
            state["st355_adafactor_step (beside adamw_bf16)"] = state["st355_adafactor_step"]
            del m16, v16, shift
        for k, meds in res.items():
            ms = statistics.median(meds)
            rate = per_param[k] * params / (ms * 1e-3)
            line = {"arena": name, "tensors": len(shapes), "params": params, "what": k, "bytes_per_param": per_param[k], "ms": round(ms, 4),
                    "ms_medians_min": round(min(meds), 4), "ms_medians_max": round(max(meds), 4), "rounds": args.rounds, "iters": args.iters,
                    "GB_per_s": round(rate / 1e9, 1), "fraction_of_hbm_8TBps": round(rate / HBM_BYTES_PER_S, 4), "state_bytes": state[k]}
            if args.memory and k in peak:
                line["peak_bytes_beyond_p_and_g"] = peak[k]
            print(json.dumps(line), flush=True)
        del p, g, rv, cv, var, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""`sampling.sample_images` on SD3 and Flux engines of real width and reduced depth (random weights, 128 x 128 latents, 4 Euler steps, no decode) with
attention_mechanism unset and set to sageattention, alternated, on one MI355X: host wall time of the whole call between device synchronisations, one warm-up
pair, then the median and (min, max) of 3 calls per setting, and the rel-L2 between the two settings' final latents.

    python tools/attn_sage_sampling_bench.py"""
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from simpletuner_amd.sampling import sample_images
from simpletuner_amd.training.trainer import St355Accelerator, default_config

dev = torch.device("cuda:0")
STEPS, REPS = 4, 3


def timed(plugin, pe, pool):
    g = torch.Generator(device=dev).manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        x = sample_images(plugin, pe, pool, 128, 128, num_inference_steps=STEPS, decode=False, generator=g)
    torch.cuda.synchronize()
    assert torch.isfinite(x.float()).all()
    return (time.perf_counter() - t0) * 1e3, x


def run(name, plugin, s_txt, pooled_dim):
    g = torch.Generator().manual_seed(0)
    pe, pool = torch.randn(1, s_txt, 4096, generator=g), torch.randn(1, pooled_dim, generator=g)
    t = {None: [], "sageattention": []}
    outs = {}
    for rep in range(REPS + 1):
        for mech in t:
            plugin.config.attention_mechanism = mech
            ms, outs[mech] = timed(plugin, pe, pool)
            if rep:
                t[mech].append(ms)
    a, b = outs[None].float(), outs["sageattention"].float()
    print(name, {str(k): (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in t.items()},
          "latents rel-L2 set vs unset %.3e" % float((a - b).norm() / a.norm()), flush=True)


from simpletuner_amd.sd3.model import SD3
p = SD3(default_config(model_family="sd3", seed=1, flow_schedule_shift=3.0), St355Accelerator(dev))
p.load_model(sample_size=128, num_layers=6, num_attention_heads=24, attention_head_dim=64, joint_attention_dim=4096, caption_projection_dim=1536,
             pooled_projection_dim=2048, pos_embed_max_size=192, qk_norm=None, dual_attention_layers=())
run("sd3 D1536 H24 d64, 6 blocks, S 4096+154, 4 steps", p, 154, 2048)
del p
from simpletuner_amd.flux.model import Flux
p = Flux(default_config(model_family="flux", seed=1, flow_schedule_shift=3.0), St355Accelerator(dev))
p.load_model(num_layers=2, num_single_layers=4, num_attention_heads=24, attention_head_dim=128, joint_attention_dim=4096, pooled_projection_dim=768,
             guidance_embeds=True, in_channels=64)
run("flux D3072 H24 d128, 2 double + 4 single blocks, S 4096+512, 4 steps", p, 512, 768)

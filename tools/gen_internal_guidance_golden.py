#!/usr/bin/env python3
"""Generate tests/golden/internal_guidance_vectors.pt by EXECUTING THE REFERENCE'S Internal Guidance module (helpers/training/internal_guidance.py, pure torch) on
the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path, at generation time only; nothing of it is copied here and the tests read only the
recorded tensors, numbers and messages.  Recorded (B = 2, 5 x 7 token grid = latent 10 x 14, D = 64, N = 64, fp32, seeded non-zero gamma, beta, W, b):

  case            hidden states, target, the four parameters, the weight; the head's tokens and the unpatchified prediction; `compute_loss`'s loss and logs against a
                  stand-in foundation whose loss() is the MSE; autograd.grad of the loss with respect to the hidden states and the four parameters
  constant_row    the same with one constant row (xhat = 0)
  offset_row      the same with one row of large offset (mean 64, a bf16-representable spread)
  guided          `guided_prediction` at s = 1.5
  patch_shapes    the patch shape `infer_patch_shape` picks for the even latent grids 8x8, 4x16, 16x4, 6x10, 2x2, 2x8 (and 10x14)
  features        `infer_internal_guidance_output_features` for an SD3 config (in_channels 16, patch_size 2)
  default_blocks  the default block index for 3, 24 and 38 blocks
  errors          the ValueError texts
  loader          `attach_internal_guidance_head_from_state_dict` and `internal_guidance_lora_state_dict` on a dict written in this project's key layout

    python tools/gen_internal_guidance_golden.py <SimpleTuner checkout>      (writes tests/golden/internal_guidance_vectors.pt)
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "internal_guidance_vectors.pt"
B, GH, GW, D, N, C = 2, 5, 7, 64, 64, 16
PREFIX = "transformer.internal_guidance_head."


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_internal_guidance", ref / "helpers/training/internal_guidance.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.config = SimpleNamespace(in_channels=C, out_channels=C, patch_size=2)
        self.anchor = torch.nn.Parameter(torch.zeros(1))


class _Foundation:
    """stand-in for the model foundation: the diffusion target from the batch, loss() = MSE"""
    NAME = "stand-in"

    def __init__(self, model):
        self.model = model

    def get_prediction_target(self, batch):
        return batch["target"]

    def get_trained_component(self, unwrap_model=False):
        return self.model

    def unwrap_model(self, model=None):
        return model

    def loss(self, batch, model_output, apply_conditioning_mask=True):
        return ((model_output["model_prediction"].float() - batch["target"].float()) ** 2).mean()


def _err(fn, kind=ValueError):
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"expected a {kind.__name__}")


def _cfg(**kw):
    return SimpleNamespace(internal_guidance_enabled=True, **kw)


def _regulariser(mod, params, weight, block, n_blocks):
    acc = SimpleNamespace(device=torch.device("cpu"))
    reg = mod.InternalGuidanceRegularizer(_cfg(internal_guidance_loss_weight=weight, internal_guidance_block_index=block), acc, D, N, n_blocks)
    model = _Model()
    reg.attach_to_model(model, torch.float32)
    with torch.no_grad():
        reg.head.norm.weight.copy_(params["gamma"]); reg.head.norm.bias.copy_(params["beta"])
        reg.head.proj.weight.copy_(params["W"]); reg.head.proj.bias.copy_(params["b"])
    return reg, model


def _run(mod, params, hidden, target, weight, block=1, n_blocks=3):
    reg, model = _regulariser(mod, params, weight, block, n_blocks)
    h = hidden.clone().requires_grad_(True)
    tokens = reg.head(h)
    pred = reg.predict(h, target, model.config)
    loss, logs = reg.compute_loss({f"layer_{block}": h}, {"target": target}, _Foundation(model))
    wrt = [h, reg.head.norm.weight, reg.head.norm.bias, reg.head.proj.weight, reg.head.proj.bias]
    gh, gg, gb, gW, gbias = torch.autograd.grad(loss, wrt)
    return {"hidden": hidden, "target": target, "weight": float(weight), "block": block, "tokens": tokens.detach(), "prediction": pred.detach(), "loss": loss.detach(),
            "logs": dict(logs), "grad_hidden": gh, "grad_gamma": gg, "grad_beta": gb, "grad_W": gW, "grad_b": gbias}


def main(ref: Path):
    mod = _load(ref)
    g = torch.Generator().manual_seed(4321)
    S = GH * GW
    hidden = torch.randn(B, S, D, generator=g)
    target = torch.randn(B, C, 2 * GH, 2 * GW, generator=g)
    params = {"gamma": 1.0 + 0.25 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g),
              "W": torch.randn(N, D, generator=g) / 8.0, "b": 0.05 * torch.randn(N, generator=g)}
    out = {"shape": (B, GH, GW, D, N), "params": params}
    out["case"] = _run(mod, params, hidden, target, 0.7)
    hc = hidden.clone()
    hc[0, 3] = 0.375                                   # constant row: xhat = 0, rstd = 1 / sqrt(eps)
    out["constant_row"] = dict(_run(mod, params, hc, target, 0.7), row=(0, 3))
    ho = hidden.clone()
    ho[1, 9] = 64.0 + torch.randint(-4, 5, (D,), generator=g).float() * 0.5      # mean 64, spread of bf16-representable values (ulp 0.5 at 64)
    out["offset_row"] = dict(_run(mod, params, ho, target, 0.7), row=(1, 9))
    reg, model = _regulariser(mod, params, 0.7, 1, 3)
    final = torch.randn(B, C, 2 * GH, 2 * GW, generator=g)
    out["guided"] = {"final": final, "scale": 1.5, "result": reg.guided_prediction(final, hidden, model.config, 1.5).detach()}
    shapes = {}
    for (H, W) in ((8, 8), (4, 16), (16, 4), (6, 10), (2, 2), (2, 8), (2 * GH, 2 * GW)):
        t = torch.zeros(1, C, H, W)
        shapes[(H, W)] = tuple(mod.InternalGuidanceHead.infer_patch_shape(t, token_count=(H // 2) * (W // 2), output_features=N, preferred_patch_size=2))
    out["patch_shapes"] = shapes
    out["features"] = int(mod.infer_internal_guidance_output_features(model))
    acc = SimpleNamespace(device=torch.device("cpu"))
    out["default_blocks"] = {n: int(mod.InternalGuidanceRegularizer(_cfg(), acc, D, N, n).block_index) for n in (3, 24, 38)}
    out["default_weight"] = float(mod.InternalGuidanceRegularizer(_cfg(), acc, D, N, 3).weight)
    R = mod.InternalGuidanceRegularizer
    out["errors"] = {
        "bad_weight": _err(lambda: R(_cfg(internal_guidance_loss_weight=-0.5), acc, D, N, 3)),
        "zero_weight": _err(lambda: R(_cfg(internal_guidance_loss_weight=0), acc, D, N, 3)),
        "index_high": _err(lambda: R(_cfg(internal_guidance_block_index=3), acc, D, N, 3)),
        "index_negative": _err(lambda: R(_cfg(internal_guidance_block_index=-1), acc, D, N, 3)),
        "no_buffer": _err(lambda: reg.compute_loss(None, {"target": target}, _Foundation(model))),
        "token_mismatch": _err(lambda: reg.predict(hidden[:, :-1], target, model.config)),
        "bad_scale": _err(lambda: reg.inference_context(0.0).__enter__()),
        "no_head": _err(lambda: mod.internal_guidance_inference(_Model(), 1.5)),
        "loader_no_head": _err(lambda: mod.attach_internal_guidance_head_from_state_dict(_Model(), {"transformer.x.lora_A.weight": torch.zeros(2, 2)})),
    }
    # this project's adapter-file layout: adapter tensors + the head under transformer.internal_guidance_head.*
    sd = {"transformer.transformer_blocks.0.attn.to_q.lora_A.weight": torch.randn(4, D, generator=g),
          "transformer.transformer_blocks.0.attn.to_q.lora_B.weight": torch.randn(D, 4, generator=g),
          PREFIX + "norm.weight": params["gamma"], PREFIX + "norm.bias": params["beta"], PREFIX + "proj.weight": params["W"], PREFIX + "proj.bias": params["b"],
          PREFIX + "block_index": torch.tensor(1, dtype=torch.int64)}
    m2 = _Model()
    head = mod.attach_internal_guidance_head_from_state_dict(m2, sd)
    out["loader"] = {"state_dict": sd, "head_state": {k: v.detach().clone() for k, v in head.state_dict().items()}, "head_tokens": head(hidden).detach(),
                     "lora_keys": sorted(mod.internal_guidance_lora_state_dict(sd).keys()), "block_index": int(head.block_index.item())}
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))

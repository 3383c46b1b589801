#!/usr/bin/env python3
"""Generate tests/golden/diff2flow_vectors.pt by EXECUTING the reference's Diff2Flow code on the CPU, seeded.

Like tools/gen_scheduled_sampling_golden.py: the reference package cannot be imported as a package here, so
  * simpletuner/diff2flow/bridge.py is loaded as a file (it imports only torch);
  * ModelFoundation.loss — the Diff2Flow branch, the conditioning mask and the reductions (common.py:6217-6248, 6402-6430) — and get_flow_target (4660-4666) are
    lifted by AST and run on stand-in `self` objects.
Three runs of everything: the bridge cast to fp64, left in fp32, and cast to bf16 (`bridge.to(dtype=...)`, what a real bf16 run does).  The lifted loss promotes
its operands with `.float()`; in the fp64 run `.float()` is widened to `.double()` for the duration of the call, so that the record is the reference's expression
in fp64 throughout.  Nothing of the reference is copied into the repository; only the recorded tensors are.  The reference tree is read ONLY by this script.

    python tools/gen_diff2flow_golden.py /path/to/reference/simpletuner
"""
from __future__ import annotations

import ast
import enum
import importlib.util
import logging
import random
import sys
import types
from pathlib import Path

import torch
import torch.nn.functional as F

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "diff2flow_vectors.pt"
NS = types.SimpleNamespace
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TIMESTEPS = [0, 1, 500, 999]
DTYPES = {"fp64": F64, "fp32": F32, "bf16": BF16}


class PredictionTypes(enum.Enum):
    EPSILON = "epsilon"; V_PREDICTION = "v_prediction"; FLOW_MATCHING = "flow_matching"; SAMPLE = "sample"


def load_bridge(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_diff2flow_bridge", str(ref / "diff2flow" / "bridge.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DiffusionToFlowBridge


def lift_methods(ref: Path, names):
    tree = ast.parse((ref / "helpers/models/common.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ModelFoundation")
    picked = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in picked} == set(names)
    for n in picked:
        n.decorator_list = []
    mod = ast.Module(body=picked, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "F": F, "random": random, "PredictionTypes": PredictionTypes, "logger": logging.getLogger("ref"), "__builtins__": __builtins__}
    exec(compile(mod, "common.py", "exec"), ns)
    return [ns[n] for n in names]


class widened_float:
    """`.float()` means `.double()` inside: the reference's promotions, one precision up"""

    def __enter__(self):
        self.saved = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.saved


class unchanged:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


def scaled_linear_acp(T=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=F32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1])
    Bridge = load_bridge(ref)
    loss_fn, get_flow_target = lift_methods(ref, ["loss", "get_flow_target"])
    acp = scaled_linear_acp()
    G = {"_cite": "simpletuner/diff2flow/bridge.py; simpletuner/helpers/models/common.py:4558-4574, 4660-4666, 6217-6248, 6402-6430",
         "schedule": dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, num_train_timesteps=1000), "alphas_cumprod": acp, "timesteps": TIMESTEPS}
    base = Bridge(alphas_cumprod=acp)
    G["tables"] = {k: getattr(base, k).clone() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                                          "sqrt_recipm1_alphas_cumprod")}
    # ---- the sigma maps ----
    all_t = torch.arange(1000)
    sig = base.timesteps_to_sigma(all_t)
    G["timesteps_to_sigma"] = sig.clone()
    mids = (sig[:-1] + sig[1:]) / 2
    grid = torch.cat([sig[::37], mids[::41], torch.tensor([0.0, 1.0, 0.5, 1e-4, 0.9999]), sig[:3], mids[:3], sig[-3:], mids[-3:]])
    G["sigma_grid"] = grid.clone()
    G["sigma_to_timesteps"] = Bridge(alphas_cumprod=acp).sigma_to_timesteps(grid.clone())
    g2 = grid[:12].reshape(4, 3).clone()
    G["sigma_grid_2d"] = g2
    G["sigma_to_timesteps_2d"] = Bridge(alphas_cumprod=acp).sigma_to_timesteps(g2.clone())
    # ---- the inputs: what a bf16 run holds ----
    g = torch.Generator().manual_seed(17)
    B, C, H, W = 4, 4, 8, 8
    lat, noise = torch.randn(B, C, H, W, generator=g).to(BF16), torch.randn(B, C, H, W, generator=g).to(BF16)
    t = torch.tensor(TIMESTEPS)
    a = acp[t].reshape(B, 1, 1, 1)
    noisy = (a.sqrt() * lat.float() + (1 - a).sqrt() * noise.float()).to(BF16)
    jitter = torch.randn(B, C, H, W, generator=g)
    cpv = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    preds = {"epsilon": (noise.float() + 0.1 * jitter).to(BF16), "v_prediction": (a.sqrt() * noise.float() - (1 - a).sqrt() * lat.float() + 0.1 * jitter).to(BF16),
             "epsilon.perfect": noise.clone()}
    G["inputs"] = dict(latents=lat, noise=noise, noisy_latents=noisy, conditioning_pixel_values=cpv, preds=preds)
    cases, flows = {}, {}
    for dname, dt in DTYPES.items():
        ctx = widened_float if dname == "fp64" else unchanged
        for pname, pred in preds.items():
            ptype = PredictionTypes.EPSILON if pname.startswith("epsilon") else PredictionTypes.V_PREDICTION
            bridge = Bridge(alphas_cumprod=acp).to(dtype=dt)
            wide = F64 if dname == "fp64" else F32
            flows[(dname, pname)] = bridge.prediction_to_flow(pred.to(wide), noisy.to(wide), t, prediction_type=ptype.value)
            for mask in (None, "mask", "segmentation"):
                cfg = NS(loss_type="l2", diff2flow_loss=True, diff2flow_enabled=True, snr_gamma=None, snr_weight=1.0, masked_loss_probability=1.0)
                self_ = NS(config=cfg, PREDICTION_TYPE=ptype, diff2flow_bridge=bridge, get_prediction_target=lambda pb: pb["noise"])
                self_.get_flow_target = lambda pb: get_flow_target(self_, pb)
                pb = {"noise": noise, "latents": lat, "noisy_latents": noisy, "timesteps": t}          # (no "flow_target": get_flow_target forms noise - latents in bf16)
                if mask:
                    pb["loss_mask_type"], pb["conditioning_pixel_values"] = mask, cpv
                p = pred.clone().to(wide).requires_grad_(True)
                per = {}
                with ctx():
                    loss = loss_fn(self_, pb, {"model_prediction": p}, True)
                    # the per-sample losses: the same call on each sample alone (batch mean of one = the sample's mean)
                    for b in range(B):
                        pb1 = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in pb.items()}
                        per[b] = loss_fn(self_, pb1, {"model_prediction": p.detach()[b:b + 1]}, True).detach()
                loss.backward()
                cases[(dname, pname, mask)] = {"loss": loss.detach(), "per_sample": torch.stack([per[b] for b in range(B)]), "grad": p.grad.clone()}
    G["cases"], G["prediction_to_flow"] = cases, flows
    # ---- the perfect-prediction floor: fp32 operands (no bf16 rounding of the noisy latents in the way), pred = the true noise, every sample at t = 999 ----
    lat32, noise32 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    t999 = torch.full((B,), 999)
    noisy32 = acp[999].sqrt() * lat32 + (1 - acp[999]).sqrt() * noise32
    floor = {"inputs": dict(latents=lat32, noise=noise32, noisy_latents=noisy32, timesteps=t999)}
    for dname in ("fp32", "bf16"):
        bridge = Bridge(alphas_cumprod=acp).to(dtype=DTYPES[dname])
        self_ = NS(config=NS(loss_type="l2", diff2flow_loss=True, diff2flow_enabled=True, snr_gamma=None, snr_weight=1.0, masked_loss_probability=1.0),
                   PREDICTION_TYPE=PredictionTypes.EPSILON, diff2flow_bridge=bridge, get_prediction_target=lambda pb: pb["noise"])
        self_.get_flow_target = lambda pb: get_flow_target(self_, pb)
        pb = {"noise": noise32, "latents": lat32, "noisy_latents": noisy32, "timesteps": t999}
        p = noise32.clone().requires_grad_(True)
        loss = loss_fn(self_, pb, {"model_prediction": p}, True)
        loss.backward()
        floor[dname] = {"loss": loss.detach(), "grad": p.grad.clone()}
    G["floor"] = floor
    torch.save(G, OUT)
    print(f"wrote {OUT}: {OUT.stat().st_size} bytes; {len(cases)} loss cases, {grid.numel()} sigma grid points")


if __name__ == "__main__":
    main()

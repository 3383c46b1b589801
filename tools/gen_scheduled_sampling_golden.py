#!/usr/bin/env python3
"""Generate tests/golden/scheduled_sampling_vectors.pt by EXECUTING the reference's scheduled-sampling code on the CPU, seeded.

Like tools/gen_golden.py: the reference package cannot be imported as a package here, so
  * helpers/scheduled_sampling/plan.py is loaded as a file (pure torch);
  * helpers/scheduled_sampling/rollout.py is loaded as a file over EMPTY stand-in modules for what it imports at module level — `skrample_adapter` (skrample is
    not installed; the flow branch calls none of it) and `simpletuner.helpers.models.common` (only the PredictionTypes enum is read) — as tools/ref_shim.py does
    for diffusers;
  * the probability ramp (the `if scheduled_sampling_max_step_offset > 0:` statement of ModelFoundation.prepare_batch, common.py:6014-6037) and
    ModelFoundation.loss / conditional_loss (common.py:6132-6166, 6217-6430) are lifted by AST and run on stand-in `self` objects.
Nothing of the reference is copied into the repository; only the recorded tensors are.  The reference tree is read ONLY by this script, never at test time.

    python tools/gen_scheduled_sampling_golden.py
"""
from __future__ import annotations

import ast
import enum
import importlib.util
import logging
import math
import random
import sys
import types
from pathlib import Path

import torch
import torch.nn.functional as F

REF = Path("/root/reference/simpletuner")
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "scheduled_sampling_vectors.pt"
NS = types.SimpleNamespace


class PredictionTypes(enum.Enum):
    EPSILON = "epsilon"; V_PREDICTION = "v_prediction"; FLOW_MATCHING = "flow_matching"; SAMPLE = "sample"


def load_file(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, str(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("simpletuner", "simpletuner.helpers", "simpletuner.helpers.models", "simpletuner.helpers.scheduled_sampling"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    common = types.ModuleType("simpletuner.helpers.models.common")
    common.PredictionTypes = PredictionTypes
    sys.modules["simpletuner.helpers.models.common"] = common
    adapter = types.ModuleType("simpletuner.helpers.scheduled_sampling.skrample_adapter")          # the empty stand-in: the flow branch uses none of it
    adapter.make_data_prediction_transform = adapter.make_sampler = adapter.make_sigma_schedule_from_ddpm = None
    sys.modules["simpletuner.helpers.scheduled_sampling.skrample_adapter"] = adapter
    plan = load_file("simpletuner.helpers.scheduled_sampling.plan", REF / "helpers/scheduled_sampling/plan.py")
    rollout = load_file("simpletuner.helpers.scheduled_sampling.rollout", REF / "helpers/scheduled_sampling/rollout.py")
    return plan, rollout


def lift_methods(names, extra_ns):
    tree = ast.parse((REF / "helpers/models/common.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ModelFoundation")
    picked = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in picked} == set(names)
    for n in picked:
        n.decorator_list = []
    mod = ast.Module(body=picked, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "math": math, "F": F, "random": random, "PredictionTypes": PredictionTypes, "logger": logging.getLogger("ref"), "__builtins__": __builtins__}
    ns.update(extra_ns)
    exec(compile(mod, "common.py", "exec"), ns)
    return [ns[n] for n in names]


def lift_ramp(recorder):
    """the statement of prepare_batch that computes the effective probability and calls build_rollout_schedule, as a function (self, state, batch, bsz)"""
    tree = ast.parse((REF / "helpers/models/common.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ModelFoundation")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "prepare_batch")
    stmt = next(n for n in ast.walk(fn) if isinstance(n, ast.If) and "scheduled_sampling_max_step_offset" in ast.unparse(n.test))
    args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ("self", "state", "batch", "bsz")], kwonlyargs=[], kw_defaults=[], defaults=[])
    wrapper = ast.FunctionDef(name="ramp", args=args, body=[stmt], decorator_list=[], type_params=[])
    mod = ast.Module(body=[wrapper], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"math": math, "build_rollout_schedule": recorder, "__builtins__": __builtins__}
    exec(compile(mod, "common.py", "exec"), ns)
    return ns["ramp"]


RAMP_SETTINGS = [
    dict(scheduled_sampling_probability=0.3),
    dict(scheduled_sampling_probability=None),
    dict(scheduled_sampling_probability=0.3, scheduled_sampling_prob_start=0.0, scheduled_sampling_prob_end=0.9, scheduled_sampling_ramp_steps=10),
    dict(scheduled_sampling_probability=0.2, scheduled_sampling_prob_start=0.1, scheduled_sampling_prob_end=0.9, scheduled_sampling_ramp_steps=10,
         scheduled_sampling_start_step=4),
    dict(scheduled_sampling_probability=0.2, scheduled_sampling_prob_start=0.1, scheduled_sampling_prob_end=0.9, scheduled_sampling_ramp_steps=8,
         scheduled_sampling_ramp_shape="cosine", scheduled_sampling_start_step=2),
    dict(scheduled_sampling_probability=0.5, scheduled_sampling_prob_start=None, scheduled_sampling_prob_end=1.0, scheduled_sampling_ramp_steps=4,
         scheduled_sampling_ramp_shape=None, scheduled_sampling_start_step=None),
    dict(scheduled_sampling_probability=1.0, scheduled_sampling_ramp_steps=0, scheduled_sampling_prob_start=0.1),
]
RAMP_STEPS = [0, 1, 3, 4, 6, 9, 10, 14, 100]

PLAN_SETTINGS = [dict(T=1000, B=6, off=4, strategy=s, prob=p, seed=11 + i) for i, (s, p) in enumerate(
    [("uniform", None), ("uniform", 1.0), ("uniform", 0.5), ("uniform", 0.0), ("biased_early", 0.7), ("biased_late", 0.7), ("biased_late", None)])]
PLAN_SETTINGS += [dict(T=1000, B=4, off=0, strategy="uniform", prob=0.5, seed=31), dict(T=50, B=5, off=30, strategy="uniform", prob=None, seed=32)]


def plan_base(T, B, seed):
    """fractional float timesteps (sigma * 1000 on this path), the last one near the top of the range so that the clamp at T - 1 acts"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, generator=g) * (T - 1)
    base[-1] = T - 1.5
    return base


def stub_predict(batch):
    """the small deterministic torch function standing in for model_predict: reads the state, the timestep and one conditioning entry of the batch-1 slice"""
    x, t, enc = batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"]
    assert x.shape[0] == 1 and t.shape[0] == 1 and enc.shape[0] == 1
    pred = 0.5 * torch.tanh(x) + torch.sin(t.float() / 100.0).view(1, 1, 1, 1) * enc.float().mean() + 0.1 * x.flip(-1)
    return {"model_prediction": pred.to(x.dtype)}


STUB_SOURCE = "0.5 * tanh(x) + sin(t / 100) * mean(enc) + 0.1 * flip(x, -1)"


def gen_rollout(rollout):
    out = {}
    g = torch.Generator().manual_seed(5)
    B, shape = 4, (4, 4, 6)
    for name, sched in (("table", NS(config=NS(num_train_timesteps=1000), sigmas=torch.linspace(1.0, 0.001, 1000) ** 1.5)), ("no_table", NS(config=NS(num_train_timesteps=1000)))):
        for reflex in (True, False):
            lat, noise = torch.randn(B, *shape, generator=g), torch.randn(B, *shape, generator=g)
            sig = torch.tensor([0.3127, 0.5004, 0.9981, 0.0012])
            t = sig * 1000.0
            s4 = sig.view(B, 1, 1, 1)
            batch = {"latents": lat, "noise": noise, "input_noise": noise, "noisy_latents": (1 - s4) * lat + s4 * noise, "timesteps": t.clone(), "sigmas": s4.clone(),
                     "encoder_hidden_states": torch.randn(B, 3, 5, generator=g)}
            base = t.long()
            offs = torch.tensor([0, 1, 3, 2])
            plan = NS(target_timesteps=base, source_timesteps=torch.clamp(base + offs, max=999), rollout_steps=offs)          # sample 2: 998 + 3 clamps to 999; sample 3: t = 1
            inputs = {k: v.clone() for k, v in batch.items()}
            batch["scheduled_sampling_plan"] = plan
            model = NS(model_predict=lambda prepared_batch: stub_predict(prepared_batch), PREDICTION_TYPE=PredictionTypes.FLOW_MATCHING)
            with torch.no_grad():
                res = rollout.apply_scheduled_sampling_rollout(model, batch, sched, NS(scheduled_sampling_reflexflow=reflex, controlnet=False))
            rec = {"inputs": inputs, "plan": (plan.target_timesteps, plan.source_timesteps, plan.rollout_steps), "sigmas_table": getattr(sched, "sigmas", None),
                   "noisy_latents": res["noisy_latents"], "timesteps": res["timesteps"], "sigmas": res["sigmas"],
                   "clean": res.get("_reflexflow_clean_pred"), "biased": res.get("_reflexflow_biased_pred")}
            out[f"{name}.reflex{int(reflex)}"] = rec
    return out


def gen_loss(loss_fn, cond_loss):
    out = {}
    g = torch.Generator().manual_seed(9)
    B, C, H, W = 3, 4, 4, 6
    rn = lambda: torch.randn(B, C, H, W, generator=g)
    pred, target, noisy, latents, clean, biased = rn(), rn(), rn(), rn(), rn(), rn()
    biased[1] = clean[1]                                  # a sample that was not rolled: e = 0
    cpv = torch.rand(B, 3, 8, 12, generator=g) * 2 - 1      # conditioning_pixel_values in [-1, 1], area-resized to the latent grid by the reference
    out["inputs"] = dict(pred=pred, target=target, noisy=noisy, latents=latents, clean=clean, biased=biased, conditioning_pixel_values=cpv)
    cases = {}
    params = [dict(), dict(alpha=0.0), dict(alpha=None), dict(beta1=0.0), dict(beta1=None), dict(beta2=0.0), dict(beta2=None), dict(alpha=0.5, beta1=2.0, beta2=0.25)]
    for lt in ("l2", "huber", "smooth_l1"):
        for mask in (False, True):
            for cached in (True, False):
                for pi, kw in enumerate(params):
                    cfg = NS(loss_type=lt, huber_schedule="constant", huber_c=0.1, scheduled_sampling_reflexflow=True, diff2flow_loss=False, diff2flow_enabled=False,
                             snr_gamma=None, masked_loss_probability=1.0)
                    for k, v in kw.items():
                        setattr(cfg, f"scheduled_sampling_reflexflow_{k}", v)
                    self_ = NS(config=cfg, PREDICTION_TYPE=PredictionTypes.FLOW_MATCHING, diff2flow_bridge=None, get_prediction_target=lambda pb: pb["target"])
                    self_.conditional_loss = lambda *a, **k: cond_loss(self_, *a, **k)
                    pb = {"target": target, "noisy_latents": noisy, "latents": latents, "timesteps": torch.full((B,), 500.0)}
                    if cached:
                        pb["_reflexflow_clean_pred"], pb["_reflexflow_biased_pred"] = clean, biased
                    if mask:
                        pb["loss_mask_type"], pb["conditioning_pixel_values"] = "mask", cpv
                    p = pred.clone().requires_grad_(True)
                    loss = loss_fn(self_, pb, {"model_prediction": p}, True)
                    loss.backward()
                    cases[(lt, mask, cached, pi)] = {"params": kw, "loss": loss.detach(), "grad": p.grad.clone()}
    out["cases"], out["params"] = cases, params
    # the flag alone, no plan and no caches: the ADR term is present (covered above by cached=False)
    return out


def main():
    torch.manual_seed(0)
    plan, rollout = load_reference()
    G = {"_cite": "simpletuner/helpers/scheduled_sampling/plan.py; rollout.py:54-199; simpletuner/helpers/models/common.py:6013-6037, 6132-6166, 6217-6430",
         "stub_model": STUB_SOURCE}
    # ---- ramp ----
    seen = {}
    ramp = lift_ramp(lambda **kw: seen.update(kw) or "plan")
    rows = []
    for si, st in enumerate(RAMP_SETTINGS):
        for step in RAMP_STEPS + [None]:
            cfg = NS(scheduled_sampling_max_step_offset=3, **st)
            self_ = NS(config=cfg, noise_schedule=NS(config=NS(num_train_timesteps=1000)), accelerator=NS(device="cpu"))
            seen.clear()
            batch = {"timesteps": torch.zeros(2)}
            ramp(self_, {"global_step": step} if step is not None else {}, batch, 2)
            assert batch["scheduled_sampling_plan"] == "plan"
            rows.append((si, step, float(seen["apply_probability"])))
    G["ramp"] = {"settings": RAMP_SETTINGS, "rows": rows}
    # ---- plan ----
    plans = []
    for st in PLAN_SETTINGS:
        base = plan_base(st["T"], st["B"], st["seed"])
        torch.manual_seed(st["seed"])
        p = plan.build_rollout_schedule(num_train_timesteps=st["T"], batch_size=st["B"], max_step_offset=st["off"], device="cpu", base_timesteps=base,
                                        strategy=st["strategy"], apply_probability=st["prob"])
        plans.append({"settings": st, "base": base, "target": p.target_timesteps, "source": p.source_timesteps, "steps": p.rollout_steps})
    G["plan"] = plans
    # ---- rollout ----
    G["rollout"] = gen_rollout(rollout)
    # ---- loss ----
    loss_fn, cond_loss = lift_methods(["loss", "conditional_loss"], {"compute_snr": None})
    G["loss"] = gen_loss(loss_fn, cond_loss)
    torch.save(G, OUT)
    print(f"wrote {OUT}: {OUT.stat().st_size} bytes; {len(rows)} ramp rows, {len(plans)} plans, {len(G['rollout'])} rollouts, {len(G['loss']['cases'])} loss cases")


if __name__ == "__main__":
    main()

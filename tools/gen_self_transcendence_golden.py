#!/usr/bin/env python3
"""Generate tests/golden/self_transcendence_vectors.pt by EXECUTING the reference's SelfTranscendenceDistiller on the CPU, seeded.

Like tools/gen_flow_dpo_golden.py: the reference package cannot be imported as a package here, so helpers/distillation/common.py (DistillationBase; pure torch) and
helpers/distillation/self_transcendence/distiller.py are loaded as files over stand-in modules for what they import at module level —
`simpletuner.helpers.models.common` (only the ModelTypes / PredictionTypes enums are read), `...data_backend.dataset_types` (only names handed to the registry) and
`...distillation.registry` (a register() that does nothing).  The model is a stub: a trained component that holds the reference's own projector module, a
`model_predict` that returns a seeded hidden-state buffer (the conditional rows for the batch's own embeddings, the unconditional rows for the negative ones) and
`get_prediction_target` = noise - latents.  Nothing of the reference is copied into the repository; only inputs and recorded outputs are.  The reference tree is read
ONLY by this script, never at test time.

    python tools/gen_self_transcendence_golden.py
"""
from __future__ import annotations

import enum
import importlib.util
import sys
import types
from pathlib import Path

import torch

REF = Path("/root/reference/simpletuner")
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "self_transcendence_vectors.pt"
NS = types.SimpleNamespace
F32, F64 = torch.float32, torch.float64
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")


class PredictionTypes(enum.Enum):
    EPSILON = "epsilon"; V_PREDICTION = "v_prediction"; FLOW_MATCHING = "flow_matching"; SAMPLE = "sample"; AUTOREGRESSIVE_NEXT_TOKEN = "autoregressive_next_token"


class ModelTypes(enum.Enum):
    UNET = "unet"; TRANSFORMER = "transformer"


def load_file(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, str(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("simpletuner", "simpletuner.helpers", "simpletuner.helpers.models", "simpletuner.helpers.data_backend", "simpletuner.helpers.distillation",
                "simpletuner.helpers.distillation.self_transcendence"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    common = types.ModuleType("simpletuner.helpers.models.common")
    common.PredictionTypes, common.ModelTypes = PredictionTypes, ModelTypes
    sys.modules["simpletuner.helpers.models.common"] = common
    dt = types.ModuleType("simpletuner.helpers.data_backend.dataset_types")
    dt.DatasetType = NS(IMAGE="image", VIDEO="video", AUDIO="audio", CONDITIONING="conditioning")
    sys.modules["simpletuner.helpers.data_backend.dataset_types"] = dt
    reg = types.ModuleType("simpletuner.helpers.distillation.registry")
    reg.DistillationRegistry = type("DistillationRegistry", (), {"register": classmethod(lambda cls, *a, **k: None)})
    sys.modules["simpletuner.helpers.distillation.registry"] = reg
    load_file("simpletuner.helpers.distillation.common", REF / "helpers/distillation/common.py")
    return load_file("simpletuner.helpers.distillation.self_transcendence.distiller", REF / "helpers/distillation/self_transcendence/distiller.py")


class Model:
    """the stub plugin: `hidden` is the student block's output (a leaf that takes the gradient), `cond` / `uncond` what the teacher forward captures"""
    PREDICTION_TYPE = PredictionTypes.FLOW_MATCHING
    MODEL_TYPE = ModelTypes.TRANSFORMER
    NAME = "stub"

    def __init__(self, projector, dtype):
        self.config = NS(model_type="lora", lora_type="standard")
        self.accelerator = NS(device=torch.device("cpu"))
        self.component = torch.nn.Module()
        self.component.self_transcendence_projector = projector.to(dtype)
        self.dtype = dtype
        self.cond = self.uncond = None

    def get_trained_component(self, unwrap_model=False):
        return self.component

    def get_prediction_target(self, prepared_batch):
        return prepared_batch["noise"] - prepared_batch["latents"]

    def model_predict(self, batch):
        neg = batch.get("_is_negative", False) or (batch["encoder_hidden_states"] is batch.get("negative_prompt_embeds"))
        return {"hidden_states_buffer": {"layer_2": (self.uncond if neg else self.cond).to(self.dtype)}}


def run_loss(mod, stage, D, Hp, B, lat_shape, S, sigmas, tmin, tmax, weight, cfg_scale, seed, dtype, step=1, stop_step=0):
    """one compute_distill_loss + backward of the executed reference in `dtype`: the recorded inputs and outputs"""
    g = torch.Generator().manual_seed(seed)
    proj = mod.SelfTranscendenceProjector(D, Hp)
    with torch.no_grad():
        for p in proj.parameters():
            p.copy_(torch.randn(p.shape, generator=g) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 20.0))
    params = {nm: p.detach().clone() for nm, p in zip(NAMES, proj.parameters())}
    model = Model(proj, dtype)
    cfg = {"stage": stage, "student_block": 1, "teacher_block": 2 if stage == "self" else None, "weight": weight, "cfg_scale": cfg_scale, "timestep_min": tmin,
           "timestep_max": tmax, "projector_hidden_dim": Hp, "stop_step": stop_step}
    dist = mod.SelfTranscendenceDistiller(model, config=cfg)
    hidden = torch.randn(B, S, D, generator=g)
    latents, noise = torch.randn(*lat_shape, generator=g), torch.randn(*lat_shape, generator=g)
    model.cond, model.uncond = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
    neg = torch.zeros(B, 3, 4)
    batch = {"latents": latents.to(dtype), "noise": noise.to(dtype), "sigmas": torch.tensor(sigmas, dtype=F32).view(B, 1, 1, 1), "encoder_hidden_states": torch.ones(B, 3, 4),
             "negative_prompt_embeds": neg}
    dist.pre_training_step(model, step)
    h = hidden.to(dtype).clone().requires_grad_(True)
    out = {"hidden_states_buffer": {"layer_1": h}}
    dist.prepare_model_output(out)
    original = torch.tensor(0.75, dtype=dtype)
    loss, logs = dist.compute_distill_loss(batch, out, original)
    loss.backward()
    guide = (loss.detach() - original) / (weight if not (stop_step and step >= stop_step) else 1.0)
    grads = {nm: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for nm, p in zip(NAMES, proj.parameters())}
    rec = dict(stage=stage, params=params, hidden=hidden, **(dict(target=(noise - latents)) if stage == "vae" else dict(cond=model.cond, uncond=model.uncond)),
               sigmas=torch.tensor(sigmas, dtype=F32), timestep_min=tmin, timestep_max=tmax, weight=weight, cfg_scale=cfg_scale, original=float(original),
               loss_out=float(loss.detach()), guide=float(guide), logs=dict(logs), dh=(h.grad.detach().clone() if h.grad is not None else torch.zeros_like(hidden)),
               grads=grads, n_active=int(((torch.tensor(sigmas, dtype=F32) >= tmin) & (torch.tensor(sigmas, dtype=F32) <= tmax)).sum()),
               buffer_cleared=(len(out["hidden_states_buffer"]) == 0))
    return rec


def both(mod, **kw):
    """the fp32 run (what is recorded) and the same class run in fp64: their distance is the reference's own fp32 error, the tolerance of the restatement's test"""
    r32, r64 = run_loss(mod, dtype=F32, **kw), run_loss(mod, dtype=F64, **kw)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))
    worst = abs(r32["guide"] - r64["guide"]) / max(abs(r64["guide"]), 1e-30)
    if r64["n_active"]:
        worst = max([worst, rel(r32["dh"], r64["dh"])] + [rel(r32["grads"][nm], r64["grads"][nm]) for nm in NAMES])
    r32["fp32_vs_fp64"] = worst
    return r32


def main():
    mod = load_reference()
    D_ = mod.SelfTranscendenceDistiller
    out = {}
    # ---- normalisation: the defaults, the casts, every ValueError ----
    configs = [
        {"student_block": 1}, {"student_block": "2", "stage": " VAE "}, {"stage": "self", "student_block": 1, "teacher_block": 3, "cfg_scale": 1, "stop_step": None},
        {"student_block": 0, "teacher_adapter_path": "  /tmp/a.safetensors ", "weight": "0.25", "projector_hidden_dim": "512"},
        {"student_block": 1, "teacher_adapter_path": ""}, {"student_block": 1, "timestep_min": 0, "timestep_max": 1},
        {"stage": "both", "student_block": 1}, {}, {"stage": "self", "student_block": 1}, {"student_block": -1}, {"stage": "self", "student_block": 1, "teacher_block": -2},
        {"student_block": 1, "weight": 0}, {"student_block": 1, "weight": -1.0}, {"student_block": 1, "cfg_scale": 0.5},
        {"student_block": 1, "timestep_min": 0.7, "timestep_max": 0.4}, {"student_block": 1, "timestep_min": 0.5, "timestep_max": 0.5},
        {"student_block": 1, "timestep_min": -0.1}, {"student_block": 1, "timestep_max": 1.5}, {"student_block": 1, "stop_step": -3}, {"student_block": 1, "projector_hidden_dim": 0},
    ]
    out["normalize"] = []
    for c in configs:
        try:
            out["normalize"].append(dict(config=dict(c), normalized=D_._normalized_config(dict(c)), error=None))
        except ValueError as e:
            out["normalize"].append(dict(config=dict(c), normalized=None, error=str(e)))
    out["requirements"] = [dict(config=c, requirements=D_.training_batch_requirements(c)) for c in ({"student_block": 1}, {"stage": "self", "student_block": 1, "teacher_block": 2})]
    # ---- _factor_grid (square, non-square, patch 1, the refusal) and _vae_target_tokens ----
    out["factor_grid"] = []
    for shape, tokens in (((10, 14), 35), ((16, 24), 96), ((128, 128), 4096), ((6, 6), 36), ((8, 24), 48), ((24, 8), 48), ((12, 12), 36), ((10, 14), 140), ((10, 14), 33), ((7, 5), 4)):
        try:
            out["factor_grid"].append(dict(shape=shape, tokens=tokens, grid=tuple(D_._factor_grid(shape, tokens)), error=None))
        except ValueError as e:
            out["factor_grid"].append(dict(shape=shape, tokens=tokens, grid=None, error=str(e)))
    g = torch.Generator().manual_seed(5)
    out["target_tokens"] = []
    for shape, tokens in (((2, 16, 10, 14), 35), ((1, 4, 6, 6), 36), ((2, 4, 8, 24), 48)):
        lat = torch.randn(*shape, generator=g)
        out["target_tokens"].append(dict(latents=lat, tokens=tokens, out=D_._vae_target_tokens(lat, torch.zeros(shape[0], tokens, 8), tokens)))
    # ---- the loss of both stages, the no-active-sample branch, the inclusive ends ----
    # (4 latent channels: P = 4 * 2 * 2 = 16 values per token — D = 16 reads every column of the projection, D = 48 a slice; small, so the file stays small)
    kw = dict(B=2, S=35, lat_shape=(2, 4, 10, 14), tmin=0.4, tmax=0.7, weight=0.5, cfg_scale=30.0)
    out["loss"] = {
        "vae": both(mod, stage="vae", D=16, Hp=40, sigmas=[0.55, 0.9], seed=1, **kw),
        "vae_slice": both(mod, stage="vae", D=48, Hp=24, sigmas=[0.55, 0.6], seed=2, **kw),
        "self": both(mod, stage="self", D=32, Hp=40, sigmas=[0.55, 0.9], seed=3, **kw),
        "self_cfg1": both(mod, stage="self", D=32, Hp=40, sigmas=[0.45, 0.65], seed=4, **{**kw, "cfg_scale": 1.0}),
        "none_active": both(mod, stage="vae", D=16, Hp=40, sigmas=[0.1, 0.9], seed=5, **kw),
        "inclusive_ends": both(mod, stage="vae", D=16, Hp=40, sigmas=[0.5, 0.75], seed=6, **{**kw, "tmin": 0.5, "tmax": 0.75}),
    }
    assert out["loss"]["inclusive_ends"]["n_active"] == 2 and out["loss"]["none_active"]["guide"] == 0.0
    # ---- stop_step: the weight is 0 once the step handed to pre_training_step reaches it ----
    below = run_loss(mod, "vae", 16, 40, 2, (2, 4, 10, 14), 35, [0.55, 0.9], 0.4, 0.7, 0.5, 30.0, 7, F32, step=2, stop_step=3)
    at = run_loss(mod, "vae", 16, 40, 2, (2, 4, 10, 14), 35, [0.55, 0.9], 0.4, 0.7, 0.5, 30.0, 7, F32, step=3, stop_step=3)
    assert below["logs"]["self_transcendence/weight"] == 0.5 and at["logs"]["self_transcendence/weight"] == 0.0
    at["step_counter"] = "trainer.py:6876 step = state['global_step']; :6955 step += 1 per fetched batch; :7000 pre_training_step(model, step)"
    at["below_logs"] = below["logs"]
    out["stop_step"] = at
    worst = max(r["fp32_vs_fp64"] for r in out["loss"].values())
    print(f"the reference's own fp32 arithmetic against itself in fp64: worst relative distance {worst:.3e}")
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()

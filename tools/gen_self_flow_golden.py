#!/usr/bin/env python3
"""Generate tests/golden/self_flow_vectors.pt by EXECUTING THE REFERENCE'S Self-Flow code (CREPA with crepa_feature_source=self_flow) on the CPU.

helpers/training/crepa.py (pure torch) is loaded where it lies in a SimpleTuner checkout, by file path; the two methods of helpers/models/common.py that module
cannot be imported for (`_prepare_image_crepa_self_flow_batch`, `_validate_crepa_configuration`) are lifted from its source by AST and executed on a stand-in
`self`.  All of it happens at generation time only; nothing of the reference is copied here and the tests read only the recorded tensors, numbers and messages.

  views         `_prepare_image_crepa_self_flow_batch` with patch size 2 on [3, 16, 6, 10] latents, fp32 and bf16, mask ratios 0 / 0.25 / 0.5, samples with sigma_alt above
                and below sigma: the inputs, the alternate draw handed to `sample_flow_sigmas`, the mask's uniforms (re-drawn from the recorded seed and checked against
                the mask the method returns), every batch entry it writes
  loss          `CrepaRegularizer.compute_loss` in self_flow / image mode (B = 2, 15 tokens, D = 64, fp32, seeded projector): loss, logs, autograd.grad with respect to
                the hidden states and the four projector parameters; the projector's state-dict keys, its LayerNorm eps and what a fresh one holds
  scheduler     `CrepaScheduler.get_weight` trajectories: every scheduler type, warm-up, `crepa_lambda_end`, the step cutoff, the similarity threshold in both modes
  sources       `CrepaFeatureSource.from_config` over the source / alias / legacy-flag table, with its ValueError texts
  errors        the ValueError texts of `_validate_crepa_configuration`, `attach_to_model` and `compute_loss`

    python tools/gen_self_flow_golden.py <SimpleTuner checkout>      (writes tests/golden/self_flow_vectors.pt)
"""
from __future__ import annotations

import ast
import importlib.util
import sys
import textwrap
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "self_flow_vectors.pt"
NAMES = ("0.weight", "0.bias", "1.weight", "1.bias")
ACC = SimpleNamespace(device=torch.device("cpu"))


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_crepa", ref / "helpers/training/crepa.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def _lift(ref: Path, names, env: dict):
    """the named methods of common.py, compiled from their own source text in `env`"""
    src = (ref / "helpers/models/common.py").read_text()
    found = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            ns = dict(env)
            exec(compile(textwrap.dedent(ast.get_source_segment(src, node)), f"common.py:{node.lineno}", "exec"), ns)
            found[node.name] = ns[node.name]
    assert set(found) == set(names), sorted(set(names) - set(found))
    return found


def _err(fn, kind=ValueError):
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"expected a {kind.__name__}")


def _views(prepare, dtype, ratio: float, seed: int):
    B, C, H, W, p = 3, 16, 6, 10, 2
    g = torch.Generator().manual_seed(100 + seed)
    lat, noise = torch.randn(B, C, H, W, generator=g).to(dtype), torch.randn(B, C, H, W, generator=g).to(dtype)
    sigmas = torch.tensor([0.30, 0.70, 0.55])
    alt = torch.tensor([0.65, 0.20, 0.55])          # above, below, equal
    stub = SimpleNamespace(config=SimpleNamespace(crepa_self_flow_mask_ratio=ratio), NAME="golden", sample_flow_sigmas=lambda batch, state: (alt.clone(), alt * 1000.0))
    batch = {"latents": lat, "input_noise": noise, "sigmas": sigmas.clone(), "timesteps": sigmas * 1000.0}
    torch.manual_seed(seed)
    out = prepare(stub, dict(batch), {}, patch_size=p)
    torch.manual_seed(seed)
    uniforms = torch.rand(B, H // p, W // p, dtype=dtype)
    assert torch.equal(uniforms < ratio, out["crepa_self_flow_mask"]), "the re-drawn uniforms do not reproduce the recorded mask"
    if 0.0 < ratio:
        assert 0 < int(out["crepa_self_flow_mask"].sum()) < out["crepa_self_flow_mask"].numel()
    keys = ("sigmas", "timesteps", "noisy_latents", "crepa_teacher_sigmas", "crepa_teacher_timesteps", "crepa_teacher_noisy_latents", "crepa_self_flow_mask")
    return {"latents": lat, "noise": noise, "base_sigmas": sigmas, "base_timesteps": sigmas * 1000.0, "alt_sigmas": alt, "alt_timesteps": alt * 1000.0, "uniforms": uniforms,
            "ratio": float(ratio), "patch_size": p, "seed": seed, **{k: out[k] for k in keys}}


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))


def _cfg(**kw):
    return SimpleNamespace(**{"crepa_enabled": True, "crepa_feature_source": "self_flow", "crepa_block_index": 1, "crepa_teacher_block_index": 2, "crepa_lambda": 0.5,
                              "use_ema": True, **kw})


def _regulariser(mod, D, params=None, **kw):
    foundation = SimpleNamespace(crepa_mode=mod.CrepaMode.IMAGE, supports_validation_preview=lambda: False, NAME="golden")
    reg = mod.CrepaRegularizer(_cfg(**kw), ACC, D, model_foundation=foundation, max_train_steps=100)
    model = _Model()
    reg.attach_to_model(model)
    if params is not None:
        own = dict(reg.projector.named_parameters())
        with torch.no_grad():
            for nm in NAMES:
                own[nm].copy_(params[nm])
    return reg, model


def _loss(mod):
    B, S, D = 2, 15, 64
    g = torch.Generator().manual_seed(4711)
    hidden, teacher = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
    params = {"0.weight": 1.0 + 0.25 * torch.randn(D, generator=g), "0.bias": 0.1 * torch.randn(D, generator=g), "1.weight": torch.randn(D, D, generator=g) / D ** 0.5,
              "1.bias": 0.05 * torch.randn(D, generator=g)}
    reg, model = _regulariser(mod, D, params)
    h = hidden.clone().requires_grad_(True)
    loss, logs = reg.compute_loss(hidden_states=h, latents=None, frame_features=teacher, step=0)
    own = dict(reg.projector.named_parameters())
    grads = torch.autograd.grad(loss, [h] + [own[nm] for nm in NAMES])
    fresh, _ = _regulariser(mod, D)
    fp = dict(fresh.projector.named_parameters())
    sd = reg.projector.state_dict()
    out = {"shape": (B, S, D), "hidden": hidden, "teacher": teacher, "params": params, "loss": loss.detach(), "logs": dict(logs), "grad_hidden": grads[0],
           "grads": {nm: gg for nm, gg in zip(NAMES, grads[1:])}, "projection": reg.projector(hidden.reshape(-1, D)).detach(),
           "state_keys": list(sd.keys()), "module_name": "crepa_projector", "attached": hasattr(model, "crepa_projector"), "eps": float(reg.projector[0].eps),
           "param_dtype": str(next(reg.projector.parameters()).dtype),
           "init": {"norm_weight_one": bool((fp["0.weight"] == 1).all()), "norm_bias_zero": bool((fp["0.bias"] == 0).all()), "linear_abs_max": float(fp["1.weight"].detach().abs().max()),
                    "bias_abs_max": float(fp["1.bias"].detach().abs().max()), "bound": 1.0 / D ** 0.5}}
    # the scheduler's cutoff inside compute_loss: no loss, the cutoff log
    reg_cut, _ = _regulariser(mod, D, params, crepa_cutoff_step=1)
    loss_cut, logs_cut = reg_cut.compute_loss(hidden_states=hidden, latents=None, frame_features=teacher, step=3)
    out["cutoff"] = {"loss_is_none": loss_cut is None, "logs": dict(logs_cut)}
    reg_thr, _ = _regulariser(mod, D, params, crepa_similarity_threshold=-1.0)
    _, logs_thr = reg_thr.compute_loss(hidden_states=hidden, latents=None, frame_features=teacher, step=0)
    out["threshold"] = {"logs": dict(logs_thr)}
    return out, reg, hidden, teacher


def _schedules(mod):
    sims = [0.10, 0.30, 0.62, 0.70, 0.20, 0.05, 0.05, 0.05, 0.40, 0.90, 0.10, 0.10]
    cases = {
        "constant": dict(crepa_scheduler="constant", crepa_lambda=0.5),
        "constant_warmup": dict(crepa_scheduler="constant", crepa_lambda=0.4, crepa_warmup_steps=4),
        "linear": dict(crepa_scheduler="linear", crepa_lambda=0.5, crepa_lambda_end=0.1, crepa_decay_steps=8),
        "linear_warmup": dict(crepa_scheduler="linear", crepa_lambda=0.5, crepa_lambda_end=0.1, crepa_warmup_steps=3, crepa_decay_steps=9),
        "cosine": dict(crepa_scheduler="cosine", crepa_lambda=0.5, crepa_lambda_end=0.05, crepa_decay_steps=10),
        "polynomial": dict(crepa_scheduler="polynomial", crepa_lambda=0.5, crepa_lambda_end=0.1, crepa_power=2.0, crepa_decay_steps=10),
        "default_decay_steps": dict(crepa_scheduler="linear", crepa_lambda=0.5),
        "unknown_type": dict(crepa_scheduler="exotic", crepa_lambda=0.3, crepa_warmup_steps=2),
        "cutoff_step": dict(crepa_scheduler="constant", crepa_lambda=0.5, crepa_cutoff_step=5),
        "threshold_permanent": dict(crepa_scheduler="constant", crepa_lambda=0.5, crepa_similarity_threshold=0.35, crepa_similarity_ema_decay=0.5, crepa_threshold_mode="permanent"),
        "threshold_recoverable": dict(crepa_scheduler="constant", crepa_lambda=0.5, crepa_similarity_threshold=0.35, crepa_similarity_ema_decay=0.5,
                                      crepa_threshold_mode="recoverable"),
        "threshold_default_decay": dict(crepa_scheduler="cosine", crepa_lambda=0.5, crepa_similarity_threshold=0.3, crepa_decay_steps=12),
        "zero_lambda": dict(crepa_scheduler="constant", crepa_lambda=0.0),
    }
    out = {}
    for name, kw in cases.items():
        sch = mod.CrepaScheduler(SimpleNamespace(**kw), 20)
        rows = []
        for step, sim in enumerate(sims):
            w = sch.get_weight(step, similarity=sim)
            rows.append({"step": step, "similarity": sim, "weight": float(w), "ema": sch.get_similarity_ema(), "cutoff": bool(sch.is_cutoff())})
        out[name] = {"config": kw, "max_train_steps": 20, "rows": rows}
    return out


def _sources(mod):
    table = []
    for raw in (None, "encoder", "external", "backbone", "internal", "self_flow", "selfflow", " Self_Flow ", "SELFFLOW", "dino"):
        for bb in (False, True):
            for sf in (False, True):
                cfg = SimpleNamespace(crepa_feature_source=raw, crepa_use_backbone_features=bb, crepa_self_flow=sf)
                try:
                    res = ("ok", mod.CrepaFeatureSource.from_config(cfg).value)
                except ValueError as e:
                    res = ("error", str(e))
                table.append({"crepa_feature_source": raw, "crepa_use_backbone_features": bb, "crepa_self_flow": sf, "result": res})
    return {"table": table, "values": [o.value for o in mod.CrepaFeatureSource]}


def main(ref: Path):
    mod = _load(ref)
    lifted = _lift(ref, ("_prepare_image_crepa_self_flow_batch", "_validate_crepa_configuration"), {"torch": torch, "CrepaFeatureSource": mod.CrepaFeatureSource})
    prepare, validate = lifted["_prepare_image_crepa_self_flow_batch"], lifted["_validate_crepa_configuration"]
    out = {"views": {}}
    for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for k, ratio in enumerate((0.0, 0.25, 0.5)):
            out["views"][f"{dt_name}_ratio{ratio}"] = _views(prepare, dt, ratio, seed=7 + k)
    out["loss"], reg, hidden, teacher = _loss(mod)
    out["scheduler"] = _schedules(mod)
    out["sources"] = _sources(mod)

    def v(supported=True, **kw):
        stub = SimpleNamespace(config=_cfg(**kw), NAME="Golden Family", supports_crepa_self_flow=lambda: supported)
        return lambda: validate(stub)
    assert validate(SimpleNamespace(config=_cfg(), NAME="x", supports_crepa_self_flow=lambda: True)).value == "self_flow"
    unattached = mod.CrepaRegularizer(_cfg(), ACC, 64, model_foundation=SimpleNamespace(crepa_mode=mod.CrepaMode.IMAGE, supports_validation_preview=lambda: False), max_train_steps=10)
    no_block = mod.CrepaRegularizer(_cfg(crepa_block_index=None), ACC, 64, max_train_steps=10)
    out["errors"] = {
        "unsupported_family": _err(v(supported=False)),
        "no_ema": _err(v(use_ema=False)),
        "no_teacher_block": _err(v(crepa_teacher_block_index=None)),
        "ratio_high": _err(v(crepa_self_flow_mask_ratio=0.6)),
        "ratio_negative": _err(v(crepa_self_flow_mask_ratio=-0.1)),
        "twinflow": _err(v(twinflow_enabled=True)),
        "both_legacy": _err(v(crepa_feature_source=None, crepa_use_backbone_features=True, crepa_self_flow=True)),
        "backbone_flag_conflict": _err(v(crepa_use_backbone_features=True)),
        "self_flow_flag_conflict": _err(v(crepa_feature_source="backbone", crepa_self_flow=True)),
        "bad_source": _err(v(crepa_feature_source="dino")),
        "no_block_index": _err(lambda: no_block.attach_to_model(_Model())),
        "no_hidden": _err(lambda: reg.compute_loss(hidden_states=None, latents=None, frame_features=teacher)),
        "no_teacher_features": _err(lambda: reg.compute_loss(hidden_states=hidden, latents=None, frame_features=None)),
        "unattached": _err(lambda: unattached.compute_loss(hidden_states=hidden, latents=None, frame_features=teacher), RuntimeError),
    }
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))

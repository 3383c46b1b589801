#!/usr/bin/env python3
"""Generate tests/golden/twinflow_vectors.pt by EXECUTING THE REFERENCE'S TwinFlow code (twinflow_enabled) on the CPU.

helpers/models/common.py cannot be imported without the whole trainer, so the TwinFlow methods of its `ModelFoundation` — `_validate_twinflow_config`,
`_twinflow_*`, `_prepare_twinflow_metadata`, `_compute_twinflow_losses`, the flow-target helpers and `auxiliary_loss` — are lifted from its source by AST and
executed on a stand-in foundation: a seeded `model_predict` that depends on its input, its timestep and its conditioning (STUB below: this tool's own formula,
which the tests restate), and an `_ema_teacher_weights_context` that switches a fixed perturbation of that formula on.  `TwinFlowScheduler` is lifted from
helpers/training/custom_schedule.py the same way, over stand-ins for the two diffusers mixins.  All of it happens at generation time only; nothing of the
reference is copied here and the tests read only the recorded tensors, numbers and messages.

  settings      `_twinflow_settings` over absent / None / "" / given values; the ValueError texts of `_validate_twinflow_config` and `_twinflow_active`
  tt            `_prepare_twinflow_metadata` (site 1) and the second cap inside `_compute_twinflow_losses` (site 2) with the dtype and eps each site sees
  loss          `auxiliary_loss` -> `_compute_twinflow_losses` in fp64, fp32 and bf16: orders 1 / 2 / 3, ratio 0 / 0.5 with and without negative embeds, clamp 1.0 / 0.25,
                sigmas including one below delta_t and one below eps: the twin term, both logs, d twin / d prediction, every teacher forward's (timestep, conditioning)
  sampler       `TwinFlowScheduler.set_timesteps` grids for 1 .. 6 steps and `step` chains of 1 / 2 / 4 steps with given noise, in fp64, fp32 and bf16

    python tools/gen_twinflow_golden.py <SimpleTuner checkout>/simpletuner      (writes tests/golden/twinflow_vectors.pt)
"""
from __future__ import annotations

import ast
import contextlib
import logging
import sys
import textwrap
from enum import Enum
from pathlib import Path
from types import SimpleNamespace
from typing import List, Mapping, Optional, Tuple, Union

import torch
import torch.nn.functional as F

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "twinflow_vectors.pt"
DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "bf16": torch.bfloat16}
STUB = {"w": (0.55, 0.30, -0.40, 0.80), "dw": (0.06, -0.05, 0.07, -0.10)}          # the stand-in model's weights and the EMA teacher's offsets

FOUNDATION_METHODS = ("_validate_twinflow_config", "_twinflow_active", "_twinflow_settings", "_twinflow_restore_rng_state", "_twinflow_sample_tt",
                      "_prepare_twinflow_metadata", "_twinflow_match_time_shape", "_twinflow_teacher_context", "_twinflow_cfg_batches", "_twinflow_enhance_target",
                      "_twinflow_forward", "_twinflow_reconstruct_states", "_twinflow_rcgm_target", "_compute_twinflow_losses", "auxiliary_loss",
                      "get_flow_matching_target", "flow_matching_target", "noiseward_flow_to_prediction", "prediction_to_noiseward_flow",
                      "flow_matching_target_direction")


class PredictionTypes(Enum):
    EPSILON = "epsilon"
    V_PREDICTION = "v_prediction"
    FLOW_MATCHING = "flow_matching"


def stub_predict(x, timesteps, enc, teacher_on: bool):
    """the stand-in model, in x's dtype: w0 x + w1 roll(x, 1, W) s + w2 tanh(flip(x, H)) (1 - s) + w3 mean(enc), s = timesteps / 1000"""
    B = x.shape[0]
    w = [a + (b if teacher_on else 0.0) for a, b in zip(STUB["w"], STUB["dw"])]
    s = (timesteps.reshape(B).to(x.dtype) / 1000.0).view(B, 1, 1, 1)
    e = enc.to(x.dtype).mean(dim=(1, 2)).view(B, 1, 1, 1)
    return w[0] * x + w[1] * torch.roll(x, 1, -1) * s + w[2] * torch.tanh(x.flip(-2)) * (1 - s) + w[3] * e


def _lift_class(path: Path, cls: str, names, env: dict) -> dict:
    """the named methods of class `cls`, compiled from their own source text in `env` (decorators re-applied by name)"""
    src = path.read_text()
    found = {}
    for top in ast.parse(src).body:
        if isinstance(top, ast.ClassDef) and top.name == cls:
            for node in top.body:
                if isinstance(node, ast.FunctionDef) and (names is None or node.name in names):
                    ns = dict(env)
                    exec(compile(textwrap.dedent(ast.get_source_segment(src, node)), f"{path.name}:{node.lineno}", "exec"), ns)
                    fn = ns[node.name]
                    for dec in reversed(node.decorator_list):
                        d = ast.unparse(dec)
                        fn = {"staticmethod": staticmethod, "contextlib.contextmanager": contextlib.contextmanager, "register_to_config": env.get("register_to_config")}[d](fn)
                    found[node.name] = fn
    if names is not None:
        assert set(found) == set(names), sorted(set(names) - set(found))
    return found


def _foundation_class(ref: Path):
    env = {"torch": torch, "F": F, "Optional": Optional, "Mapping": Mapping, "contextlib": contextlib, "logger": logging.getLogger("twinflow_golden"),
           "PredictionTypes": PredictionTypes}
    holder = {}
    env["ModelFoundation"] = type("_Late", (), {"__getattr__": lambda self, name: getattr(holder["cls"], name)})()      # `_twinflow_reconstruct_states` names its class
    body = _lift_class(ref / "helpers/models/common.py", "ModelFoundation", FOUNDATION_METHODS, env)

    @contextlib.contextmanager
    def _ema_teacher_weights_context(self, *, require_ema=True, allow_student_fallback=False):
        has_ema = self.ema_model is not None and getattr(self.config, "use_ema", False)
        if require_ema and not has_ema and not allow_student_fallback:
            raise ValueError("EMA teacher weights are required but unavailable; enable use_ema or allow fallback.")
        self.teacher_on = bool(has_ema)
        try:
            yield has_ema
        finally:
            self.teacher_on = False

    def model_predict(self, prepared_batch):
        enc = prepared_batch["encoder_hidden_states"]
        self.calls.append(dict(timesteps=prepared_batch["timesteps"].detach().clone(), cond="uncond" if enc is self.negative else "cond",
                               teacher=self.teacher_on, grad=torch.is_grad_enabled(), noisy=prepared_batch["noisy_latents"].detach().clone(),
                               sign=prepared_batch.get("twinflow_time_sign")))
        return {"model_prediction": stub_predict(prepared_batch["noisy_latents"], prepared_batch["timesteps"], enc, self.teacher_on)}

    body.update(_ema_teacher_weights_context=_ema_teacher_weights_context, model_predict=model_predict, PREDICTION_TYPE=PredictionTypes.FLOW_MATCHING,
                diff2flow_bridge=None, NAME="golden")
    cls = holder["cls"] = type("Foundation", (), body)
    return cls


def _make(cls, dtype, prediction=PredictionTypes.FLOW_MATCHING, **cfg):
    f = cls.__new__(cls)
    f.config = SimpleNamespace(weight_dtype=dtype, **cfg)
    f.accelerator = SimpleNamespace(device=torch.device("cpu"))
    f.PREDICTION_TYPE = prediction
    f.ema_model = object() if cfg.get("use_ema") else None
    f.teacher_on, f.calls, f.negative = False, [], None
    return f


def _err(fn, kind=ValueError):
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"expected a {kind.__name__}")


def _settings(cls):
    rec = {}
    for name, cfg in (("absent", {}), ("none", dict(twinflow_estimate_order=None, twinflow_enhanced_ratio=None, twinflow_target_step_count=None, twinflow_delta_t=None,
                                                    twinflow_target_clamp=None)),
                      ("empty", dict(twinflow_estimate_order="", twinflow_enhanced_ratio="", twinflow_target_step_count="", twinflow_delta_t="", twinflow_target_clamp="")),
                      ("given", dict(twinflow_estimate_order=3, twinflow_enhanced_ratio=0.25, twinflow_target_step_count=4, twinflow_delta_t=0.05, twinflow_target_clamp=0.5,
                                     twinflow_adversarial_enabled=True, twinflow_require_ema=False)),
                      ("floors", dict(twinflow_estimate_order=0, twinflow_target_step_count=-2, twinflow_enhanced_ratio=0, twinflow_delta_t=0, twinflow_target_clamp=0))):
        rec[name] = dict(config=cfg, settings=_make(cls, torch.float32, twinflow_enabled=True, use_ema=True, **cfg)._twinflow_settings())
    errors = {}
    for name, pt, cfg in (("not_flow", PredictionTypes.EPSILON, dict(twinflow_enabled=True, use_ema=True)),
                          ("not_flow_one_flag", PredictionTypes.V_PREDICTION, dict(twinflow_enabled=True, use_ema=True, diff2flow_enabled=True)),
                          ("no_ema", PredictionTypes.FLOW_MATCHING, dict(twinflow_enabled=True))):
        errors[name] = dict(config=cfg, prediction=pt.value, message=_err(lambda: _make(cls, torch.float32, pt, **cfg)._validate_twinflow_config()))
    passes = {}
    for name, pt, cfg in (("off", PredictionTypes.EPSILON, {}), ("ema", PredictionTypes.FLOW_MATCHING, dict(twinflow_enabled=True, use_ema=True)),
                          ("allow_student", PredictionTypes.FLOW_MATCHING, dict(twinflow_enabled=True, twinflow_allow_no_ema_teacher=True)),
                          ("not_required", PredictionTypes.FLOW_MATCHING, dict(twinflow_enabled=True, twinflow_require_ema=False)),
                          ("bridge", PredictionTypes.EPSILON, dict(twinflow_enabled=True, use_ema=True, diff2flow_enabled=True, twinflow_allow_diff2flow=True))):
        f = _make(cls, torch.float32, pt, **cfg)
        f._validate_twinflow_config()
        passes[name] = dict(config=cfg, prediction=pt.value, bridge=bool(f._twinflow_diffusion_bridge), active=bool(f._twinflow_active()))
    f = _make(cls, torch.float32, PredictionTypes.EPSILON, twinflow_enabled=True)
    f._twinflow_diffusion_bridge = False
    errors["active_not_flow"] = dict(config=dict(twinflow_enabled=True), prediction="epsilon", message=_err(f._twinflow_active))
    f = _make(cls, torch.float32, twinflow_enabled=True)
    f._twinflow_allow_student_teacher = False
    errors["teacher_context_no_ema"] = dict(message=_err(lambda: f._twinflow_teacher_context({}, {"require_ema": True}, None).__enter__()))
    return dict(settings=rec, errors=errors, passes=passes)


SIGMAS = (0.62, 0.305, 0.004, 3.0e-8, 0.97)          # ordinary, ordinary, below delta_t, below eps (fp32), near the noise end
UNIFORMS = (0.35, 0.999999, 0.5, 0.25, 1.0e-9)       # second: tt close to 0; last: tt would reach sigma, capped at sigma - eps


def _case(cls, name, dtype, order, ratio, negative, clamp, teacher="ema"):
    B, C, H, W = len(SIGMAS), 4, 4, 6
    g = torch.Generator().manual_seed(20260 + order)
    lat, noise = torch.randn(B, C, H, W, generator=g, dtype=torch.float64), torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    enc, neg = torch.randn(B, 3, 8, generator=g, dtype=torch.float64), torch.randn(B, 3, 8, generator=g, dtype=torch.float64)
    base = 0.8 * (noise - lat) + 0.9 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    sig_dtype = torch.float64 if dtype is torch.float64 else torch.float32          # the sampler's sigmas are fp32 whatever the weight dtype
    sigmas, uni = torch.tensor(SIGMAS, dtype=sig_dtype), torch.tensor(UNIFORMS, dtype=sig_dtype)
    cfg = dict(twinflow_enabled=True, twinflow_estimate_order=order, twinflow_enhanced_ratio=ratio, twinflow_target_clamp=clamp)
    cfg.update({"ema": dict(use_ema=True), "student": dict(twinflow_allow_no_ema_teacher=True)}[teacher])
    f = _make(cls, dtype, **cfg)
    f._validate_twinflow_config()
    s4 = sigmas.view(B, 1, 1, 1)
    batch = {"latents": lat.to(dtype), "noise": noise.to(dtype), "input_noise": noise.to(dtype), "sigmas": s4.clone(), "timesteps": sigmas * 1000.0,
             "encoder_hidden_states": enc.to(dtype), "prompt_embeds": enc.to(dtype)}
    batch["noisy_latents"] = ((1.0 - s4) * batch["latents"] + s4 * batch["input_noise"]).to(dtype)
    if negative:
        f.negative = batch["negative_prompt_embeds"] = neg.to(dtype)
    # site 1: `_twinflow_sample_tt` draws torch.rand_like(sigmas); the draw is pinned by patching it for this one call
    rand_like = torch.rand_like
    torch.rand_like = lambda t, **k: uni.view_as(t).to(t.dtype)
    try:
        f._prepare_twinflow_metadata(batch)
    finally:
        torch.rand_like = rand_like
    tt1 = batch["twinflow_tt"].detach().clone()
    site1 = dict(dtype=str(batch["sigmas"].dtype), eps=float(torch.finfo(batch["sigmas"].dtype).eps), shape=tuple(tt1.shape))
    pred = base.to(dtype).requires_grad_(True)
    zero = torch.zeros((), dtype=torch.float32)
    loss, logs = f.auxiliary_loss({"model_prediction": pred}, batch, zero, apply_layersync=False)
    (grad,) = torch.autograd.grad(loss, pred)
    tt2 = batch["twinflow_tt"].detach().clone()
    site2 = dict(dtype=str(dtype), eps=float(torch.finfo(dtype).eps), shape=tuple(tt2.shape), tt_dtype=str(tt2.dtype))
    calls = [dict(timesteps=c["timesteps"], cond=c["cond"], teacher=c["teacher"], grad=c["grad"], noisy=c["noisy"],
                  sign=None if c["sign"] is None else c["sign"].detach().clone()) for c in f.calls]
    return dict(name=name, dtype=str(dtype), order=order, ratio=ratio, negative=bool(negative), clamp=clamp, teacher=teacher, latents=batch["latents"], noise=batch["noise"],
                noisy=batch["noisy_latents"], enc=batch["encoder_hidden_states"], neg=batch.get("negative_prompt_embeds"), sigmas=sigmas, uniforms=uni, pred=pred.detach(),
                tt_site1=tt1, tt_site2=tt2, site1=site1, site2=site2, loss=loss.detach(), logs=dict(logs), grad=grad, calls=calls, rng_state_recorded="twinflow_rng_state" in batch)


def _losses(cls):
    out = {}
    grid = [(1, 0.0, False, 1.0), (2, 0.0, False, 1.0), (2, 0.5, True, 1.0), (2, 0.5, False, 1.0), (2, 0.0, True, 1.0), (3, 0.5, True, 0.25), (3, 0.0, False, 0.25),
            (1, 0.5, True, 0.25)]
    for dn, dtype in DTYPES.items():
        for order, ratio, negative, clamp in grid:
            name = f"{dn}.order{order}.ratio{ratio}.neg{int(negative)}.clamp{clamp}"
            out[name] = _case(cls, name, dtype, order, ratio, negative, clamp)
        out[f"{dn}.student"] = _case(cls, f"{dn}.student", dtype, 2, 0.5, True, 1.0, teacher="student")
    return out


def _scheduler_class(ref: Path):
    def register_to_config(init):
        def wrapped(self, *a, **k):
            import inspect
            bound = inspect.signature(init).bind(self, *a, **k)
            bound.apply_defaults()
            self.config = SimpleNamespace(**{n: v for n, v in bound.arguments.items() if n != "self"})
            init(self, *a, **k)
        return wrapped

    env = {"torch": torch, "Optional": Optional, "Union": Union, "List": List, "Tuple": Tuple, "logger": logging.getLogger("twinflow_golden"),
           "register_to_config": register_to_config,
           "TwinFlowSchedulerOutput": lambda prev_sample, pred_original_sample=None: SimpleNamespace(prev_sample=prev_sample, pred_original_sample=pred_original_sample)}
    body = _lift_class(ref / "helpers/training/custom_schedule.py", "TwinFlowScheduler", None, env)
    return type("TwinFlowScheduler", (), body)


def _sampler(Sched):
    grids = {}
    for n in (1, 2, 3, 4, 5, 6):
        s = Sched()
        s.set_timesteps(n)
        grids[n] = dict(sigmas=s.sigmas.clone(), timesteps=s.timesteps.clone())
    chains = {}
    for dn, dtype in DTYPES.items():
        for n in (1, 2, 4):
            for rho in (1.0, 0.0, 0.36):
                g = torch.Generator().manual_seed(777 + n)
                x0 = torch.randn(2, 4, 4, 6, generator=g, dtype=torch.float64).to(dtype)
                vs = [torch.randn(2, 4, 4, 6, generator=g, dtype=torch.float64).to(dtype) for _ in range(n)]
                noises = [torch.randn(2, 4, 4, 6, generator=g, dtype=torch.float64).to(dtype) for _ in range(n)]
                s = Sched(stochast_ratio=rho)
                s.set_timesteps(n)
                x, states = x0, []
                randn = torch.randn
                for i, t in enumerate(s.timesteps):
                    torch.randn = lambda *a, _i=i, **k: noises[_i]          # `step` draws torch.randn(sample.shape, ...): the draw is pinned to the recorded noise
                    try:
                        x = s.step(vs[i], t, x, return_dict=False)[0]
                    finally:
                        torch.randn = randn
                    states.append(x.clone())
                chains[f"{dn}.steps{n}.rho{rho}"] = dict(dtype=str(dtype), steps=n, rho=rho, x0=x0, v=vs, noise=noises, states=states, sigmas=s.sigmas.clone())
    return dict(grids=grids, chains=chains)


def main():
    ref = Path(sys.argv[1])
    cls = _foundation_class(ref)
    rec = dict(stub=STUB, sigmas=SIGMAS, uniforms=UNIFORMS, config=_settings(cls), losses=_losses(cls), sampler=_sampler(_scheduler_class(ref)))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(rec, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(rec['losses'])} loss cases, {len(rec['sampler']['chains'])} sampler chains")
    for k in ("fp64", "fp32", "bf16"):
        c = rec["losses"][f"{k}.order2.ratio0.5.neg1.clamp1.0"]
        print(k, "site1", c["site1"], "site2", c["site2"], "tt1", c["tt_site1"].flatten().tolist(), "tt2", c["tt_site2"].flatten().tolist(), "logs", c["logs"])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/eval_loss_vectors.pt by EXECUTING THE REFERENCE'S evaluation-loss code (eval_steps_interval) on the CPU.

helpers/training/validation.py and helpers/training/trainer.py cannot be imported without the whole trainer, so the methods of `Evaluation`, `Trainer.
_prepare_custom_timestep_batch` and `ModelFoundation.calculate_dynamic_shift_mu` (with sd3/pipeline.py's `calculate_shift`) are lifted from their source by AST and
executed over stand-ins: a StateTracker that hands out the config / the eval sets / a model, iterators in place of the eval samplers, a seeded `calculate_loss`
(STUB below: this tool's own formula, which the tests restate).  The timestep grid is set on THIS repository's FlowMatchEulerDiscreteScheduler (the reference
calls diffusers' class, which is not installed here; the repository's restates it).  All of it happens at generation time only; nothing of the reference is copied
here and the tests read only the recorded tensors, numbers and messages.

  schedule      `get_timestep_schedule` for eval_timesteps 1 / 4 / 7 / 28: static shift 1.0 / 3.0 (training bounds reset), dynamic shifting at three latent sizes (the mu
                the lifted `calculate_dynamic_shift_mu` derives), and the ValueError when no mu can be derived
  custom_batch  `_prepare_custom_timestep_batch`, flow-matching branch, on small bf16 and fp32 batches for every timestep of two grids, the timestep tensor built as
                validation.py:5584-5591 builds it (cast to the weight dtype first): the overridden timesteps / sigmas / noisy_latents with their dtypes
  would         `would_evaluate` over runs of states: step interval with a resume step, epoch interval, both (the warning), a non-main process, unset / unparsable values
  table         `generate_tracker_table` on given loss tables
  passes        `execute_eval` -> `_evaluate_dataset_pass` over two eval sets, pooled and per dataset, with and without num_eval_images: which (set, batch, timestep)
                entries were evaluated, the returned keys, the tracker table, and that the torch RNG state is restored

    python tools/gen_eval_loss_golden.py <SimpleTuner checkout>/simpletuner      (writes tests/golden/eval_loss_vectors.pt)
"""
from __future__ import annotations

import ast
import inspect
import logging
import math
import sys
import textwrap
import types
from enum import Enum
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "eval_loss_vectors.pt"
STUB = {"scale": 0.001, "base": 0.25}          # calculate_loss of the pass records: base * (1 + batch id) + scale * timestep


class PredictionTypes(Enum):
    EPSILON = "epsilon"
    V_PREDICTION = "v_prediction"
    FLOW_MATCHING = "flow_matching"


class MultiDatasetExhausted(Exception):
    pass


def _lift_methods(path: Path, cls: str, names, env: dict) -> dict:
    src = path.read_text()
    found = {}
    for top in ast.parse(src).body:
        if isinstance(top, ast.ClassDef) and top.name == cls:
            for node in top.body:
                if isinstance(node, ast.FunctionDef) and (names is None or node.name in names):
                    ns = dict(env)
                    exec(compile(textwrap.dedent(ast.get_source_segment(src, node)), f"{path.name}:{node.lineno}", "exec"), ns)
                    found[node.name] = ns[node.name]
    if names is not None:
        assert set(found) == set(names), sorted(set(names) - set(found))
    return found


def _lift_function(path: Path, name: str, env: dict):
    src = path.read_text()
    for top in ast.parse(src).body:
        if isinstance(top, ast.FunctionDef) and top.name == name:
            ns = dict(env)
            exec(compile(ast.get_source_segment(src, top), f"{path.name}:{top.lineno}", "exec"), ns)
            return ns[name]
    raise KeyError(name)


class _Tqdm:
    """tqdm's two uses in the pass: a progress bar that is updated, and a wrapped iterable"""

    def __init__(self, iterable=None, **kw):
        self.iterable = iterable

    def __iter__(self):
        return iter(self.iterable)

    def update(self, n=1):
        pass


class _World:
    """what the lifted code reaches through module globals: StateTracker, the eval samplers, reset / retrieve"""

    def __init__(self):
        self.config = None
        self.model = None
        self.sets = {}          # name -> list of raw batches
        self.cursor = {}
        self.warnings = []

    # StateTracker
    def get_args(self):
        return self.config

    def get_epoch(self):
        return 1

    def get_model(self):
        return self.model

    def get_data_backends(self, _type=None, _types=None):
        return {name: {"sampler": batches} for name, batches in self.sets.items()}

    # validation.py's module-level helpers, over plain lists
    def reset_eval_datasets(self):
        self.cursor = {name: 0 for name in self.sets}

    def retrieve_eval_images(self, dataset_name=None):
        for name in ([dataset_name] if dataset_name is not None else list(self.sets)):
            i = self.cursor.get(name, 0)
            if i < len(self.sets[name]):
                self.cursor[name] = i + 1
                return self.sets[name][i]
        raise MultiDatasetExhausted()


def _classes(ref: Path, world: _World):
    log = logging.getLogger("eval_loss_golden")

    class _Catch(logging.Handler):
        def emit(self, record):
            if record.levelno >= logging.WARNING:
                world.warnings.append(record.getMessage())
    log.addHandler(_Catch())
    log.propagate = False
    env = {"torch": torch, "math": math, "inspect": inspect, "logger": log, "StateTracker": world, "tqdm": _Tqdm, "wandb": None,
           "reset_eval_datasets": world.reset_eval_datasets, "retrieve_eval_images": world.retrieve_eval_images, "MultiDatasetExhausted": MultiDatasetExhausted}
    Evaluation = type("Evaluation", (), _lift_methods(ref / "helpers/training/validation.py", "Evaluation", None, env))
    trainer = _lift_methods(ref / "helpers/training/trainer.py", "Trainer", ("_prepare_custom_timestep_batch",), {"torch": torch, "PredictionTypes": PredictionTypes})
    Trainer = type("Trainer", (), trainer)
    # `calculate_dynamic_shift_mu` imports sd3/pipeline.py's calculate_shift by module path: that one function, lifted, behind the same path
    shift = _lift_function(ref / "helpers/models/sd3/pipeline.py", "calculate_shift", {})
    for name in ("simpletuner", "simpletuner.helpers", "simpletuner.helpers.models", "simpletuner.helpers.models.sd3", "simpletuner.helpers.models.sd3.pipeline"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["simpletuner.helpers.models.sd3.pipeline"].calculate_shift = shift
    Foundation = type("Foundation", (), _lift_methods(ref / "helpers/models/common.py", "ModelFoundation", ("_get_patch_size_for_dynamic_shift", "calculate_dynamic_shift_mu"),
                                                      {"torch": torch}))
    return Evaluation, Trainer, Foundation


def _model(Foundation, patch_size=2):
    m = Foundation.__new__(Foundation)
    m.config = SimpleNamespace()
    m.get_trained_component = lambda: SimpleNamespace(config=SimpleNamespace(patch_size=patch_size))
    return m


def _schedulers():
    from simpletuner_amd.sampling import FlowMatchEulerDiscreteScheduler, fix_flow_match_euler_schedule_bounds
    return {"shift1": lambda: fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=1.0)),
            "shift3": lambda: fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=3.0)),
            "dynamic": lambda: FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=True)}


def _err(fn, kind=ValueError):
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"expected a {kind.__name__}")


def _schedule(world, Evaluation, Foundation):
    rec = {}
    for name, make in _schedulers().items():
        for T in (1, 4, 7, 28):
            for hw in ((16, 16), (32, 48), (128, 128)) if name == "dynamic" else ((16, 16),):
                world.config = SimpleNamespace(eval_timesteps=T)
                world.model = _model(Foundation)
                ev = Evaluation(SimpleNamespace(is_main_process=True))
                sched = make()
                lat = torch.zeros(1, 16, *hw)
                ts = ev.get_timestep_schedule(sched, latents=lat)
                mu = world.model.calculate_dynamic_shift_mu(sched, lat) if name == "dynamic" else None
                rec[f"{name}.T{T}.{hw[0]}x{hw[1]}"] = dict(scheduler=name, eval_timesteps=T, hw=hw, timesteps=ts.clone(), sigmas=sched.sigmas.clone(), mu=mu)
    world.config = SimpleNamespace(eval_timesteps=4)
    world.model = None
    ev = Evaluation(SimpleNamespace(is_main_process=True))
    no_model = _err(lambda: ev.get_timestep_schedule(_schedulers()["dynamic"](), latents=torch.zeros(1, 16, 16, 16)))
    world.model = _model(Foundation)
    no_latents = _err(lambda: ev.get_timestep_schedule(_schedulers()["dynamic"](), latents=None))
    return dict(grids=rec, errors=dict(no_model=no_model, no_latents=no_latents))


def _custom_batch(world, Evaluation, Trainer, Foundation):
    out = {}
    for dn, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        for grid_name, T in (("shift3", 7), ("shift3", 28), ("shift1", 4)):
            world.config = SimpleNamespace(eval_timesteps=T, weight_dtype=dtype)
            world.model = _model(Foundation)
            ev = Evaluation(SimpleNamespace(is_main_process=True))
            sched = _schedulers()[grid_name]()
            grid = ev.get_timestep_schedule(sched, latents=None)
            g = torch.Generator().manual_seed(31 + T)
            B = 2
            lat, noise = torch.randn(B, 4, 4, 4, generator=g).to(dtype), torch.randn(B, 4, 4, 4, generator=g).to(dtype)
            sig0 = torch.tensor([0.3, 0.7])
            prepared = {"latents": lat, "noise": noise, "input_noise": noise, "timesteps": sig0 * 1000.0, "sigmas": sig0.view(B, 1, 1, 1),
                        "noisy_latents": ((1 - sig0.view(B, 1, 1, 1)) * lat.float() + sig0.view(B, 1, 1, 1) * noise.float()).to(dtype)}
            tr = Trainer.__new__(Trainer)
            tr.model = SimpleNamespace(uses_noise_schedule=lambda: True, PREDICTION_TYPE=PredictionTypes.FLOW_MATCHING)
            tr.noise_scheduler = sched
            tr.accelerator = SimpleNamespace(device=torch.device("cpu"))
            steps = []
            for eval_timestep in grid:
                # validation.py:5584-5591, as written there
                current = torch.Tensor([eval_timestep]).expand(prepared["noisy_latents"].shape[0]).to(dtype=world.config.weight_dtype, device=prepared["noisy_latents"].device)
                o = tr._prepare_custom_timestep_batch(prepared, current)
                steps.append(dict(grid_timestep=float(eval_timestep), given=current.clone(), timesteps=o["timesteps"].clone(), sigmas=o["sigmas"].clone(),
                                  noisy_latents=o["noisy_latents"].clone(), same_keys=sorted(k for k in o if o[k] is prepared.get(k))))
            out[f"{dn}.{grid_name}.T{T}"] = dict(dtype=str(dtype), grid=grid.clone(), latents=lat, noise=noise, prepared_timesteps=prepared["timesteps"],
                                                 prepared_sigmas=prepared["sigmas"], steps=steps)
    return out


def _would(world, Evaluation):
    runs = {}
    cases = {
        "steps3": (dict(eval_steps_interval=3), True, [dict(global_step=s) for s in range(0, 13)]),
        "steps3_resume4": (dict(eval_steps_interval=3), True, [dict(global_step=s, global_resume_step=4) for s in range(0, 13)]),
        "steps_str": (dict(eval_steps_interval="2"), True, [dict(global_step=s) for s in range(0, 6)]),
        "steps_bad": (dict(eval_steps_interval="soon", eval_epoch_interval=""), True, [dict(global_step=s) for s in range(0, 6)]),
        "steps_zero": (dict(eval_steps_interval=0, eval_epoch_interval="None"), True, [dict(global_step=s) for s in range(0, 6)]),
        "epoch_half": (dict(eval_epoch_interval=0.5, num_update_steps_per_epoch=4), True,
                       [dict(global_step=s, current_epoch=1 + (s - 1) // 4 if s else 1) for s in range(0, 13)]),
        "epoch_no_steps_per_epoch": (dict(eval_epoch_interval=0.5), True, [dict(global_step=s) for s in range(0, 6)]),
        "both": (dict(eval_steps_interval=5, eval_epoch_interval=1.0, num_update_steps_per_epoch=4), True,
                 [dict(global_step=s, current_epoch=1 + (s - 1) // 4 if s else 1) for s in range(0, 13)]),
        "epoch_schedule": (dict(eval_epoch_interval=1.0, num_update_steps_per_epoch=4, epoch_batches_schedule={1: 8, 2: 4}, gradient_accumulation_steps=2), True,
                           [dict(global_step=s, current_epoch=1 if s <= 4 else 2) for s in range(0, 12)]),
        "not_main": (dict(eval_steps_interval=1), False, [dict(global_step=s) for s in range(0, 4)]),
    }
    for name, (cfg, main, states) in cases.items():
        world.config = SimpleNamespace(**cfg)
        world.warnings.clear()
        ev = Evaluation(SimpleNamespace(is_main_process=main))
        answers = [bool(ev.would_evaluate(dict(s))) for s in states]
        runs[name] = dict(config=cfg, main=main, states=states, answers=answers, warnings=list(world.warnings))
    return runs


def _tables(world, Evaluation):
    world.config = SimpleNamespace(report_to="none")
    ev = Evaluation(SimpleNamespace(is_main_process=True))
    cases = {
        "pooled": {"pooled": {900.0: [0.5, 0.25], 500.0: [0.125, 1.0], 100.0: [2.0, 0.75]}},
        "two_sets": {"a": {900.0: [0.5], 100.0: [1.5]}, "b": {900.0: [0.25, 0.125, 4.0]}},
        "one_empty": {"a": {900.0: [0.5]}, "b": {}},
        "empty": {},
    }
    rec = {name: dict(given=t, table=ev.generate_tracker_table(all_accumulated_losses=t)) for name, t in cases.items()}
    rec["none"] = dict(given=None, table=ev.generate_tracker_table(all_accumulated_losses=None))
    off = Evaluation(SimpleNamespace(is_main_process=False))
    rec["not_main"] = dict(given=cases["pooled"], table=off.generate_tracker_table(all_accumulated_losses=cases["pooled"]))
    return rec


def _passes(world, Evaluation):
    rec = {}
    sets = {"a": [{"id": 0, "hw": (16, 16)}, {"id": 1, "hw": (16, 16)}, {"id": 2, "hw": (16, 16)}], "b": [{"id": 3, "hw": (16, 16)}, {"id": 4, "hw": (16, 16)}]}
    for pooling in (True, False):
        for cap in (None, 1, 2, 4, 9):
            world.config = SimpleNamespace(eval_timesteps=4, eval_dataset_pooling=pooling, num_eval_images=cap, weight_dtype=torch.bfloat16, report_to="none")
            world.sets = sets
            world.model = None
            world.reset_eval_datasets()
            ev = Evaluation(SimpleNamespace(is_main_process=True))
            seen = []

            def prepare_batch(raw):
                torch.rand(3)          # (a draw the pass must not leak into the training stream)
                return {"latents": torch.zeros(2, 4, *raw["hw"]), "noisy_latents": torch.zeros(2, 4, *raw["hw"]), "id": raw["id"]}

            def model_predict(prepared_batch, custom_timesteps=None):
                return {"id": prepared_batch["id"], "t": float(custom_timesteps[0])}

            def calculate_loss(prepared_batch, model_output, apply_conditioning_mask=True):
                seen.append((model_output["id"], model_output["t"], bool(apply_conditioning_mask), torch.is_grad_enabled()))
                return STUB["base"] * (1 + model_output["id"]) + STUB["scale"] * model_output["t"]

            from simpletuner_amd.sampling import FlowMatchEulerDiscreteScheduler, fix_flow_match_euler_schedule_bounds
            sched = fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=3.0))
            torch.manual_seed(1234)
            before = torch.get_rng_state().clone()
            acc = ev.execute_eval(prepare_batch=prepare_batch, model_predict=model_predict, calculate_loss=calculate_loss, get_prediction_target=None, noise_scheduler=sched)
            restored = bool(torch.equal(before, torch.get_rng_state()))
            flat = {name: sorted((float(t), float(v)) for t, vals in by_t.items() for v in vals) for name, by_t in acc.items()}
            rec[f"pooling{int(pooling)}.cap{cap}"] = dict(pooling=pooling, num_eval_images=cap, names=list(acc), entries=flat, seen=list(seen), rng_restored=restored,
                                                          table=ev.generate_tracker_table(all_accumulated_losses=acc))
    return dict(sets=sets, runs=rec)


def main():
    ref = Path(sys.argv[1])
    world = _World()
    Evaluation, Trainer, Foundation = _classes(ref, world)
    rec = dict(stub=STUB, schedule=_schedule(world, Evaluation, Foundation), custom_batch=_custom_batch(world, Evaluation, Trainer, Foundation),
               would=_would(world, Evaluation), table=_tables(world, Evaluation), passes=_passes(world, Evaluation))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(rec, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    c = rec["custom_batch"]["bf16.shift3.T28"]
    print("grid (fp32)        ", [round(float(t), 3) for t in c["grid"]])
    print("given (bf16)       ", [float(s["given"][0]) for s in c["steps"]])
    print("model timestep     ", [float(s["timesteps"][0]) for s in c["steps"]], c["steps"][0]["timesteps"].dtype)
    print("sigma              ", [float(s["sigmas"].flatten()[0]) for s in c["steps"]], c["steps"][0]["sigmas"].dtype, tuple(c["steps"][0]["sigmas"].shape))
    print("distinct model timesteps:", len({float(s["timesteps"][0]) for s in c["steps"]}), "of", len(c["steps"]))
    for k, v in rec["would"].items():
        print(k, v["answers"], v["warnings"])
    for k, v in rec["passes"]["runs"].items():
        print(k, v["names"], {n: len(e) for n, e in v["entries"].items()}, v["table"], "rng restored", v["rng_restored"])


if __name__ == "__main__":
    main()

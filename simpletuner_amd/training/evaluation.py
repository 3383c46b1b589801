"""Evaluation loss (`eval_steps_interval` / `eval_epoch_interval`): a held-out loss at a fixed timestep grid with fixed noise — the reference's "stable
evaluation loss" (helpers/training/validation.py `Evaluation`, trainer.py `_prepare_custom_timestep_batch` and its call site).  Imported only when an interval is
set and `eval_loss_disable` is false; Flux and SD3.

Per eval batch: ONE `prepare_batch` under the fixed eval noise stream, then for chunks of k = `eval_timestep_stack` timesteps: `ops.eval_flow_views` builds the k * B
noisy rows from one read of the latents and the noise, the [B, ...] conditioning tensors are repeated k times, ONE no-grad `model_predict` serves the k timesteps,
and `ops.eval_loss` writes the k losses straight into a device-resident table [batches, T].  The table is read on the host once, at the end of the pass.  k = 1 is
the reference's launch order.

Under `hip_graph` the pass runs eager between replays of the captured step: it allocates its own tensors (never the capture's static inputs, loss or gradient
buffers), and every scratch buffer it outgrows is retired, not freed (ops._scratch), so the addresses a captured graph holds stay valid.

Eval must not move training: the torch CPU / device RNG states, the plugin's Philox position (`_noise_step` / `_noise_offset`) and the `flow_custom_timesteps`
round-robin cursor are saved and restored around every pass, and the grid is set on a copy of the training schedule.
"""
from __future__ import annotations

import copy
import inspect
import logging
import math
from typing import Dict, Iterable, Optional

import torch

from .. import ops

logger = logging.getLogger(__name__)

EVAL_NOISE_SEED = 0x6576616C          # the eval noise stream's own Philox seed ("eval"), offset 0: the same noise for every batch and every eval
BUILT_FAMILIES = ("flux", "sd3")
# the keys of a prepared batch the pass builds itself (or that only the one-slab loss reads): never repeated along the batch axis
_OWN_KEYS = frozenset(("latents", "latent_batch", "noise", "input_noise", "noisy_latents", "flow_target", "target", "sigmas", "timesteps"))


def _interval(raw, kind):
    """validation.py:5363-5381: "" / "None" / unparsable / non-positive -> None"""
    if raw in ("", "None"):
        return None
    try:
        v = kind(raw)
    except (TypeError, ValueError):
        return None
    return v if v > 0 else None


def schedule_configured(config) -> bool:
    """an interval is set and `eval_loss_disable` is false (what makes the trainer import this module)"""
    if getattr(config, "eval_loss_disable", False):
        return False
    return _interval(getattr(config, "eval_steps_interval", None), int) is not None or _interval(getattr(config, "eval_epoch_interval", None), float) is not None


# `eval_timestep_stack` when the config does not set it: per family the smallest k whose pass was measured faster than k = 1 by more than the run-to-run spread
# (profiles/eval_loss_kernel_stats.md; a family without such a k keeps 1, the reference's launch order)
DEFAULT_TIMESTEP_STACK = {"sd3": 2, "flux": 2}


def timestep_stack(config) -> int:
    raw = getattr(config, "eval_timestep_stack", None)
    k = DEFAULT_TIMESTEP_STACK.get(str(getattr(config, "model_family", None)), 1) if raw is None else raw
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"eval_timestep_stack must be an integer >= 1, got {raw!r}")
    if k > ops.EVAL_MAX_STACK:
        raise ValueError(f"eval_timestep_stack={k}: at most {ops.EVAL_MAX_STACK} timesteps are stacked into one forward; set eval_timestep_stack<={ops.EVAL_MAX_STACK}")
    return k


def refuse_unbuilt(config, model, eval_sets) -> None:
    """Every configuration the no-grad stacked pass is not built for, refused by the flag's name and the value to set — never a silently different number."""
    steps, epochs = getattr(config, "eval_steps_interval", None), getattr(config, "eval_epoch_interval", None)
    flag = f"eval_steps_interval={steps}" if _interval(steps, int) is not None else f"eval_epoch_interval={epochs}"
    family = str(getattr(config, "model_family", None))
    flow = getattr(getattr(model, "PREDICTION_TYPE", None), "value", None) == "flow_matching"
    if family not in BUILT_FAMILIES or not flow:
        raise NotImplementedError(f"{flag}: the evaluation loss is not built for model_family={family} on the st355 path (built: flux, sd3) — the DDPM grid needs "
                                  "diffusers' DDPMScheduler.set_timesteps; unset eval_steps_interval and eval_epoch_interval, or set eval_loss_disable=true")
    if not eval_sets:
        raise ValueError(f"{flag}: no eval set was given — pass eval_sets={{name: batches}} to the Trainer (the reference's _type='eval' backends), "
                         "or set eval_loss_disable=true")
    timestep_stack(config)
    n = getattr(config, "eval_timesteps", 28)
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"eval_timesteps must be an integer >= 1, got {n!r}")
    why = "the reference's eval forwards are training-mode forwards that {}, which the no-grad route of the st355 path does not; not built"
    if (float(getattr(config, "lora_dropout", 0.0) or 0.0) > 0.0 and "lora" in str(getattr(config, "model_type", "lora"))
            and str(getattr(config, "lora_type", "standard") or "standard").lower() == "standard"):
        raise NotImplementedError(f"{flag} with lora_dropout={getattr(config, 'lora_dropout')}: " + why.format("drop") + "; set lora_dropout=0 or eval_loss_disable=true")
    tc = getattr(config, "tread_config", None)
    if tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)):
        raise NotImplementedError(f"{flag} with TREAD routing: " + why.format("route tokens") + "; unset tread_config or set eval_loss_disable=true")
    if getattr(config, "crepa_enabled", False):
        raise NotImplementedError(f"{flag} with crepa_enabled: the evaluation loss next to Self-Flow's views is not built on the st355 path; "
                                  "set crepa_enabled=false or eval_loss_disable=true")
    if getattr(config, "twinflow_enabled", False):
        raise NotImplementedError(f"{flag} with twinflow_enabled: the evaluation loss next to TwinFlow's signed times is not built on the st355 path; "
                                  "set twinflow_enabled=false or eval_loss_disable=true")
    if getattr(config, "distillation_method", None):
        raise NotImplementedError(f"{flag} with distillation_method={getattr(config, 'distillation_method')}: the evaluation loss of a distillation run is not built "
                                  "on the st355 path; unset distillation_method or set eval_loss_disable=true")
    try:
        offset = float(getattr(config, "scheduled_sampling_max_step_offset", 0) or 0)
    except Exception:
        offset = 0.0
    if offset > 0:
        raise NotImplementedError(f"{flag} with scheduled_sampling_max_step_offset={getattr(config, 'scheduled_sampling_max_step_offset')}: the reference's eval "
                                  "batches carry a rollout plan, which the stacked pass does not run; set scheduled_sampling_max_step_offset=0 or eval_loss_disable=true")
    if getattr(config, "scheduled_sampling_reflexflow", False):
        raise NotImplementedError(f"{flag} with scheduled_sampling_reflexflow: the reference's eval loss then carries the ReflexFlow terms, which the eval loss "
                                  "kernel does not compute; set scheduled_sampling_reflexflow=false or eval_loss_disable=true")
    if getattr(getattr(model, "xm_config", None), "enabled", False):
        raise NotImplementedError(f"{flag} with XM noise candidates: the eval forwards would expand every row into candidates; not built on the st355 path — "
                                  "disable the XM noise candidates or set eval_loss_disable=true")


def repeat_conditioning(prepared: dict, k: int, batch: int) -> dict:
    """a shallow copy of the prepared batch whose [B, ...] conditioning tensors (text embeds, pooled embeds, masks, ids, Kontext tokens, ...; nested dicts included)
    are repeated k times along the batch axis, slab-major like the views.  The keys the pass builds itself are left out."""
    def rep(v):
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == batch:
            return v if k == 1 else v.repeat(k, *([1] * (v.dim() - 1)))
        if isinstance(v, dict):
            return {n: rep(x) for n, x in v.items()}
        return v
    return {n: rep(v) for n, v in prepared.items() if n not in _OWN_KEYS}


def prepare_custom_timestep_batch(prepared: dict, custom_timesteps: torch.Tensor, num_train_timesteps: float = 1000.0, weight_dtype=torch.bfloat16) -> dict:
    """The flow-matching branch of trainer.py `_prepare_custom_timestep_batch`, dtype chain included, for a VECTOR of grid timesteps [K] (each the value the
    reference expands over the batch): the scheduler's timestep is cast to the weight dtype first (validation.py:5584-5591) and carried in the prepared
    timesteps' dtype; the sigma is formed (/ num_train_timesteps when any value exceeds 1) and clamped in the latents' dtype; the model's timestep is
    sigma * num_train_timesteps formed from THAT sigma in the latents' dtype, then cast back.  Returns {"given": the weight-dtype grid values [K],
    "sigmas": [K] in the latents' dtype, "timesteps": [K] in the prepared timesteps' dtype}; the noisy rows are ops.eval_flow_views' (fp32 arithmetic on that sigma, one rounding: the noising pass's rule, not the reference's
    three bf16 roundings)."""
    latents = prepared["latents"]
    ref_t = prepared.get("timesteps")
    ref_dtype = ref_t.dtype if torch.is_tensor(ref_t) else torch.float32
    custom = torch.as_tensor(custom_timesteps).to(dtype=weight_dtype).to(device=latents.device, dtype=ref_dtype)
    sigma = custom.to(dtype=latents.dtype)
    # the reference decides per call, i.e. per grid value: a value above 1 is a timestep, a value of at most 1 is taken AS a sigma and handed to the model unscaled
    # (kept: a grid that ends at timestep 1.0, the unshifted schedule's last value, evaluates sigma 1 there)
    is_t = sigma > 1.0
    sigma = torch.where(is_t, sigma / float(num_train_timesteps), sigma).clamp(0.0, 1.0)
    timesteps = torch.where(custom.detach().float() > 1.0, sigma * float(num_train_timesteps), sigma)
    return {"given": custom, "sigmas": sigma, "timesteps": timesteps.to(dtype=ref_dtype)}


class Evaluation:
    """validation.py `Evaluation`.  `eval_sets`: dict name -> re-iterable of raw batches (what SimpleTuner's `_type="eval"` backends / `retrieve_eval_images` hand
    out)."""

    def __init__(self, config, accelerator, eval_sets: Dict[str, Iterable[dict]]):
        self.config = config
        self.accelerator = accelerator
        self.eval_sets = dict(eval_sets or {})
        self._epoch_intervals_completed: Optional[int] = None
        self._warned_dual_schedule = False

    # ---- the schedule of evals (validation.py:5363-5466) ----
    def _step_interval(self):
        return _interval(getattr(self.config, "eval_steps_interval", None), int)

    def _epoch_interval(self):
        return _interval(getattr(self.config, "eval_epoch_interval", None), float)

    def _epoch_progress(self, state: dict, steps_per_epoch):
        current_epoch = state.get("current_epoch") or state.get("epoch") or 1
        try:
            global_step = float(state.get("global_step", 0))
            steps_per_epoch = float(steps_per_epoch)
            if steps_per_epoch <= 0:
                return None
            sched = getattr(self.config, "epoch_batches_schedule", None)
            if sched and isinstance(sched, dict):
                start = 0.0
                accum = max(getattr(self.config, "gradient_accumulation_steps", 1) or 1, 1)
                for e in range(1, int(current_epoch)):
                    start += math.ceil(sum(b for s, b in sched.items() if int(s) <= e) / accum)
            else:
                start = max(0.0, (float(current_epoch) - 1.0) * steps_per_epoch)
            return max(0.0, (float(current_epoch) - 1.0) + max(0.0, global_step - start) / steps_per_epoch)
        except (TypeError, ValueError) as exc:
            logger.warning(f"_epoch_progress calculation failed: {exc}")
            return None

    def _should_eval_epoch(self, state: dict, epoch_interval) -> bool:
        if epoch_interval is None:
            return False
        if state.get("global_step", 0) <= state.get("global_resume_step", 0):
            return False
        steps_per_epoch = getattr(self.config, "num_update_steps_per_epoch", None)
        if steps_per_epoch is None:
            return False
        progress = self._epoch_progress(state, steps_per_epoch)
        if progress is None:
            return False
        done = math.floor(progress / epoch_interval)
        if self._epoch_intervals_completed is None:
            self._epoch_intervals_completed = done
            return False
        if done > self._epoch_intervals_completed:
            self._epoch_intervals_completed = done
            return True
        return False

    def would_evaluate(self, state: dict) -> bool:
        if not self.accelerator.is_main_process:
            return False
        step_interval, epoch_interval = self._step_interval(), self._epoch_interval()
        if step_interval is None and epoch_interval is None:
            return False
        if step_interval is not None and epoch_interval is not None and not self._warned_dual_schedule:
            logger.warning("Both eval_steps_interval and eval_epoch_interval are set; evaluation will run on both schedules.")
            self._warned_dual_schedule = True
        global_step, resume_step = state.get("global_step", 0), state.get("global_resume_step", 0)
        by_step = False
        if step_interval is not None and step_interval > 0 and global_step > resume_step:
            by_step = global_step % step_interval == 0
        by_epoch = self._should_eval_epoch(state, epoch_interval)          # (evaluated on every call, like the reference: it keeps the interval count)
        return by_step or by_epoch

    # ---- the timestep grid (validation.py:5480-5496) ----
    def get_timestep_schedule(self, noise_scheduler, latents=None, model=None):
        accept_mu = "mu" in set(inspect.signature(noise_scheduler.set_timesteps).parameters.keys())
        kwargs = {}
        dynamic = getattr(noise_scheduler.config, "use_dynamic_shifting", False)
        if accept_mu and dynamic:
            mu = None
            if model is not None and hasattr(model, "calculate_dynamic_shift_mu"):
                mu = model.calculate_dynamic_shift_mu(noise_scheduler, latents)
            if mu is not None:
                kwargs["mu"] = mu
            elif dynamic:
                raise ValueError("Flow scheduler requires `mu` for dynamic shifting but none could be derived.")
        noise_scheduler.set_timesteps(getattr(self.config, "eval_timesteps", 28), **kwargs)
        return noise_scheduler.timesteps

    @staticmethod
    def noise_scheduler_of(model):
        """the plugin's training schedule (the reference passes `_get_noise_schedule()`), or — when it was never set up — one built the same way, without
        attaching it to the plugin"""
        sched = getattr(model, "noise_schedule", None)
        if sched is not None:
            return sched
        from ..sampling import FlowMatchEulerDiscreteScheduler, fix_flow_match_euler_schedule_bounds
        return fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=float(getattr(model.config, "flow_schedule_shift", None) or 1.0)))

    # ---- the pass ----
    def total_eval_batches(self, dataset_name=None):
        sets = self.eval_sets if dataset_name is None else {dataset_name: self.eval_sets.get(dataset_name, ())}
        total = 0
        for s in sets.values():
            total += len(s) if hasattr(s, "__len__") else sum(1 for _ in s)
        return total

    def _batches(self, dataset_name=None):
        for name, s in self.eval_sets.items():
            if dataset_name is None or name == dataset_name:
                yield from s

    def _evaluate_dataset_pass(self, dataset_name, model, noise_scheduler):
        """validation.py:5498-5623 for one dataset (or all of them, pooled).  Returns {timestep -> [losses]} as host floats, from ONE host read."""
        if not self.accelerator.is_main_process:
            return {}
        cfg = self.config
        total = self.total_eval_batches(dataset_name)
        cap = getattr(cfg, "num_eval_images", None)
        if cap is not None:
            total = min(int(cap), total)          # (the reference's quirk, kept: num_eval_images caps BATCHES)
        T = int(getattr(cfg, "eval_timesteps", 28))
        k = timestep_stack(cfg)
        if total <= 0:
            return {}
        dev = self.accelerator.device
        table = torch.zeros(total, T, dtype=torch.float32, device=dev)
        grids = []
        saved = _save_training_streams(model)
        sched = copy.copy(noise_scheduler)          # the grid is set on a copy: the training schedule's own timesteps stay
        T_train = float(getattr(noise_scheduler.config, "num_train_timesteps", 1000) or 1000)
        grid = grid_dev = None
        last_hw = None
        state = {"global_step": 0}
        try:
            for row, raw in enumerate(self._batches(dataset_name)):
                if row >= total:
                    break
                torch.manual_seed(0)
                model._noise_step, model._noise_offset, model._eval_noise_seed = 0, 0, EVAL_NOISE_SEED
                with torch.no_grad():
                    prepared = model.prepare_batch(dict(raw), state)
                if "latents" not in prepared:
                    raise ValueError("Error calculating eval batch: no 'latents' found.")
                lat = prepared["latents"]
                hw = tuple(lat.shape[-2:])
                if grid is None or hw != last_hw:
                    grid = self.get_timestep_schedule(sched, latents=lat, model=model)
                    grid_dev = prepare_custom_timestep_batch(prepared, grid, T_train, getattr(cfg, "weight_dtype", torch.bfloat16))
                    grid_dev["sigma32"] = grid_dev["sigmas"].to(device=dev, dtype=torch.float32).contiguous()
                    last_hw = hw
                    if grid.numel() != T:
                        raise ValueError(f"the scheduler returned {grid.numel()} timesteps for eval_timesteps={T}")
                grids.append(grid)
                self._evaluate_batch(model, prepared, grid_dev, table[row], k)
        finally:
            _restore_training_streams(model, saved)
        host = table.cpu()          # the pass's ONE host read
        out = {}
        for row, g in enumerate(grids):
            for j, t in enumerate(g.tolist()):
                out.setdefault(float(t), []).append(float(host[row, j]))
        return out

    def _evaluate_batch(self, model, prepared: dict, grid: dict, row: torch.Tensor, k: int) -> None:
        """T timesteps of one prepared batch in chunks of k: views -> repeated conditioning -> ONE no-grad forward -> k losses into `row`"""
        lat = prepared["latents"]
        noise = prepared.get("input_noise", prepared.get("noise"))
        B, T = lat.shape[0], row.numel()
        target = model.get_prediction_target(prepared)
        loss_type = getattr(self.config, "loss_type", "l2")
        if loss_type not in ops.LOSS_TYPES:
            raise NotImplementedError(f"Unsupported Loss Type {loss_type}")
        cond = {}
        with torch.no_grad():
            for lo in range(0, T, k):
                n = min(k, T - lo)
                views = ops.eval_flow_views(lat, noise, grid["sigma32"][lo:lo + n])
                if n not in cond:
                    cond[n] = repeat_conditioning(prepared, n, B)
                batch = dict(cond[n])
                batch["noisy_latents"] = views.view(n * B, *lat.shape[1:])
                batch["latents"] = batch["noisy_latents"]          # (model_predict reads only its shape)
                batch["timesteps"] = grid["timesteps"][lo:lo + n].repeat_interleave(B)
                batch["sigmas"] = grid["sigmas"][lo:lo + n].repeat_interleave(B).view(n * B, *([1] * (lat.dim() - 1)))
                pred = model.model_predict(batch)["model_prediction"]
                huber_c = None
                if loss_type != "l2":
                    huber_c = model.compute_scheduled_huber_c(batch["timesteps"]).to(device=pred.device, dtype=torch.float32).reshape(-1).contiguous()
                ops.eval_loss(pred.reshape(n, B, *lat.shape[1:]), target, loss_type, huber_c, loss_out=row[lo:lo + n])

    def execute_eval(self, model, noise_scheduler):
        """validation.py:5632-5691: one pooled pass, or one pass per dataset (the reference also collects a pooled table there and never returns it: kept)"""
        if not self.accelerator.is_main_process:
            return {}
        if len(self.eval_sets) == 0:
            return {}
        if getattr(self.config, "eval_dataset_pooling", False):
            return {"pooled": self._evaluate_dataset_pass(None, model, noise_scheduler)}
        accumulated = {}
        pooled_collector = {}
        for name in self.eval_sets.keys():
            losses = self._evaluate_dataset_pass(name, model, noise_scheduler)
            accumulated[name] = losses
            for t, vals in losses.items():
                pooled_collector.setdefault(t, []).extend(vals)
        return accumulated

    def generate_tracker_table(self, all_accumulated_losses: dict) -> dict:
        """validation.py:5693-5745: `loss/val/<name>` = the mean over all (timestep, batch) entries"""
        if not self.accelerator.is_main_process:
            return {}
        if all_accumulated_losses == {} or all_accumulated_losses is None:
            return {}
        results = {}
        for name, by_t in all_accumulated_losses.items():
            rows = [(t, v) for t, vals in by_t.items() for v in vals]
            if not rows:
                continue
            results[f"loss/val/{name}"] = sum(v for _, v in rows) / len(rows)
        return results


def _save_training_streams(model) -> dict:
    saved = {"cpu": torch.get_rng_state(), "noise_step": getattr(model, "_noise_step", 0), "noise_offset": getattr(model, "_noise_offset", 0),
             "cursor": getattr(model, "_flow_custom_timestep_cursor", None), "has_cursor": hasattr(model, "_flow_custom_timestep_cursor"),
             "resume": getattr(model, "_flow_custom_timestep_resume_step", None), "has_resume": hasattr(model, "_flow_custom_timestep_resume_step")}
    if torch.cuda.is_available():
        saved["device"] = torch.cuda.get_rng_state()
    import random
    saved["python"] = random.getstate()          # (the "fast" discrete schedule and random-range guidance draw from it)
    return saved


def _restore_training_streams(model, saved: dict) -> None:
    import random
    torch.set_rng_state(saved["cpu"])
    if "device" in saved:
        torch.cuda.set_rng_state(saved["device"])
    random.setstate(saved["python"])
    model._noise_step, model._noise_offset = saved["noise_step"], saved["noise_offset"]
    if hasattr(model, "_eval_noise_seed"):
        del model._eval_noise_seed
    for attr, has, val in (("_flow_custom_timestep_cursor", saved["has_cursor"], saved["cursor"]),
                           ("_flow_custom_timestep_resume_step", saved["has_resume"], saved["resume"])):
        if has:
            setattr(model, attr, val)
        elif hasattr(model, attr):
            delattr(model, attr)

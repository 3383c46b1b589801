"""Scheduled sampling for the flow-matching families (Flux, SD3), restating the reference's host logic:

    effective_probability      the probability ramp of ModelFoundation.prepare_batch          simpletuner/helpers/models/common.py:6013-6037
    build_rollout_schedule     the per-sample (target, source, offset) plan                    simpletuner/helpers/scheduled_sampling/plan.py
    flow_timestep_to_sigma     `_flow_timestep_to_sigma`                                       simpletuner/helpers/scheduled_sampling/rollout.py:54-67
    apply_flow_rollout         `_apply_flow_matching_rollout` (+ the ReflexFlow caches)        simpletuner/helpers/scheduled_sampling/rollout.py:70-199

The rollout is host-driven: per rolled sample one batch-1 forward per integer timestep through the plugin's own `model_predict`, under no_grad — the engines' route
that saves nothing, taps nothing (LayerSync, Internal Guidance, NextLat) and advances no counter of the step — and one fused Euler update (ops.flow_euler_step).
The start state is ops.flow_noise_mix.  The epsilon / v rollout (skrample's samplers) is not built: ModelFoundation refuses those families by the flag's name.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops

F32 = torch.float32


class ScheduledSamplingPlan:
    """What one step rolls: per sample the integer timestep it trains at (`target_timesteps`), the timestep its rollout starts from (`source_timesteps`, never
    below the target, never above T - 1) and the number of steps that were drawn for it (`rollout_steps`; 0 = left alone).  The three attribute names are the
    reference's, so a plan built on either side reads the same; the tensors are int64 [B]."""
    __slots__ = ("target_timesteps", "source_timesteps", "rollout_steps")

    def __init__(self, target_timesteps, source_timesteps, rollout_steps):
        self.target_timesteps, self.source_timesteps, self.rollout_steps = target_timesteps, source_timesteps, rollout_steps

    def on_host(self):
        """(steps, source, target) as python lists: one read for the whole batch"""
        return self.rollout_steps.tolist(), self.source_timesteps.tolist(), self.target_timesteps.tolist()


def effective_probability(config, global_step) -> float:
    """common.py:6015-6028, with its `or` idiom: an explicit prob_start / prob_end of 0.0 (or None) falls back to the plain probability, and with a ramp configured the
    value before `scheduled_sampling_start_step` is prob_start"""
    prob = float(getattr(config, "scheduled_sampling_probability", 0.0) or 0.0)
    start = float(getattr(config, "scheduled_sampling_prob_start", prob) or prob)
    end = float(getattr(config, "scheduled_sampling_prob_end", prob) or prob)
    ramp_steps = int(getattr(config, "scheduled_sampling_ramp_steps", 0) or 0)
    shape = getattr(config, "scheduled_sampling_ramp_shape", "linear") or "linear"
    ramp_start = int(getattr(config, "scheduled_sampling_start_step", 0) or 0)
    step = int(global_step or 0)
    if ramp_steps > 0 and step >= ramp_start:
        progress = min(1.0, max(0.0, (step - ramp_start) / max(ramp_steps, 1)))
        if shape == "cosine":
            progress = 0.5 - 0.5 * math.cos(math.pi * progress)
        return start + (end - start) * progress
    return start if ramp_steps > 0 else prob


def _training_timesteps(timesteps, count: int, T: int, device):
    """the integer timestep every sample trains at: the sampler's own timesteps with their fraction cut off, or (none given) a uniform draw over [0, T)"""
    if timesteps is None:
        return torch.randint(0, T, (count,), device=device)
    t = timesteps.to(device=device)
    if t.shape[0] != count:
        raise ValueError(f"scheduled sampling: the batch has {count} samples but the timesteps have shape {tuple(t.shape)}")
    return t.reshape(count).long()


def _eligible(count: int, probability, device):
    """which samples may be rolled: None = all of them (no probability, or one of at least 1: nothing is drawn then), else one Bernoulli draw per sample"""
    if probability is None or probability >= 1.0:
        return None
    return torch.bernoulli(torch.full((count,), probability, device=device)).bool()


def _squared_uniform(count: int, device):
    return torch.rand((count,), device=device) ** 2


# strategy -> int64 step counts in [0, limit]: flat, or the square of a uniform draw pushed toward 0 / toward the limit
_STEP_DRAWS = {
    "uniform": lambda count, limit, device: torch.randint(0, limit + 1, (count,), device=device),
    "biased_early": lambda count, limit, device: torch.round(_squared_uniform(count, device) * limit).to(torch.long),
    "biased_late": lambda count, limit, device: torch.round((1.0 - _squared_uniform(count, device)) * limit).to(torch.long),
}


def build_rollout_schedule(*, num_train_timesteps: int, batch_size: int, max_step_offset: int, device, base_timesteps: Optional[torch.Tensor] = None,
                           strategy: str = "uniform", apply_probability: Optional[float] = None) -> ScheduledSamplingPlan:
    """The plan of one step, with the reference's keyword interface and its random draws in its order (helpers/scheduled_sampling/plan.py; held to it draw for draw
    by tests/golden/scheduled_sampling_vectors.pt): the eligibility draw (only for a probability below 1) comes before the step-count draw of the strategy; a
    sample that is not eligible gets 0 steps; the start timestep is target + steps, capped at T - 1."""
    target = _training_timesteps(base_timesteps, batch_size, num_train_timesteps, device)
    if max_step_offset <= 0:
        return ScheduledSamplingPlan(target, target, torch.zeros_like(target))
    keep = _eligible(batch_size, apply_probability, device)
    draw = _STEP_DRAWS.get(strategy)
    if draw is None:
        raise ValueError(f"scheduled_sampling_strategy {strategy!r} is not built (one of: {', '.join(_STEP_DRAWS)})")
    steps = draw(batch_size, max_step_offset, device)
    if keep is not None:
        steps = torch.where(keep, steps, torch.zeros_like(steps))
    last = torch.full_like(target, num_train_timesteps - 1)
    return ScheduledSamplingPlan(target, torch.minimum(target + steps, last), steps)


def num_train_timesteps_of(noise_schedule) -> int:
    return int(getattr(getattr(noise_schedule, "config", None), "num_train_timesteps", 1000) or 1000)


def timestep_fraction(timestep, T: int) -> float:
    """t / (T - 1): where an integer timestep lies between the data (0) and the noise (1)"""
    return float(timestep) / max(float(T - 1), 1.0)


def flow_timestep_to_sigma(noise_schedule, timestep: int, num_train_timesteps: int) -> float:
    """The sigma recorded for a rolled sample (rollout.py's rule): entry int(t) of the schedule's `sigmas` table where the schedule has one that long — indexed by
    the timestep as it is, whatever order the table is in — and the linear t / (T - 1) otherwise (no table, a table too short, or one that cannot be read)."""
    index = int(timestep)
    table = getattr(noise_schedule, "sigmas", None)
    if table is not None:
        try:
            if index < len(table):
                return float(table[index])
        except (TypeError, ValueError, IndexError, RuntimeError):
            pass          # an unreadable table counts as no table
    return timestep_fraction(timestep, num_train_timesteps)


def rollout_window(offset: int, source_t: int, target_t: int, T: int):
    """the clamped (source, target) of one sample and whether it is rolled at all (rollout.py:108-112, 132)"""
    target_t = max(0, min(int(target_t), T - 1))
    source_t = max(0, min(int(source_t), T - 1))
    return source_t, target_t, not (int(offset) <= 0 or source_t <= target_t)


def _slice(model, prepared_batch: dict, i: int, noisy, timesteps) -> dict:
    """the batch-1 view of what the plugin's model_predict reads (its ROLLOUT_BATCH_KEYS), with the state and the timestep of this forward"""
    mini = {k: prepared_batch[k][i:i + 1] for k in model.ROLLOUT_BATCH_KEYS if torch.is_tensor(prepared_batch.get(k))}
    mini["noisy_latents"], mini["timesteps"] = noisy, timesteps
    return mini


def _predict(model, mini: dict):
    out = model.model_predict(mini)
    pred = out.get("model_prediction", out) if isinstance(out, dict) else out
    return pred.detach().contiguous()


@torch.no_grad()
def apply_flow_rollout(model, prepared_batch: dict, noise_schedule=None, config=None) -> dict:
    """rollout.py:70-199 on a flow-matching plugin.  Replaces noisy_latents / timesteps / sigmas of the rolled samples; with ReflexFlow on, leaves the clean and the
    biased prediction of every sample in the batch (`_reflexflow_clean_pred`, `_reflexflow_biased_pred`) and the pre-rollout tensors next to them.  The flow target is
    not touched."""
    plan = prepared_batch.get("scheduled_sampling_plan")
    if plan is None:
        return prepared_batch
    steps, src, tgt = getattr(plan, "rollout_steps", None), getattr(plan, "source_timesteps", None), getattr(plan, "target_timesteps", None)
    if steps is None or src is None or tgt is None:
        return prepared_batch
    config = model.config if config is None else config
    latents = prepared_batch["latents"]
    noise = prepared_batch.get("input_noise", prepared_batch.get("noise"))
    if noise is None:
        return prepared_batch
    dev, dtype = latents.device, latents.dtype
    base_noisy, base_t, base_s = prepared_batch["noisy_latents"], prepared_batch["timesteps"], prepared_batch.get("sigmas")
    T = num_train_timesteps_of(noise_schedule)
    reflex = bool(getattr(config, "scheduled_sampling_reflexflow", False))
    clean = torch.zeros_like(latents) if reflex else None
    biased = torch.zeros_like(latents) if reflex else None
    new_noisy, new_t = base_noisy.clone(), base_t.clone()
    new_s = base_s.clone() if base_s is not None else torch.zeros_like(base_t, dtype=dtype)
    steps, src, tgt = steps.tolist(), src.tolist(), tgt.tolist()          # the plan, read once on the host: the loop below is host-driven
    for i in range(latents.shape[0]):
        source_t, target_t, rolled = rollout_window(steps[i], src[i], tgt[i], T)
        if reflex:                                                        # the "clean" prediction at the unchanged state, always
            clean[i:i + 1] = _predict(model, _slice(model, prepared_batch, i, base_noisy[i:i + 1], base_t[i:i + 1]))
        if not rolled:
            if reflex:
                biased[i:i + 1] = clean[i:i + 1]
            continue
        ts = [t for t in range(source_t, target_t, -1) if t > 0]
        fr = [timestep_fraction(source_t, T)] + [timestep_fraction(max(target_t, t - 1), T) for t in ts]
        t_dev = torch.tensor([float(t) for t in ts] + [float(target_t)], device=dev).to(base_t.dtype)
        dt_dev = torch.tensor([fr[k + 1] - fr[k] for k in range(len(ts))] + [fr[0]], dtype=F32, device=dev)          # (last entry: the start sigma)
        current = ops.flow_noise_mix(latents[i:i + 1], dt_dev[-1:], noise=noise[i:i + 1], want_target=False)[0]
        for k in range(len(ts)):
            pred = _predict(model, _slice(model, prepared_batch, i, current, t_dev[k:k + 1]))
            ops.flow_euler_step(current, pred, dt_dev[k:k + 1])
        if reflex:                                                        # one more forward at the target state
            biased[i:i + 1] = _predict(model, _slice(model, prepared_batch, i, current, t_dev[-1:]))
        new_noisy[i:i + 1] = current
        new_t[i] = float(target_t)
        new_s[i] = flow_timestep_to_sigma(noise_schedule, target_t, T)
    prepared_batch["noisy_latents"], prepared_batch["timesteps"], prepared_batch["sigmas"] = new_noisy, new_t, new_s
    if reflex:
        prepared_batch["_reflexflow_clean_pred"], prepared_batch["_reflexflow_biased_pred"] = clean, biased
        prepared_batch["_reflexflow_pre_rollout_noisy"] = base_noisy
        prepared_batch["_reflexflow_pre_rollout_timesteps"] = base_t
        prepared_batch["_reflexflow_pre_rollout_sigmas"] = base_s
    return prepared_batch

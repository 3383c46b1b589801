"""TwinFlow (RCGM) few-step training for the flow-matching families (SD3, Flux), restating the reference's host logic:

    settings / validate        `_twinflow_settings`, `_validate_twinflow_config`, `_twinflow_active`      simpletuner/helpers/models/common.py:5412-5436, 5105-5140, 5399-5410
    sample_tt / cap_tt         `_twinflow_sample_tt`, `_prepare_twinflow_metadata`, the second cap        common.py:5459-5468, 5578-5601, 6521-6526
    time_schedule              the times of `_twinflow_rcgm_target`                                       common.py:5823-5841
    compute_losses             `_compute_twinflow_losses` (`_twinflow_enhance_target`, `_twinflow_rcgm_target`, `_twinflow_forward`)   common.py:6485-6629
    ucgm_sigmas / ucgm_sample  `TwinFlowScheduler.set_timesteps` / `.step`                                simpletuner/helpers/training/custom_schedule.py:1489-1692

Imported only when `twinflow_enabled` is set.  The teacher is the EMA copy of the adapters, read in place from the EMA's flat shadow (ArenaModule.teacher_values: the
masters are never written); its forwards go through the plugin's own `model_predict` under no_grad — the engines' route that saves nothing, taps nothing (LayerSync,
Internal Guidance, NextLat) and advances no counter of the step.  The per-sample times are [B] torch tensors on the device, evaluated in the dtypes the reference
has them in (the sigmas are cast to the weight dtype before the second cap, so that cap uses the weight dtype's eps and the times carry its rounding); the
[B, C, H, W] work is three kernels (ops.twinflow_rcgm_step, ops.twinflow_loss, ops.twinflow_ucgm_step)."""
from __future__ import annotations

import logging
from contextlib import contextmanager
from typing import List

import torch

from . import ops

F32 = torch.float32          # (the storage type is read as ops.BF16: this module binds no constant of its own)
logger = logging.getLogger(__name__)
_logged = set()

E_NOT_FLOW = ("TwinFlow requires flow-matching prediction_type. Enable diff2flow_enabled and twinflow_allow_diff2flow to bridge epsilon/v_prediction models "
              "explicitly.")
E_NO_EMA = "TwinFlow requires an EMA teacher; enable use_ema or set twinflow_allow_no_ema_teacher to fall back to student weights explicitly."
E_TEACHER_NO_EMA = "EMA teacher weights are required but unavailable; enable use_ema or allow fallback."


def _info_once(key: str, msg: str, *args):
    if key not in _logged:
        _logged.add(key)
        logger.info(msg, *args)


def settings(config) -> dict:
    """common.py:5412-5436: None and "" both mean the default; the order and the step count are floored at 1"""
    def get(name, default):
        v = getattr(config, name, None)
        return default if v is None or v == "" else v
    return {"estimate_order": max(1, int(get("twinflow_estimate_order", 2))), "enhanced_ratio": float(get("twinflow_enhanced_ratio", 0.5)),
            "target_step_count": max(1, int(get("twinflow_target_step_count", 1))), "delta_t": float(get("twinflow_delta_t", 0.01)),
            "clamp_target": float(get("twinflow_target_clamp", 1.0)), "require_ema": bool(getattr(config, "twinflow_require_ema", True)), "use_rng_state": True,
            "adversarial_enabled": bool(getattr(config, "twinflow_adversarial_enabled", False)), "adversarial_weight": float(get("twinflow_adversarial_weight", 1.0)),
            "rectify_weight": float(get("twinflow_rectify_weight", 1.0))}


def allow_student_teacher(config) -> bool:
    return bool(getattr(config, "twinflow_allow_no_ema_teacher", False))


def validate(config, flow_matching: bool) -> bool:
    """`_validate_twinflow_config` with its texts.  Returns whether the diff2flow bridge was asked for (an epsilon / v family with both bridge flags)."""
    if not getattr(config, "twinflow_enabled", False):
        return False
    bridge = False
    if not flow_matching:
        if not (bool(getattr(config, "twinflow_allow_diff2flow", False)) and bool(getattr(config, "diff2flow_enabled", False))):
            raise ValueError(E_NOT_FLOW)
        bridge = True
    if bool(getattr(config, "twinflow_require_ema", True)) and not getattr(config, "use_ema", False) and not allow_student_teacher(config):
        raise ValueError(E_NO_EMA)
    return bridge


def _has_routes(config) -> bool:
    tc = getattr(config, "tread_config", None)
    return bool(tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)))


def refuse_unbuilt(config, name: str, flow_matching: bool, built: bool) -> None:
    """one check for every plugin: the reference's ValueErrors first (`validate`), then what this path does not take, by the flag's name and the value to set"""
    bridge = validate(config, flow_matching)
    no = lambda what, to: NotImplementedError(f"twinflow_enabled {what} is not built on the st355 path; set {to}")
    if bridge or not built:
        flags = "with diff2flow_enabled + twinflow_allow_diff2flow (the diff2flow bridge) " if bridge else ""
        raise NotImplementedError(f"twinflow_enabled {flags}is not built for {name} on the st355 path (built: SD3, Flux); set --twinflow_enabled=false")
    if getattr(config, "twinflow_adversarial_enabled", False):
        raise no("with twinflow_adversarial_enabled (the adversarial and rectify terms need negative-time forwards and a trained sign embedding)",
                 "--twinflow_adversarial_enabled=false")
    if "lora" not in str(getattr(config, "model_type", "lora")):
        raise no(f"with model_type={getattr(config, 'model_type')} (under a full fine-tune the time-sign embedding table would be trainable)", "--model_type=lora")
    if str(getattr(config, "lora_type", "standard") or "standard").lower() != "standard":
        raise no(f"with lora_type={getattr(config, 'lora_type')} (the teacher forward packs standard LoRA operands from the EMA shadow)", "--lora_type=standard")
    v = getattr(config, "use_dora", False)
    if v.strip().lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v):
        raise no("with use_dora (the DoRA fold does not take the EMA shadow)", "--use_dora=false")
    p = float(getattr(config, "lora_dropout", 0.0) or 0.0)
    if p > 0.0:
        raise no(f"with lora_dropout={getattr(config, 'lora_dropout')} (the reference aligns the teacher's dropout masks by restoring the RNG state, which has no "
                 "counterpart here)", "--lora_dropout=0")
    if getattr(config, "hip_graph", False):
        raise no("with hip_graph (the two logs are read on the host every step)", "--hip_graph=false")
    if _has_routes(config):
        raise no("with TREAD routing (the teacher forwards of the no-grad route do not route tokens)", "tread_config without routes")
    if getattr(config, "mixflow_enabled", False) is True:
        raise no("with mixflow_enabled (MixFlow interpolates at a slowed time the RCGM integration does not know)", "--mixflow_enabled=false")
    if getattr(config, "controlnet", False):
        raise no("with controlnet (teacher forwards through controlnet_predict)", "--controlnet=false")
    if getattr(config, "distillation_method", None):
        raise no(f"with distillation_method={getattr(config, 'distillation_method')} (a distiller owns the step's loss)", "--distillation_method=None")


def drop_sign_embedding(state_dict):
    """A checkpoint's `time_sign_embed.weight` ([2, D], indexed by the sign of the time): zero-initialised and frozen under LoRA, so an all-zero table adds nothing and
    is dropped; a trained one would change every forward and is refused."""
    keys = [k for k in state_dict if k.endswith("time_sign_embed.weight")]
    if not keys:
        return state_dict
    for k in keys:
        if bool((state_dict[k] != 0).any()):
            raise NotImplementedError(f"twinflow_enabled with a checkpoint that carries a non-zero {k} (a trained time-sign embedding: the adversarial branch's product) "
                                      "is not built on the st355 path; set --twinflow_enabled=false or load the base checkpoint")
    return {k: v for k, v in state_dict.items() if k not in keys}


# ---- the per-sample times ([B]-sized torch ops on the device, in the reference's dtypes) ----
def _eps(dtype) -> float:
    return torch.finfo(dtype).eps if dtype.is_floating_point else 1e-4


def sample_tt(sigmas, uniforms=None):
    """site 1, `_twinflow_sample_tt`: tt = sigma - U sigma, floored at 0, then capped at sigma - eps(sigma's dtype) — which is negative for a sigma below eps"""
    u = torch.rand_like(sigmas) if uniforms is None else uniforms.to(device=sigmas.device, dtype=sigmas.dtype).view_as(sigmas)
    tt = sigmas - u * sigmas
    tt = torch.maximum(tt, torch.zeros_like(tt))
    return torch.minimum(tt, sigmas - _eps(sigmas.dtype))


def clamp_given_tt(tt, sigmas):
    """site 1 with a `twinflow_tt` already in the batch (common.py:5590-5591)"""
    tt = tt.to(device=sigmas.device).view_as(sigmas)
    return torch.minimum(torch.maximum(tt, torch.zeros_like(tt)), sigmas - _eps(sigmas.dtype))


def cap_tt(tt, sigmas, weight_dtype):
    """site 2 (common.py:6521-6526): the sigmas are cast to the weight dtype first, so the cap is sigma_w - eps(weight dtype), evaluated in that dtype; tt keeps
    its own dtype by promotion.  Returns (sigma_w in the weight dtype, tt)."""
    sw = sigmas.to(weight_dtype)
    if tt is None:
        tt = sample_tt(sw)
    return sw, torch.minimum(tt.view_as(sw), sw - _eps(sw.dtype))


def time_schedule(sigma_w, tt, order: int, delta: float) -> List[torch.Tensor]:
    """the t_next of every step of `_twinflow_rcgm_target` (common.py:5823-5841), in the reference's expression and dtypes"""
    steps = max(1, int(order))
    anchor = torch.maximum(tt, sigma_w - delta)
    out = []
    for i in range(steps - 1):
        frac = float(i + 1) / float(steps)
        out.append(anchor * frac + sigma_w * (1 - frac))
    out.append(tt)
    return out


def teacher_timesteps(s):
    """`_twinflow_forward`: the model sees |s| * 1000 (in s's dtype) — the sign travels apart and indexes a table that is frozen zeros under LoRA"""
    return (s.abs() * 1000.0).to(F32)


def prepare_metadata(batch: dict) -> None:
    """`_prepare_twinflow_metadata`, after the noisy latents exist: `twinflow_tt` in the sigmas' shape and dtype (fp32, on the device).  `twinflow_uniforms` (tests /
    parity runs inject the draw, like the noise) replaces torch's device RNG.  No RNG state is captured: nothing random runs in a teacher pass."""
    sigmas = batch.get("sigmas")
    if sigmas is None:
        return
    t = batch.get("timesteps")
    if getattr(t, "ndim", 1) != 1:
        raise NotImplementedError(f"twinflow_enabled with tokenwise timesteps {tuple(t.shape)} is not built on the st355 path (the RCGM times are per sample)")
    tt = batch.get("twinflow_tt")
    batch["twinflow_tt"] = sample_tt(sigmas, batch.get("twinflow_uniforms")) if tt is None else clamp_given_tt(tt, sigmas)


# ---- the teacher ----
@contextmanager
def teacher_context(model, st: dict):
    """`_twinflow_teacher_context` / `_ema_teacher_weights_context`: inside, the adapters' operands come from the EMA's flat shadow; the student's own weights only
    under the reference's two opt-out flags.  Yields whether the EMA is the teacher."""
    ema = getattr(model, "ema_model", None)
    has_ema = ema is not None and bool(getattr(model.config, "use_ema", False))
    if st["require_ema"] and not has_ema and not allow_student_teacher(model.config):
        raise ValueError(E_TEACHER_NO_EMA)
    if not has_ema:
        _info_once("student", "TwinFlow: no EMA model, the student's own weights are the teacher (twinflow_allow_no_ema_teacher / twinflow_require_ema=false)")
        yield False
        return
    shadow = getattr(ema, "shadow_flat", None)
    if shadow is None:
        raise NotImplementedError("twinflow_enabled: the EMA shadow is not one flat buffer over the adapter arena; not built on the st355 path")
    comp = model.unwrap_model(model.get_trained_component())
    with comp.teacher_values(shadow):
        yield True


def _predict(model, batch: dict):
    out = model.model_predict(batch)
    pred = out.get("model_prediction", out) if isinstance(out, dict) else out
    return pred.detach().to(ops.BF16).contiguous()


_STEP_KEYS = ("scheduled_sampling_plan", "_scheduled_sampling_rolled", "return_internal_guidance", "crepa_teacher_noisy_latents", "crepa_teacher_timesteps")


def teacher_forward(model, prepared_batch: dict, noisy, s):
    """`_twinflow_forward` under no_grad on a copy of the batch with noisy_latents / sigmas / timesteps replaced; s: [B] in any float dtype"""
    twin = {k: v for k, v in prepared_batch.items() if k not in _STEP_KEYS}
    twin["noisy_latents"] = noisy
    twin["sigmas"] = s.abs().to(F32).view(-1, *([1] * (noisy.dim() - 1)))
    twin["timesteps"] = teacher_timesteps(s.reshape(-1))
    with torch.no_grad():
        return _predict(model, twin)


def cfg_embeds(prepared_batch: dict):
    """`_twinflow_cfg_batches`: (positive, negative) or None"""
    neg = prepared_batch.get("negative_prompt_embeds")
    if neg is None:
        neg = prepared_batch.get("uncond_prompt_embeds")
    pos = prepared_batch.get("prompt_embeds")
    if pos is None:
        pos = prepared_batch.get("encoder_hidden_states")
    return None if neg is None or pos is None else (pos, neg)


def cfg_pair_forward(model, prepared_batch: dict, noisy, s, pos, neg):
    """teacher_cond and teacher_uncond of `_twinflow_enhance_target` as ONE forward at batch 2B, cond rows first (as Flow-DPO stacks its pairs)"""
    if tuple(neg.shape) != tuple(pos.shape):
        raise ValueError(f"twinflow_enabled: negative_prompt_embeds {tuple(neg.shape)} must have the shape of the prompt embeds {tuple(pos.shape)} (one 2B forward)")
    B = noisy.shape[0]
    neg = neg.to(device=pos.device, dtype=pos.dtype)
    double = {}
    for k in tuple(model.ROLLOUT_BATCH_KEYS):
        v = prepared_batch.get(k)
        if torch.is_tensor(v) and v.shape[0] == B:
            double[k] = torch.cat([v, v], dim=0)
    for k in ("prompt_embeds", "encoder_hidden_states"):
        if k in prepared_batch or k in double:
            double[k] = torch.cat([pos, neg], dim=0)
    s2 = torch.cat([s.reshape(-1), s.reshape(-1)], dim=0)
    out = teacher_forward(model, double, torch.cat([noisy, noisy], dim=0), s2)
    return out[:B], out[B:]


class _TwinFlowLossFn(torch.autograd.Function):
    """base + real velocity on the training prediction (ops.twinflow_loss), gradient from the same kernel pass; also returns the two terms [2]"""

    @staticmethod
    def forward(ctx, pred, target, acc, cond, uncond, ratio, clamp):
        to = lambda t: None if t is None else t.detach().to(ops.BF16)
        losses, dpred = ops.twinflow_loss(to(pred), to(target), acc, cond=to(cond), uncond=to(uncond), ratio=ratio, clamp=clamp, want_grad=True)
        ctx.save_for_backward(dpred)
        ctx.in_dtype = pred.dtype
        ctx.mark_non_differentiable(losses)
        return losses.sum().reshape(()), losses

    @staticmethod
    def backward(ctx, g, _glosses):
        (dpred,) = ctx.saved_tensors
        # g is the upstream scalar (1.0, or the loss scale); fold it without a host sync
        return ((dpred.float() * g).to(ctx.in_dtype) if g.numel() == 1 else dpred.to(ctx.in_dtype),) + (None,) * 6


def compute_losses(model, prepared_batch: dict, base_pred):
    """`_compute_twinflow_losses`: (twin term with autograd on `base_pred`, {"twinflow_base", "twinflow_realvel"} as host floats — ONE read)."""
    st = settings(model.config)
    latents, noise, noisy, sigmas = (prepared_batch.get(k) for k in ("latents", "noise", "noisy_latents", "sigmas"))
    if base_pred is None:
        raise ValueError("TwinFlow requires a model_prediction tensor.")
    if latents is None or noise is None or noisy is None:
        raise ValueError("TwinFlow requires latents, noise, sigmas, and noisy_latents in the prepared batch.")
    if sigmas is None:
        raise ValueError("TwinFlow requires sigmas in the prepared batch.")
    dev, wd = base_pred.device, model.config.weight_dtype
    B = noisy.shape[0]
    sig = sigmas.to(device=dev).reshape(B, -1)[:, 0]
    tt = prepared_batch.get("twinflow_tt")
    sw, tt = cap_tt(None if tt is None else tt.to(device=dev).reshape(B, -1)[:, 0], sig, wd)
    prepared_batch["twinflow_tt"] = tt.view(B, *([1] * (noisy.dim() - 1)))
    target = prepared_batch.get("flow_target")
    if target is None:
        target = ops.flow_noise_mix(latents, torch.zeros(B, dtype=F32, device=dev), noise=noise)[1]
    noisy = noisy.to(device=dev, dtype=ops.BF16)
    f32 = lambda t: t.to(F32).contiguous()
    cond = uncond = None
    with teacher_context(model, st):
        ratio = st["enhanced_ratio"]
        pair = cfg_embeds(prepared_batch) if ratio > 0.0 else None
        if pair is not None:
            cond, uncond = cfg_pair_forward(model, prepared_batch, noisy, sw, *pair)
        else:
            ratio = 0.0
            if st["enhanced_ratio"] > 0.0:
                _info_once("no_negative", "TwinFlow: twinflow_enhanced_ratio=%s but the batch carries no negative_prompt_embeds / uncond_prompt_embeds: the target is "
                           "not enhanced", st["enhanced_ratio"])
        x = noisy.clone()
        acc = torch.empty(noisy.shape, dtype=F32, device=dev)
        t_prev = sw
        for k, t_next in enumerate(time_schedule(sw, tt, st["estimate_order"], st["delta_t"])):
            fc = teacher_forward(model, prepared_batch, x, t_prev)
            ops.twinflow_rcgm_step(x, acc, fc, f32(t_prev), f32(t_next), first=(k == 0))
            t_prev = t_next
    loss, terms = _TwinFlowLossFn.apply(base_pred, target, acc, cond, uncond, ratio, st["clamp_target"])
    base, real = terms.tolist()
    return loss, {"twinflow_base": base, "twinflow_realvel": real}


# ---- the UCGM sampler (custom_schedule.py `TwinFlowScheduler`) ----
def ucgm_sigmas(num_inference_steps: int, time_dist_ctrl=(1.0, 1.0, 1.0), gap_start: float = 0.001, gap_end: float = 0.0) -> torch.Tensor:
    """`set_timesteps`: the Kumaraswamy-transformed grid in fp64, as 1 - t, with a final 0, rounded to fp32 ([steps + 1]).  gap_end 0 means the step-count default:
    0.6 up to 2 steps, 0.5 up to 4, 0.3 beyond."""
    n = int(num_inference_steps)
    if gap_end == 0.0:
        gap_end = 0.6 if n <= 2 else (0.5 if n <= 4 else 0.3)
    t = torch.linspace(gap_start, 1.0 - gap_end, n, dtype=torch.float64)
    a, b, c = time_dist_ctrl
    t = (1 - (1 - t ** a) ** b) ** c
    return torch.cat([1 - t, torch.zeros(1, dtype=torch.float64)]).to(F32)


def ucgm_sample(predict, latents, num_inference_steps: int, stochast_ratio: float = 1.0, generator=None, noises=None, on_step=None):
    """the sampling loop over `TwinFlowScheduler.step`: predict(x, t[B]) with t = sigma * 1000, one ops.twinflow_ucgm_step per grid entry, in place on a bf16 copy
    of `latents`.  `noises` (a list, one per step) replaces the Gaussian draw."""
    sig_t = ucgm_sigmas(num_inference_steps)
    sig, ts = sig_t.tolist(), (sig_t[:-1] * 1000.0).tolist()          # (the timesteps are the fp32 product, as `set_timesteps` forms them)
    x = latents.to(ops.BF16).contiguous().clone()
    rho = float(stochast_ratio)
    with torch.no_grad():
        for i in range(int(num_inference_steps)):
            t = torch.full((x.shape[0],), ts[i], dtype=F32, device=x.device)
            v = predict(x, t).to(ops.BF16).contiguous()
            noise = None
            if rho > 0.0:
                noise = noises[i] if noises is not None else torch.randn(x.shape, device=x.device, dtype=F32, generator=generator)
                noise = noise.to(device=x.device, dtype=ops.BF16).contiguous()
            ops.twinflow_ucgm_step(x, v, sig[i], sig[i + 1], rho, noise)
            if on_step is not None:
                on_step(i, x)
    return x

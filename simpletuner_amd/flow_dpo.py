"""Flow-DPO preference training (`distillation_method=flow_dpo`), restating the reference's host logic:

    method_config / merged_config     `DistillerFactory._method_config` + the distiller's `_DEFAULTS`       simpletuner/helpers/distillation/factory.py:48-53
    FlowDPODistiller                  the constructor's checks, `_validate_batch`, `_conditioning_latents`,
                                      `_build_rejected_batch`, `_mask_for_loss`, `compute_distill_loss`      simpletuner/helpers/distillation/flow_dpo/distiller.py
    adapter_dropout_override          `safety_check`'s lora_dropout override under a distillation method     simpletuner/helpers/training/default_settings/safety_check.py:23-49

LoRA-only, flow-matching-only: the frozen base under the adapters is the DPO reference model.  Where the reference runs four batch-B forwards per step (policy
preferred, policy rejected, and both again with the adapters off), this path runs TWO at batch 2B — rows [0, B) the preferred samples, [B, 2B) the rejected ones:
one training forward (one autograd node, one hand-written backward, one gradient exchange) and one no-grad forward under `component.lora_disabled()` on the
engines' route that saves nothing, taps nothing and advances no counter.  The loss is three kernels (ops.flow_dpo_stats / flow_dpo_head / flow_dpo_grad): the
margin is accumulated element by element as sum m (r - p)(r + p - 2 t), never as the difference of the four per-sample errors (which cancels at LoRA
initialisation, where policy ~ reference), the auto-beta EMA is one device-resident scalar, and the host reads the log vector once per step.
"""
from __future__ import annotations

import logging
import math
import os
from contextlib import nullcontext
from typing import Any, Dict, Optional

import torch

from . import ops

logger = logging.getLogger(__name__)

METHOD = "flow_dpo"
DEFAULTS: Dict[str, Any] = {
    "distillation_type": "flow_dpo", "beta": 1.0, "loss_weight": 1.0, "sft_loss_weight": 0.0, "anchor_alpha": 0.0, "norm_type": "sum", "mask_dilate": 0,
    "auto_beta": True, "auto_beta_target_gf": 0.2, "auto_beta_decay": 0.99, "auto_beta_min": 1e-3, "auto_beta_max": 1.0, "auto_beta_eps": 1e-6,
}
REQUIRED_KEYS = ("latents", "noise", "input_noise", "sigmas", "timesteps", "noisy_latents")
REFERENCE_IMAGE_KEYS = ("conditioning_packed_latents", "conditioning_ids")          # Kontext's reference-image tokens: never built from the rejected sample
DROPOUT_FORCE_ENV = "SIMPLETUNER_LORA_DROPOUT_FORCE_ENABLED"


def _cfg_get(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


def method_of(config) -> Optional[str]:
    """the configured distillation method as a lower-case name, None when unset ("", "none", "false", "0" included)"""
    m = _cfg_get(config, "distillation_method", None)
    m = getattr(m, "value", m)
    if m is None or str(m).strip().lower() in ("", "none", "false", "0"):
        return None
    return str(m).strip().lower()


def method_config(config, method: str = METHOD) -> Dict[str, Any]:
    """`distillation_config` as the factory resolves it: a dict, either flat or keyed by the method's name; anything else is no configuration"""
    configured = _cfg_get(config, "distillation_config", None)
    if not isinstance(configured, dict):
        return {}
    mc = configured.get(method, configured)
    return mc if isinstance(mc, dict) else {}


def merged_config(config) -> Dict[str, Any]:
    """the method's configuration laid over the distiller's defaults"""
    out = dict(DEFAULTS)
    out.update(method_config(config))
    return out


def adapter_dropout_override(config) -> float:
    """`lora_dropout` under a distillation method (safety_check.py:23-49): every reference implementation trains its adapters without dropout, so a configured
    value is overridden to 0.0 with the reference's warning.  SIMPLETUNER_LORA_DROPOUT_FORCE_ENABLED keeps the value in the reference; here a positive value under
    it is refused by name — the policy and the reference forward would draw different masks, a different computation."""
    current = _cfg_get(config, "lora_dropout", 0.0)
    method = _cfg_get(config, "distillation_method", None)
    if current != 0.0 and current is not None:
        if os.environ.get(DROPOUT_FORCE_ENV, "").strip().lower() in ("1", "true", "yes", "on"):
            if float(current) > 0.0:
                raise NotImplementedError(f"{DROPOUT_FORCE_ENV} with lora_dropout={current} under distillation_method={method}: the training forward and the "
                                          "adapters-off forward would draw different masks; not built on the st355 path — unset the variable or set --lora_dropout=0")
        else:
            logger.warning(f"{method} distillation reference implementations train adapters with lora_dropout=0.0; overriding --lora_dropout={current}. Set "
                           f"{DROPOUT_FORCE_ENV}=1 to keep the configured value. Adapter dropout also injects amplified noise into finite-difference "
                           "distillation targets.")
            if isinstance(config, dict):
                config["lora_dropout"] = 0.0
            else:
                setattr(config, "lora_dropout", 0.0)
    return float(_cfg_get(config, "lora_dropout", 0.0) or 0.0)


def _truthy(v) -> bool:
    return v.strip().lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v)


def refuse_unbuilt(config, model=None) -> None:
    """everything the two-forward step is not built for, by the flag's name — after the reference's own ValueErrors, never a silently different computation"""
    flag = "distillation_method=flow_dpo"
    if _cfg_get(config, "hip_graph", False):
        raise NotImplementedError(f"{flag} with hip_graph: the step reads its logs on the host every step and cannot be captured")
    tc = _cfg_get(config, "tread_config", None)
    if tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)):
        raise NotImplementedError(f"{flag} with TREAD routing: the reference's four forwards would each route their own token subset; not built on the st355 path")
    if getattr(getattr(model, "xm_config", None), "enabled", False) or _truthy(_cfg_get(config, "xm_noise_candidates_enabled", False)):
        raise NotImplementedError(f"{flag} with XM noise candidates is not built on the st355 path")
    try:
        offset = float(_cfg_get(config, "scheduled_sampling_max_step_offset", 0) or 0)
    except Exception:
        offset = 0.0
    if offset > 0 or _cfg_get(config, "scheduled_sampling_reflexflow", False):
        raise NotImplementedError(f"{flag} with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow): the rollout "
                                  "would re-time the preferred sample only; not built on the st355 path")
    for k, name in (("layersync_enabled", "LayerSync"), ("internal_guidance_enabled", "Internal Guidance"), ("nextlat_enabled", "NextLat")):
        if _cfg_get(config, k, False):
            raise NotImplementedError(f"{flag} with {k}: {name}'s taps would see the 2B rows of the doubled batch; not built on the st355 path")
    if _truthy(_cfg_get(config, "use_dora", False)):
        raise NotImplementedError(f"{flag} with use_dora: the adapters-off forward through the DoRA fold is not built on the st355 path; set --use_dora=false")
    if str(_cfg_get(config, "lora_type", "standard") or "standard").lower() == "lycoris":
        raise NotImplementedError(f"{flag} with lora_type=lycoris: the adapters-off forward through the LoKr fold is not built on the st355 path; set --lora_type=standard")
    if _cfg_get(config, "controlnet", False):
        raise NotImplementedError(f"{flag} with controlnet is not built on the st355 path")


def conditioning_latents(prepared_batch: Dict[str, Any]) -> torch.Tensor:
    """the rejected sample of every pair: `conditioning_latents`, or its `reference_strict` entry in the list form"""
    latents = prepared_batch["conditioning_latents"]
    if isinstance(latents, list):
        types = prepared_batch.get("conditioning_latents_type")
        if isinstance(types, list) and "reference_strict" in types:
            latents = latents[types.index("reference_strict")]
        elif len(latents) == 1:
            latents = latents[0]
        else:
            raise ValueError("Flow-DPO requires one reference_strict conditioning latent set.")
    if not torch.is_tensor(latents):
        raise ValueError("Flow-DPO conditioning_latents must be a tensor.")
    return latents


def validate_batch(prepared_batch: Dict[str, Any]) -> None:
    if prepared_batch.get("conditioning_type") != "reference_strict":
        raise ValueError("Flow-DPO requires a rejected-sample conditioning dataset with conditioning_type=reference_strict.")
    cl = prepared_batch.get("conditioning_latents")
    if cl is None or (isinstance(cl, list) and not cl):
        raise ValueError("Flow-DPO requires conditioning_latents from the rejected-sample dataset.")
    missing = [k for k in REQUIRED_KEYS if k not in prepared_batch or prepared_batch[k] is None]
    if missing:
        raise ValueError(f"Flow-DPO prepared batch is missing required fields: {', '.join(missing)}.")


def mask_for_loss(prepared_batch: Dict[str, Any], prediction: torch.Tensor, mask_dilate: int = 0) -> Optional[torch.Tensor]:
    """The distiller's own `_mask_for_loss` (not the plugin's `_conditioning_loss_mask`): the last `conditioning_pixel_values` entry, its first channel ("mask") or its
    channel mean ("segmentation": divided by the channel count), area-resized to the latent grid, mapped from [-1, 1] to [0, 1] and CLAMPED there, binarised for
    "segmentation", then dilated by a (2 d + 1)^2 max-pool.  Returns the fp32 [B, H*W] element mask the kernels broadcast over the channels, or None.  (Input
    preparation of a one-channel image, done with torch as the existing mask is.)"""
    kind = prepared_batch.get("loss_mask_type")
    if kind not in ("mask", "segmentation"):
        return None
    img = prepared_batch.get("conditioning_pixel_values")
    if isinstance(img, list):
        if not img:
            return None
        img = img[-1]
    if not torch.is_tensor(img):
        raise ValueError("Flow-DPO loss masking requires conditioning_pixel_values to be a tensor.")
    if prediction.dim() != 4:
        raise NotImplementedError("distillation_method=flow_dpo: loss masks are built for [B, C, H, W] predictions")
    img = img.to(device=prediction.device, dtype=prediction.dtype)          # (the reference casts the image to the prediction's dtype first)
    if img.dim() == 3:
        img = img.unsqueeze(1)
    if img.dim() == 4:
        if kind == "segmentation":
            img = torch.sum(img, dim=1, keepdim=True) / img.shape[1]
        elif img.shape[1] > 1:
            img = img[:, 0:1]
    if img.dim() != prediction.dim():
        raise ValueError(f"Flow-DPO mask rank must match prediction rank. Got {img.dim()} vs {prediction.dim()}.")
    m = torch.nn.functional.interpolate(img, size=prediction.shape[2:], mode="area")
    m = (m / 2 + 0.5).clamp(0.0, 1.0)
    if kind == "segmentation":
        m = (m > 0).to(dtype=prediction.dtype)
    d = int(mask_dilate or 0)
    if d > 0:
        m = torch.nn.functional.max_pool2d(m, kernel_size=2 * d + 1, stride=1, padding=d)
    return m.to(torch.float32).reshape(m.shape[0], -1).contiguous()


class _FlowDPOFn(torch.autograd.Function):
    """the Flow-DPO loss over the 2B prediction: stats + head in the forward, the gradient kernel in the backward (one bf16 write, the upstream gradient folded on
    the device).  Also returns the head's log vector (non-differentiable)."""

    @staticmethod
    def forward(ctx, policy, ref, target_w, target_l, emask, original_loss, d):
        bf = ops.BF16
        p_, r_ = policy.detach().to(bf), ref.detach().to(bf)
        tw, tl = target_w.detach().to(bf), target_l.detach().to(bf)
        B = tw.shape[0]
        n = tw.numel() // B
        stats = ops.flow_dpo_stats(p_, r_, tw, tl, emask)
        orig = None if original_loss is None else original_loss.detach().to(torch.float32).reshape(1)
        loss, pair, logs = ops.flow_dpo_head(stats, n, norm_type=d.norm_type, has_mask=emask is not None, beta=d.beta, loss_weight=d.loss_weight,
                                             anchor_alpha=d.anchor_alpha, ema_state=d.ema_state_for(p_.device), auto_num=d.auto_num, decay=d.decay,
                                             beta_min=d.beta_min, beta_max=d.beta_max, eps=d.eps, original_loss=orig, sft_weight=d.sft_loss_weight,
                                             reduce_absmean=d.reduce_absmean)
        ctx.save_for_backward(p_, r_ if d.anchor_alpha != 0.0 else None, tw, tl, emask, pair)
        ctx.anchor_alpha = d.anchor_alpha
        ctx.mark_non_differentiable(logs)
        return loss.reshape(()), logs

    @staticmethod
    def backward(ctx, g, _glogs):
        p_, r_, tw, tl, emask, pair = ctx.saved_tensors
        dpred = ops.flow_dpo_grad(p_, r_, tw, tl, pair, emask, anchor_alpha=ctx.anchor_alpha, upstream=g.detach().to(torch.float32).reshape(1))
        return dpred, None, None, None, None, None, None


class FlowDPODistiller:
    """`FlowDPODistiller(model_plugin)`: the plugin is teacher and student (low-rank distillation).  The Trainer's seams, in the order the reference calls them:
    `prepare_batch` (after the plugin's), `policy_batch` -> the plugin's `model_predict` at batch 2B, `compute_distill_loss`, `generator_loss_step`."""

    def __init__(self, model, config: Optional[Dict[str, Any]] = None, noise_scheduler=None):
        from .foundation import PredictionTypes
        self.model = self.teacher_model = self.student_model = model
        self.noise_scheduler = noise_scheduler
        mcfg = model.config
        self.config = merged_config(mcfg) if config is None else {**DEFAULTS, **config}
        self.config["model_type"] = _cfg_get(mcfg, "model_type", "lora")
        if model.PREDICTION_TYPE is not PredictionTypes.FLOW_MATCHING:
            raise ValueError("Flow-DPO requires a flow-matching model.")
        if self.config.get("model_type") != "lora":
            raise ValueError("Flow-DPO only supports low-rank LoRA/LyCORIS training.")
        norm_type = str(self.config.get("norm_type", "sum")).lower()
        if norm_type not in ops.FLOW_DPO_NORMS:
            raise ValueError("Flow-DPO norm_type must be one of: sum, mean, masked_mean.")
        self.config["norm_type"] = self.norm_type = norm_type
        target_gf = float(self.config.get("auto_beta_target_gf", 0.0) or 0.0)
        if bool(self.config.get("auto_beta", True)) and target_gf >= 0.5:
            raise ValueError("Flow-DPO auto_beta_target_gf must be less than 0.5.")
        refuse_unbuilt(mcfg, model)
        if getattr(model, "ROLLOUT_BATCH_KEYS", None) is None:
            raise NotImplementedError(f"distillation_method=flow_dpo is not built for {getattr(model, 'NAME', type(model).__name__)} on the st355 path (built: Flux, SD3)")
        c = self.config
        self.beta = float(c.get("beta", 1.0))
        self.loss_weight = float(c.get("loss_weight", 1.0))
        self.sft_loss_weight = float(c.get("sft_loss_weight", 0.0) or 0.0)
        self.anchor_alpha = float(c.get("anchor_alpha", 0.0) or 0.0)
        self.mask_dilate = int(c.get("mask_dilate", 0) or 0)
        self.auto = bool(c.get("auto_beta", True)) and target_gf > 0.0
        self.eps = float(c.get("auto_beta_eps", 1e-6))
        self.decay = float(c.get("auto_beta_decay", 0.99))
        self.beta_min = None if c.get("auto_beta_min") is None else float(c["auto_beta_min"])
        self.beta_max = None if c.get("auto_beta_max") is None else float(c["auto_beta_max"])
        t = min(max(target_gf, self.eps), 1.0 - self.eps)
        self.auto_num = -2.0 * math.log(t / (1.0 - t)) if self.auto else 0.0
        self._ema_state = None          # fp32 [2] on the device: (margin EMA, initialised).  Not checkpointed: as in the reference, a resumed run starts it afresh

    # ---- the auto-beta state ----
    def ema_state_for(self, device):
        if not self.auto:
            return None
        if self._ema_state is None or self._ema_state.device != device:
            self._ema_state = torch.zeros(2, dtype=torch.float32, device=device)
        return self._ema_state

    @property
    def margin_ema(self) -> Optional[float]:
        """the EMA of mean |margin| as a host number (a read; None before the first step) — for tests and inspection, the step never calls it"""
        if self._ema_state is None:
            return None
        ema, init = self._ema_state.tolist()
        return ema if init else None

    @property
    def reduce_absmean(self):
        """world size > 1: the rank mean of the device scalar mean_b |margin_b|, one all_reduce between the head's two launches"""
        acc = getattr(self.model, "accelerator", None)
        world = int(getattr(acc, "num_processes", 1) or 1)
        if world <= 1:
            return None
        import torch.distributed as dist

        def reduce(t):
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            t.div_(world)
        return reduce

    # ---- the seams ----
    def prepare_batch(self, prepared_batch: Dict[str, Any], model=None, state=None) -> Dict[str, Any]:
        """after the plugin's prepare_batch: the batch contract, then the rejected input (1 - sigma) lose + sigma input_noise and both bf16 targets from
        ops.flow_noise_mix, and the doubled batch of the two forwards under `_flow_dpo`"""
        if not prepared_batch:
            return prepared_batch
        validate_batch(prepared_batch)
        win = prepared_batch["latents"]
        t = prepared_batch["timesteps"]
        if getattr(t, "ndim", 1) != 1:
            raise NotImplementedError(f"distillation_method=flow_dpo with tokenwise timesteps {tuple(t.shape)}: the margin is per sample; not built on the st355 path")
        lose = conditioning_latents(prepared_batch).to(device=win.device, dtype=win.dtype)
        if lose.shape != win.shape:
            raise ValueError(f"Flow-DPO rejected latents must match preferred latents. Got {lose.shape} vs {win.shape}.")
        B = win.shape[0]
        sig = prepared_batch["sigmas"].to(device=win.device, dtype=torch.float32).reshape(B).contiguous()
        lose_noisy, _, _ = ops.flow_noise_mix(lose.contiguous(), sig, noise=prepared_batch["input_noise"], want_target=False)
        zero = torch.zeros_like(sig)
        target_w = prepared_batch.get("flow_target")          # noise - latents, rounded to bf16 once: the plugin's prepare_batch already has it
        if target_w is None:
            _, target_w, _ = ops.flow_noise_mix(win, zero, noise=prepared_batch["noise"])
        _, target_l, _ = ops.flow_noise_mix(lose.contiguous(), zero, noise=prepared_batch["noise"])
        m = self.model
        double = {}
        for k in tuple(m.ROLLOUT_BATCH_KEYS) + ("timesteps", "sigmas"):
            v = prepared_batch.get(k)
            if k in REFERENCE_IMAGE_KEYS or not torch.is_tensor(v):
                continue
            double[k] = torch.cat([v, v], dim=0)
        double["latents"] = torch.cat([win, lose], dim=0)
        double["noisy_latents"] = torch.cat([prepared_batch["noisy_latents"], lose_noisy], dim=0)
        prepared_batch["_flow_dpo"] = dict(batch=double, target_w=target_w, target_l=target_l, pairs=B)
        return prepared_batch

    def policy_batch(self, prepared_batch: Dict[str, Any]) -> Dict[str, Any]:
        """a fresh shallow copy of the doubled batch (plugins may replace entries of the dict they are given: Flux divides `timesteps` by 1000)"""
        return dict(prepared_batch["_flow_dpo"]["batch"])

    def preferred_output(self, model_output):
        """the preferred rows of the 2B prediction, as the model output the plugin's own loss() takes"""
        B = model_output["model_prediction"].shape[0] // 2
        return {"model_prediction": model_output["model_prediction"][:B]}

    def original_loss(self, prepared_batch, model_output):
        """the plugin's own loss() on the preferred rows: with gradient only when sft_loss_weight != 0 (autograd then sums the two contributions to the 2B
        prediction's gradient), else without, for the log"""
        with (nullcontext() if self.sft_loss_weight != 0.0 else torch.no_grad()):
            return self.model.loss(prepared_batch, self.preferred_output(model_output), apply_conditioning_mask=True)

    def reference_prediction(self, prepared_batch: Dict[str, Any]) -> torch.Tensor:
        """ONE no-grad forward at batch 2B with the adapters off"""
        comp = self.model.unwrap_model(self.model.get_trained_component())
        with torch.no_grad(), comp.lora_disabled():
            out = self.model.model_predict(self.policy_batch(prepared_batch))
        return out["model_prediction"].detach()

    def compute_distill_loss(self, prepared_batch: Dict[str, Any], model_output, original_loss: torch.Tensor):
        """(loss, logs): model_output is the 2B policy prediction, original_loss the plugin's loss on the preferred rows"""
        st = prepared_batch.get("_flow_dpo")
        if st is None:
            raise RuntimeError("distillation_method=flow_dpo: the batch did not pass through the distiller's prepare_batch (Trainer.train_step calls it)")
        policy = model_output["model_prediction"]
        if policy.shape[0] != 2 * st["pairs"]:
            raise RuntimeError(f"distillation_method=flow_dpo: the policy prediction has {policy.shape[0]} rows, expected the doubled batch's {2 * st['pairs']}")
        ref = self.reference_prediction(prepared_batch)
        emask = mask_for_loss(prepared_batch, policy[:st["pairs"]], self.mask_dilate)
        loss, logv = _FlowDPOFn.apply(policy, ref, st["target_w"], st["target_l"], emask, original_loss, self)
        if self.sft_loss_weight != 0.0:
            loss = loss + original_loss * self.sft_loss_weight
        vals = logv.tolist()                                                  # the step's one host read
        logs = {k: vals[i] for i, k in enumerate(ops.FLOW_DPO_LOGS[:12])}
        if self.anchor_alpha != 0.0:
            logs["flow_dpo_anchor_loss"] = vals[12]
        return loss, logs

    def generator_loss_step(self, prepared_batch, model_output, current_loss):
        return current_loss, {}


def create_distiller(model):
    """the Trainer's factory seam: None without a method, the distiller for flow_dpo, every other method refused by name"""
    method = method_of(model.config)
    if method is None:
        return None
    if method != METHOD:
        raise NotImplementedError(f"distillation_method={method}: not built on the st355 path (built: flow_dpo)")
    return FlowDPODistiller(model)

"""Self-Transcendence (`distillation_method=self_transcendence`; the reference's helpers/distillation/self_transcendence/distiller.py, documented in
documentation/experimental/SELF_TRANSCENDENCE.md), restated for the st355 path.  Imported only when the method is named.

A 3-layer SiLU MLP projector reads a shallow block's image-token output.  Stage `vae` trains it to the patchified diffusion target; stage `self` trains it to the
feature-space CFG target u + cfg_scale (c - u) of a frozen teacher snapshot.  The loss is the mean over the samples with timestep_min <= sigma_b <= timestep_max of
the per-sample mean squared error, added to the plugin's loss with `weight` behind `auxiliary_loss`; from `stop_step` on nothing of it runs.

What lives where: the projector, its kernels' sequencing and the tap in engine.py (SelfTranscendenceHead / SelfTranscendenceTap, csrc/self_transcendence.hip); the
arena tail and the forward's keyword arguments in sd3/transformer.py (`set_self_transcendence`); here the configuration rule with the reference's texts, what this
path refuses by name, the teacher snapshot and its ONE no-grad forward at batch 2B, and the distiller object the Trainer drives.  Deviations: DESIGN.md §7."""
import logging
import os
from typing import Any, Dict, Optional

import torch

from .flow_dpo import _cfg_get, _truthy, method_config, method_of

logger = logging.getLogger("SelfTranscendenceDistiller")

METHOD = "self_transcendence"
VALID_STAGES = ("vae", "self")
DEFAULTS: Dict[str, Any] = {"stage": "vae", "student_block": None, "teacher_block": None, "weight": 0.5, "cfg_scale": 30.0, "timestep_min": 0.4, "timestep_max": 0.7,
                            "stop_step": 0, "projector_hidden_dim": 2048, "teacher_adapter_path": None}
BUILT = "built: SD3 LoRA"


def normalized_config(config: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """distiller.py `_normalized_config`: the defaults, the casts and every ValueError in the reference's order and with its texts"""
    n = dict(DEFAULTS)
    n.update(config or {})
    n["stage"] = str(n["stage"]).strip().lower()
    if n["stage"] not in VALID_STAGES:
        raise ValueError("Self-Transcendence stage must be either 'vae' or 'self'.")
    if n["student_block"] is None:
        raise ValueError("Self-Transcendence requires student_block.")
    if n["stage"] == "self" and n["teacher_block"] is None:
        raise ValueError("Self-Transcendence self stage requires teacher_block.")
    n["student_block"] = int(n["student_block"])
    if n["teacher_block"] is not None:
        n["teacher_block"] = int(n["teacher_block"])
    if n["student_block"] < 0 or (n["teacher_block"] is not None and n["teacher_block"] < 0):
        raise ValueError("Self-Transcendence block indices must be zero-based non-negative integers.")
    n["weight"] = float(n["weight"])
    n["cfg_scale"] = float(n["cfg_scale"])
    n["timestep_min"] = float(n["timestep_min"])
    n["timestep_max"] = float(n["timestep_max"])
    n["stop_step"] = int(n["stop_step"] or 0)
    n["projector_hidden_dim"] = int(n["projector_hidden_dim"])
    path = n.get("teacher_adapter_path")
    n["teacher_adapter_path"] = str(path).strip() if path else None
    if n["weight"] <= 0:
        raise ValueError("Self-Transcendence weight must be greater than zero.")
    if n["cfg_scale"] < 1:
        raise ValueError("Self-Transcendence cfg_scale must be at least 1.0.")
    if not 0 <= n["timestep_min"] < n["timestep_max"] <= 1:
        raise ValueError("Self-Transcendence timestep range must satisfy 0 <= min < max <= 1.")
    if n["stop_step"] < 0:
        raise ValueError("Self-Transcendence stop_step must be non-negative.")
    if n["projector_hidden_dim"] <= 0:
        raise ValueError("Self-Transcendence projector_hidden_dim must be greater than zero.")
    return n


def settings_of(config) -> Dict[str, Any]:
    """the run configuration's `distillation_config` (flat, or keyed by the method's name), normalised"""
    return normalized_config(method_config(config, METHOD))


def is_named(config) -> bool:
    return method_of(config) == METHOD


def training_batch_requirements(config: Dict[str, Any]) -> set:
    """distiller.py `training_batch_requirements`: stage `self` needs the cached empty-prompt embeddings in every batch"""
    return {"unconditional_text_embeddings"} if normalized_config(config)["stage"] == "self" else set()


def refuse_unbuilt(config, model) -> None:
    """distiller.py `prepare_model_for_adapter`'s ValueErrors with their texts, then everything this path does not take, by the method's name"""
    from .foundation import ModelTypes
    flag = f"distillation_method={METHOD}"
    if getattr(model, "MODEL_TYPE", None) is not ModelTypes.TRANSFORMER:
        raise ValueError("Self-Transcendence supports diffusion transformer model families, not UNet models.")
    model_type = str(_cfg_get(config, "model_type", "lora") or "lora").lower()
    if "lora" in model_type and str(_cfg_get(config, "lora_type", "standard") or "standard").lower() == "lycoris":
        raise ValueError("Self-Transcendence supports full-model and standard PEFT LoRA training; LyCORIS is not supported.")
    no = lambda what: NotImplementedError(f"{flag} {what} is not built on the st355 path ({BUILT})")
    if not getattr(model, "SELF_TRANSCENDENCE_BUILT", False):
        raise NotImplementedError(f"{flag} is not built for {getattr(model, 'NAME', type(model).__name__)} on the st355 path ({BUILT})")
    if model_type != "lora":
        raise no(f"with model_type={model_type} (a full fine-tune needs a separate frozen copy of the model as the teacher)")
    if _truthy(_cfg_get(config, "use_dora", False)):
        raise no("with use_dora (the teacher forward packs standard LoRA operands from the snapshot, which the DoRA fold does not take)")
    if _cfg_get(config, "hip_graph", False):
        raise no("with hip_graph (the step reads its logs on the host every step and cannot be captured)")
    tc = _cfg_get(config, "tread_config", None)
    if tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)):
        raise no("with TREAD routing (the routed block's token count no longer matches the target's)")
    if _truthy(_cfg_get(config, "crepa_enabled", False)):
        raise no("with crepa_enabled (Self-Flow's tokenwise timesteps; the same arena tail)")
    if getattr(getattr(model, "xm_config", None), "enabled", False) or _truthy(_cfg_get(config, "xm_noise_candidates_enabled", False)):
        raise no("with XM noise candidates")
    try:
        offset = float(_cfg_get(config, "scheduled_sampling_max_step_offset", 0) or 0)
    except Exception:
        offset = 0.0
    if offset > 0 or _cfg_get(config, "scheduled_sampling_reflexflow", False):
        raise no("with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow: the rollout re-times the samples the mask reads)")
    if _truthy(_cfg_get(config, "twinflow_enabled", False)):
        raise no("with twinflow_enabled")
    for k, name in (("layersync_enabled", "LayerSync"), ("internal_guidance_enabled", "Internal Guidance"), ("nextlat_enabled", "NextLat")):
        if _cfg_get(config, k, False):
            raise no(f"with {k} ({name} claims the same arena tail or tap order)")
    if _cfg_get(config, "controlnet", False):
        raise no("with controlnet")


class SelfTranscendenceDistiller:
    """The object the Trainer drives: `pre_training_step(model, step)` ahead of every micro-step (the early stop, and in stage `self` the teacher snapshot at the first
    one), `forward_inputs(model, batch)` from the plugin's training forward (what the engine's tap is trained to), `compute_distill_loss` behind the plugin's
    `auxiliary_loss`."""

    STUDENT_OUTPUT_KEY = "self_transcendence_guide_loss"

    def __init__(self, model, config: Optional[Dict[str, Any]] = None):
        s = normalized_config(method_config(model.config, METHOD) if config is None else config)
        refuse_unbuilt(model.config, model)
        self.model, self.settings = model, s
        self.stage, self.student_block, self.teacher_block = s["stage"], s["student_block"], s["teacher_block"]
        self.weight, self.cfg_scale = s["weight"], s["cfg_scale"]
        self.timestep_min, self.timestep_max, self.stop_step = s["timestep_min"], s["timestep_max"], s["stop_step"]
        self.teacher_adapter_path = s["teacher_adapter_path"]
        self._global_step = 0
        self.snapshot = None          # stage `self`: the frozen teacher — ONE flat fp32 copy of the adapter arena, never updated
        comp = self.component()
        if comp is None or getattr(comp, "_st", None) is None:
            raise ValueError("Self-Transcendence projector was not attached before distiller initialization.")
        # (validates the blocks against the component, and moves the tap's settings: the projector exists)
        comp.set_self_transcendence(self.stage, self.student_block, self.teacher_block, s["projector_hidden_dim"], self.timestep_min, self.timestep_max, self.cfg_scale)

    def component(self):
        comp = self.model.get_trained_component()
        return None if comp is None else self.model.unwrap_model(comp)

    @property
    def active_weight(self) -> float:
        return 0.0 if self.stop_step and self._global_step >= self.stop_step else self.weight

    def pre_training_step(self, model, step):
        """distiller.py `pre_training_step`: `step` is the training loop's own counter (trainer.py:6876, 6955, 7000: the global step the loop started from plus the
        micro-steps fetched so far, this one included)"""
        self._global_step = int(step)
        comp = self.component()
        comp.self_transcendence_off(self.active_weight == 0.0)
        if self.stage != "self" or self.snapshot is not None:
            return
        self.snapshot = self._snapshot_teacher_adapter(comp) if self.teacher_adapter_path else comp.lora_flat.detach().clone()
        logger.info("Captured a fixed Self-Transcendence teacher snapshot with %d trainable tensors.", len(comp.trainable_parameters()))

    def _snapshot_teacher_adapter(self, comp):
        """`teacher_adapter_path`: the file's adapter values laid over a copy of the arena (the live values are never written)"""
        if not os.path.isfile(self.teacher_adapter_path):
            raise FileNotFoundError(f"Self-Transcendence teacher adapter does not exist: {self.teacher_adapter_path}")
        from safetensors.torch import load_file
        from .training.lora_keys import to_peft_keys
        prefix = (getattr(self.model, "MODEL_SUBFOLDER", None) or "transformer") + "."
        flat = to_peft_keys(load_file(self.teacher_adapter_path))
        flat = {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in flat.items()}
        snap, base = comp.lora_flat.detach().clone(), comp.lora_flat.data_ptr()
        own = {n.replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B."): p for n, p in comp.named_parameters() if ".lora_" in n}
        missing = sorted(k for k in own if k not in flat)
        if missing:
            raise ValueError(f"Self-Transcendence teacher adapter is missing required tensors: {', '.join(missing)}")
        extra = sorted(k for k in flat if k not in own)
        if extra:
            logger.warning("Self-Transcendence teacher adapter contains unused tensors: %s", ", ".join(extra))
        for k, p in own.items():
            lo = (p.data_ptr() - base) // 4
            snap[lo:lo + p.numel()].copy_(flat[k].to(device=snap.device, dtype=torch.float32).reshape(-1))
        return snap

    # ---- what the training forward's tap is trained to ----
    def forward_inputs(self, model, prepared_batch: Dict[str, Any]) -> Dict[str, Any]:
        if self.active_weight == 0.0:
            return {}          # past stop_step: no teacher forwards, no projector (the reference still runs the projector behind a zero weight, for DDP)
        sig = prepared_batch.get("sigmas")
        if sig is None:
            raise ValueError("Self-Transcendence requires sigmas or timesteps for range masking.")
        if self.stage == "vae":
            target = model.get_prediction_target(prepared_batch)
        else:
            target = self.teacher_capture(model, prepared_batch)
        return {"self_transcendence_target": target, "self_transcendence_sigmas": sig}

    def teacher_capture(self, model, prepared_batch: Dict[str, Any]):
        """distiller.py `_cfg_teacher_hidden`, as ONE no-grad forward at batch 2B — the batch's own embeddings on rows [0, B), the empty-prompt embeddings on rows
        [B, 2B) — through the plugin's own model_predict with the adapter operands packed from the snapshot; the forward ends behind `teacher_block`.  Returns the
        [2B, S, D] bf16 capture; the CFG combine happens inside the loss kernel."""
        if self.snapshot is None:
            raise ValueError("Self-Transcendence teacher snapshot was not captured before the training forward.")
        neg = prepared_batch.get("negative_encoder_hidden_states")
        if neg is None:
            neg = prepared_batch.get("negative_prompt_embeds")
        if neg is None:
            raise ValueError("Self-Transcendence self stage requires cached empty-prompt embeddings.")
        enc, pooled = prepared_batch["encoder_hidden_states"], prepared_batch["add_text_embeds"]
        neg_pooled = prepared_batch.get("negative_add_text_embeds")
        neg_pooled = pooled if neg_pooled is None else neg_pooled
        B = enc.shape[0]
        both = lambda a, b: torch.cat([a, b.to(device=a.device, dtype=a.dtype).expand(B, *b.shape[1:])], dim=0)
        two = lambda a: torch.cat([a, a], dim=0)
        batch = {"noisy_latents": two(prepared_batch["noisy_latents"]), "timesteps": two(prepared_batch["timesteps"]), "encoder_hidden_states": both(enc, neg),
                 "add_text_embeds": both(pooled, neg_pooled), "self_transcendence_capture_block": self.teacher_block}
        comp = self.component()
        with torch.no_grad(), comp.teacher_values(self.snapshot):
            out = model.model_predict(batch)
        hidden = out.get("crepa_hidden_states")
        if hidden is None:
            raise ValueError(f"Self-Transcendence teacher forward did not capture layer_{self.teacher_block}.")
        return hidden

    # ---- the loss (trainer.py:6119-6131) ----
    def prepare_model_output(self, model_output: Dict[str, Any]) -> None:
        """the reference keeps the student block's output here; on this path the projector has already run at that block (the engine's tap), so only the presence of
        its output is checked"""
        if self.active_weight != 0.0 and (not isinstance(model_output, dict) or model_output.get(self.STUDENT_OUTPUT_KEY) is None):
            raise ValueError("Self-Transcendence requires a transformer hidden-state buffer.")

    def compute_distill_loss(self, prepared_batch, model_output, original_loss):
        w = self.active_weight
        if w == 0.0:
            return original_loss, {"self_transcendence/loss": 0.0, "self_transcendence/weight": 0.0}
        guide = model_output.get(self.STUDENT_OUTPUT_KEY) if isinstance(model_output, dict) else None
        if guide is None:
            raise ValueError("Self-Transcendence student hidden state was not preserved before auxiliary losses.")
        logs = {"self_transcendence/loss": guide.detach().float().item(), "self_transcendence/weight": w}
        if self.stage == "self":
            logs["self_transcendence/teacher_cfg_scale"] = self.cfg_scale
        return original_loss + guide.to(dtype=original_loss.dtype) * w, logs

    def generator_loss_step(self, prepared_batch, model_output, current_loss):
        return current_loss, {}


def create_distiller(model):
    return SelfTranscendenceDistiller(model)

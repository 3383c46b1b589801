"""SD3 model-family plugin — drop-in for simpletuner/helpers/models/sd3/model.py on MI355X.

Same class attributes and step-path methods as the reference plugin (sd3/model.py:111-125, 540-570): `SD3(config, accelerator)`,
`prepare_batch` (flow matching, common.py:5862-6041), `model_predict -> {"model_prediction": [B,16,H,W]}` with the timesteps passed
to the transformer in 0..1000 (sd3/model.py:542 — no /1000, unlike Flux), `loss_with_logs`, `get_trained_component`,
`add_lora_adapter` (DEFAULT_LORA_TARGET to_k,to_q,to_v,to_out.0).
"""
from __future__ import annotations

import torch

from ..foundation import ModelFoundation, ModelRegistry, ModelTypes, PredictionTypes
from .transformer import SD3Transformer2DModel

BF16 = torch.bfloat16


class SD3(ModelFoundation):
    NAME = "Stable Diffusion 3.x"
    PREDICTION_TYPE = PredictionTypes.FLOW_MATCHING
    MODEL_TYPE = ModelTypes.TRANSFORMER
    MODEL_CLASS = SD3Transformer2DModel
    MODEL_SUBFOLDER = "transformer"
    LORA_DROPOUT_BUILT = True
    DORA_BUILT = True
    LYCORIS_BUILT = True
    SELF_FLOW_BUILT = True
    SELF_TRANSCENDENCE_BUILT = True
    ROLLOUT_BATCH_KEYS = ("encoder_hidden_states", "add_text_embeds")          # what _model_predict_single reads per sample (scheduled sampling's batch-1 forwards)
    LATENT_CHANNEL_COUNT = 16
    COMFYUI_LORA_PRESERVE_COMPONENT_PREFIXES = {"transformer"}      # sd3/model.py:117
    VAE_CONFIG = dict(latent_channels=16, scaling_factor=1.5305, shift_factor=0.0609, use_quant_conv=False)
    DEFAULT_MODEL_FLAVOUR = "medium"
    DEFAULT_LORA_TARGET = ["to_k", "to_q", "to_v", "to_out.0"]
    HUGGINGFACE_PATHS = {"medium": "stabilityai/stable-diffusion-3-medium-diffusers", "large": "stabilityai/stable-diffusion-3.5-large"}

    def load_model(self, state_dict=None, **arch):
        if getattr(self.config, "internal_guidance_enabled", False) and "internal_guidance_block_index" not in arch:
            # Internal Guidance: the head is laid out with the component's arenas (post_model_load_setup repeats the checks in the reference's order)
            import inspect
            n_layers = arch.get("num_layers", inspect.signature(SD3Transformer2DModel.__init__).parameters["num_layers"].default)          # (the constructor's own default)
            arch = dict(arch, internal_guidance_block_index=self.internal_guidance_block_index(int(n_layers)))
        if getattr(self.config, "nextlat_enabled", False) and "nextlat_block_index" not in arch:
            # NextLat: the predictor is laid out with the component's arenas; the constructor applies the reference's index rule (None / 0 / negative = last block)
            arch = dict(arch, nextlat_block_index=getattr(self.config, "nextlat_block_index", None) or -1)
        self.model = SD3Transformer2DModel(device=self.accelerator.device, **arch)
        if getattr(self.config, "crepa_enabled", False) and not getattr(self.config, "irepa_enabled", False) and self._crepa_source() == "self_flow" \
                and "lora" in str(getattr(self.config, "model_type", "lora")):
            # Self-Flow: the projector goes to the tail of the adapter arena, so the component learns its blocks ahead of add_lora_adapter (post_model_load_setup
            # repeats the checks in the reference's order and refuses what this path does not take)
            self.model.set_self_flow(getattr(self.config, "crepa_block_index", None), getattr(self.config, "crepa_teacher_block_index", None))
        if getattr(self.config, "distillation_method", None):
            from ..flow_dpo import method_of
            if method_of(self.config) == "self_transcendence" and str(getattr(self.config, "model_type", "lora")) == "lora" \
                    and str(getattr(self.config, "lora_type", "standard") or "standard").lower() == "standard":
                # Self-Transcendence: the projector goes to the tail of the adapter arena, so the component learns its settings ahead of add_lora_adapter (the
                # distiller repeats the checks in the reference's order and refuses what this path does not take)
                from ..self_transcendence import settings_of
                s = settings_of(self.config)
                self.model.set_self_transcendence(s["stage"], s["student_block"], s["teacher_block"], s["projector_hidden_dim"], s["timestep_min"],
                                                  s["timestep_max"], s["cfg_scale"])
        if state_dict is not None and getattr(self.config, "twinflow_enabled", False):
            from ..twinflow import drop_sign_embedding          # TwinFlow: a zero time-sign table adds nothing under LoRA and is dropped, a trained one is refused
            state_dict = drop_sign_embedding(state_dict)
        if state_dict is not None:
            self.model.load_flat_state(state_dict)
        else:
            self.model.init_synthetic(seed=int(getattr(self.config, "seed", 42) or 42))
        return self.model

    def add_lora_adapter(self):
        if getattr(self.config, "model_type", "lora") != "lora":
            raise RuntimeError("model_type == 'full' trains every transformer parameter: call enable_full_finetune() (or freeze_components()) instead of add_lora_adapter()")
        comp = self.unwrap_model(self.model)
        if str(getattr(self.config, "lora_type", "standard") or "standard").lower() == "lycoris":
            return self._add_lycoris_adapter(comp)
        params = comp.add_lora_adapter(rank=int(self.config.lora_rank), alpha=getattr(self.config, "lora_alpha", None),
                                       targets="default", seed=int(getattr(self.config, "seed", 42) or 42) + 7,
                                       init_b_std=float(getattr(self.config, "lora_init_b_std", 0.0)),
                                       dropout=self.lora_dropout_value(), dropout_seed=int(getattr(self.config, "seed", 42) or 42),
                                       dropout_rank=int(getattr(self.accelerator, "process_index", 0) or 0), dora=self.use_dora_value())
        comp.prepare_for_training()
        return params

    def _add_lycoris_adapter(self, comp):
        """`lora_type=lycoris`: LoKr (or, `algo: tlora`, T-LoRA) adapters on the Attention / FeedForward Linears from the JSON named by `lycoris_config` (ModelFoundation.lycoris_value).  The
        standard-LoRA-only flags keep their treatment (lora_dropout / use_dora ignored); Internal Guidance / NextLat raise the reference's ValueError first."""
        cfg = self.config
        if getattr(cfg, "internal_guidance_enabled", False):
            raise ValueError("Internal Guidance requires standard PEFT LoRA or full-model training so its auxiliary head is optimized and saved.")
        if getattr(cfg, "nextlat_enabled", False):
            raise ValueError("NextLat requires standard PEFT LoRA or full-model training so its predictor is optimized and saved.")
        lc = self.lycoris_value()
        seed = int(getattr(cfg, "seed", 42) or 42) + 7
        if lc.get("algo") == "tlora":          # T-LoRA: low-rank pairs with the timestep rank mask on the same site list
            params = comp.add_tlora_adapter(classes=lc["classes"], linear_dim=lc["linear_dim"], linear_alpha=lc["linear_alpha"], multiplier=lc["multiplier"],
                                            min_rank=lc["min_rank"], alpha=lc["alpha"], num_train_timesteps=lc["num_train_timesteps"], seed=seed)
        else:
            params = comp.add_lokr_adapter(factors=lc["factors"], multiplier=lc["multiplier"], seed=seed, init_norm=lc["init_norm"], linear_dim=lc["linear_dim"])
        comp.lokr_validation_strength = lc["validation_strength"]
        self.lycoris = lc
        comp.prepare_for_training()
        return params

    def enable_full_finetune(self):
        """model_type == "full" (BASELINE.json configs[3]): every transformer parameter trains (bf16 params + bf16 grads in two arenas)"""
        return self.unwrap_model(self.model).enable_full_finetune()

    def _model_predict_single(self, prepared_batch: dict):
        """sd3/model.py:540-570"""
        self._require_per_sample_timesteps(prepared_batch, tokenwise_ok=True)      # [B] or tokenwise [B, S_img], handed through unchanged (sd3/model.py:542)
        dev = self.accelerator.device
        extra = {}
        if getattr(self, "self_flow", None) is not None and torch.is_grad_enabled() and prepared_batch.get("crepa_teacher_noisy_latents") is not None:
            extra["crepa_teacher_features"] = self._self_flow_teacher_features(prepared_batch)          # the teacher forward first, then the training forward with the tap
        st = getattr(self, "self_transcendence", None)
        if st is not None and prepared_batch.get("self_transcendence_capture_block") is not None:
            extra["crepa_capture_block_index"] = prepared_batch["self_transcendence_capture_block"]     # Self-Transcendence's teacher forward (no grad, ends behind the block)
        elif st is not None and torch.is_grad_enabled():
            extra.update(st.forward_inputs(self, prepared_batch))                                      # (stage `self`: the teacher forward first, as Self-Flow does)
        res = self.model(
            hidden_states=prepared_batch["noisy_latents"].to(device=dev, dtype=BF16),
            timestep=prepared_batch["timesteps"].to(device=dev, dtype=torch.float32),
            encoder_hidden_states=prepared_batch["encoder_hidden_states"].to(device=dev, dtype=BF16),
            pooled_projections=prepared_batch["add_text_embeds"].to(device=dev, dtype=BF16),
            return_dict=True,
            **({"return_internal_guidance": True} if prepared_batch.get("return_internal_guidance") else {}),          # sampling with validation_internal_guidance_scale != 1
            **extra,
        )
        # further outputs travel by name; (a component that hands back a plain tuple has only its sample)
        out = {"model_prediction": res[0] if isinstance(res, tuple) else res.sample, "crepa_hidden_states": None, "hidden_states_buffer": None}
        for k in ("layersync_similarity", "internal_guidance_prediction", "nextlat_state_loss", "crepa_similarity", "self_transcendence_guide_loss") \
                + (("crepa_hidden_states",) if "crepa_capture_block_index" in extra else ()):          # LayerSync / Internal Guidance / NextLat / Self-Flow: the training forward's further outputs
            if getattr(res, k, None) is not None:
                out[k] = getattr(res, k)
        return out


    def _self_flow_teacher_features(self, prepared_batch: dict):
        """common.py `_run_crepa_teacher_forward`: the EMA teacher's forward on the cleaner homogeneous view — no grad, the adapter operands packed from the EMA's
        flat shadow (ArenaModule.teacher_values: the masters are never written, unlike the reference's store / copy_to / restore), the image rows of block
        `crepa_teacher_block_index` copied out; the forward ends behind that block."""
        ema = getattr(self, "ema_model", None)
        if ema is None or not getattr(self.config, "use_ema", False):
            raise ValueError("EMA teacher weights are required but unavailable; enable use_ema or allow fallback.")          # common.py:5294-5295
        shadow = getattr(ema, "shadow_flat", None)
        if shadow is None:
            raise NotImplementedError("crepa_enabled (self_flow): the EMA shadow is not one flat buffer over the adapter arena; not built on the st355 path")
        dev = self.accelerator.device
        comp = self.unwrap_model(self.model)
        with torch.no_grad(), comp.teacher_values(shadow):
            res = comp(hidden_states=prepared_batch["crepa_teacher_noisy_latents"].to(device=dev, dtype=BF16),
                       timestep=prepared_batch["crepa_teacher_timesteps"].to(device=dev, dtype=torch.float32),
                       encoder_hidden_states=prepared_batch["encoder_hidden_states"].to(device=dev, dtype=BF16),
                       pooled_projections=prepared_batch["add_text_embeds"].to(device=dev, dtype=BF16), return_dict=True,
                       crepa_capture_block_index=self.self_flow.teacher_block_index)
        return res.crepa_hidden_states


ModelRegistry.register("sd3", SD3)

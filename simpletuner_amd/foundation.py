"""Model-family plugin surface, mirroring the reference's duck-typed contract:

    ModelRegistry.register / get / model_families        simpletuner/helpers/models/registry.py:54-98
    PredictionTypes / ModelTypes                         simpletuner/helpers/models/common.py:368-392
    ModelFoundation.prepare_batch                        simpletuner/helpers/models/common.py:5862-6041
                   .sample_flow_sigmas                   simpletuner/helpers/models/common.py:4994-5090
                   ._prepare_flow_noisy_latents          simpletuner/helpers/models/common.py:4975-4992
                   .get_prediction_target / flow target  simpletuner/helpers/models/common.py:4610-4658
                   .loss / loss_with_logs / aux loss     simpletuner/helpers/models/common.py:6217-6430, xm_mixin.py:476-485
    apply_flow_schedule_shift                            simpletuner/helpers/training/custom_schedule.py:443-478

Same method names, argument meaning, batch-dict keys and error behaviour; the bulk arithmetic (noising, target, MSE and
its gradient) runs in libst355 (ops.flow_noise_mix / ops.mse_loss).  Per-sample scalars ([B]-sized sigma math) stay in torch.
Only the options used by the BASELINE configs are implemented; anything else raises NotImplementedError (never a silent
different path).
"""
from __future__ import annotations

import math
from enum import Enum
from types import SimpleNamespace
from typing import Any, Dict, Optional, Type

import torch

from . import ops
from .xm import ExplorativeModelingConfig, ExplorativeModelingMixin

BF16 = torch.bfloat16


class PredictionTypes(Enum):
    EPSILON = "epsilon"
    SAMPLE = "sample"
    V_PREDICTION = "v_prediction"
    FLOW_MATCHING = "flow_matching"

    @staticmethod
    def from_str(label):
        if label in ("eps", "epsilon"):
            return PredictionTypes.EPSILON
        if label in ("vpred", "v_prediction", "v-prediction"):
            return PredictionTypes.V_PREDICTION
        if label in ("sample", "x_prediction", "x-prediction"):
            return PredictionTypes.SAMPLE
        if label in ("flow", "flow_matching", "flow-matching"):
            return PredictionTypes.FLOW_MATCHING
        raise NotImplementedError


class ModelTypes(Enum):
    UNET = "unet"
    TRANSFORMER = "transformer"
    VAE = "vae"
    TEXT_ENCODER = "text_encoder"


class ModelRegistry:
    """registry.py:54-98 (the metadata-JSON lazy path is the reference's own; a drop-in only needs register/get)."""
    _registry: Dict[str, Type[Any]] = {}

    @classmethod
    def register(cls, family: str, model_class: Type[Any]) -> None:
        cls._registry[family.lower()] = model_class

    @classmethod
    def get(cls, family: str):
        return cls._registry.get(family.lower())

    @classmethod
    def model_families(cls) -> Dict[str, Type[Any]]:
        return dict(cls._registry)


def calculate_shift(image_seq_len, base_seq_len: int = 256, max_seq_len: int = 4096, base_shift: float = 0.5, max_shift: float = 1.15):
    """diffusers.pipelines.flux.pipeline_flux.calculate_shift (imported at flux/__init__.py:5)"""
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    b = base_shift - m * base_seq_len
    return image_seq_len * m + b


def apply_flow_schedule_shift(args, noise_scheduler, sigmas, noise):
    """custom_schedule.py:443-478"""
    shift = None
    if getattr(args, "flow_schedule_shift", None) is not None and args.flow_schedule_shift > 0:
        shift = args.flow_schedule_shift
    elif getattr(args, "flow_schedule_auto_shift", False):
        if noise.ndim == 5:
            num_frames, height, width = noise.shape[-3:]
        else:
            num_frames = 1
            height, width = noise.shape[-2:]
        cfg = getattr(noise_scheduler, "config", None)
        patch_size = getattr(cfg, "patch_size", 2) or 2
        if patch_size <= 0:
            patch_size = 2
        seq_len = num_frames * (height // patch_size) * (width // patch_size)
        mu = calculate_shift(seq_len, getattr(cfg, "base_image_seq_len", 256), getattr(cfg, "max_image_seq_len", 4096),
                             getattr(cfg, "base_shift", 0.5), getattr(cfg, "max_shift", 1.15))
        shift = math.exp(mu)
    if shift is not None:
        sigmas = (sigmas * shift) / (1 + (shift - 1) * sigmas)
    return sigmas


def enforce_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """`rescale_betas_zero_snr` (custom_schedule.py:157-175; "Common Diffusion Noise Schedules and Sample Steps are Flawed", alg. 1): shift
    sqrt(alphas_cumprod) so the last step carries no signal, rescale so the first step keeps its value, convert back to betas"""
    root = (1 - betas).cumprod(0).sqrt()
    first, last = root[0].clone(), root[-1].clone()
    root = (root - last) * (first / (first - last))
    bar = root ** 2
    return 1 - torch.cat([bar[0:1], bar[1:] / bar[:-1]])


class DDPMSchedule:
    """the training-side arithmetic of diffusers' DDPMScheduler as the reference configures it for SD1.5 / SDXL (common.py:4529-4550; the
    checkpoint's scheduler_config.json: beta_schedule "scaled_linear", beta_start 0.00085, beta_end 0.012, 1000 steps)."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012, beta_schedule: str = "scaled_linear",
                 prediction_type: str = "epsilon", device=None, rescale_betas_zero_snr: bool = False):
        from types import SimpleNamespace
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(beta_schedule)
        if rescale_betas_zero_snr:
            betas = enforce_zero_terminal_snr(betas)
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, prediction_type=prediction_type, beta_schedule=beta_schedule,
                                      rescale_betas_zero_snr=bool(rescale_betas_zero_snr))
        self._acp_dev = {}
        self._sa = self.alphas_cumprod.sqrt().to(device)
        self._sb = (1.0 - self.alphas_cumprod).sqrt().to(device)

    def mix_coefficients(self, timesteps):
        return self._sa[timesteps].contiguous(), self._sb[timesteps].contiguous()

    def snr(self, timesteps):
        """compute_snr (min_snr_gamma.py:4-41): (alpha/sigma)^2 = acp / (1 - acp)"""
        a = self.acp_on(timesteps.device)[timesteps.long()].float()
        return a / (1.0 - a)

    def acp_on(self, device):
        """alphas_cumprod resident on `device` (copied once): the SNR / huber paths run inside hipGraph capture, where an H2D copy is illegal"""
        key = str(torch.device(device))
        hit = self._acp_dev.get(key)
        if hit is None:
            hit = self._acp_dev[key] = self.alphas_cumprod.to(device)
        return hit

    def min_snr_weights(self, timesteps, gamma: float, v_prediction: bool):
        """common.py:6363-6397: min(snr, gamma) / snr  (epsilon)  or  / (snr + 1)  (v-prediction), one weight per sample"""
        snr = self.snr(timesteps)
        return torch.minimum(snr, torch.full_like(snr, float(gamma))) / (snr + 1.0 if v_prediction else snr)

    @staticmethod
    def timestep_weights(config, T: int) -> torch.Tensor:
        """generate_timestep_weights (custom_schedule.py:61-100): uniform, or a multiplier on the later / earlier / [begin, end) timesteps"""
        w = torch.ones(T)
        strat = getattr(config, "timestep_bias_strategy", "none") if config is not None else "none"
        n = int(float(getattr(config, "timestep_bias_portion", 0.25)) * T) if config is not None else 0
        if strat == "later":
            idx = slice(-n, None)
        elif strat == "earlier":
            idx = slice(0, n)
        elif strat == "range":
            lo, hi = int(config.timestep_bias_begin), int(config.timestep_bias_end)
            if lo < 0 or hi > T:
                raise ValueError("timestep_bias_begin / timestep_bias_end must lie inside [0, num_train_timesteps]")
            idx = slice(lo, hi)
        else:
            return w
        mult = float(getattr(config, "timestep_bias_multiplier", 1.0))
        if mult <= 0:
            raise ValueError("timestep_bias_multiplier must be positive (use timestep_bias_strategy=none to disable the bias)")
        w[idx] *= mult
        return w / w.sum()

    def sample_timesteps(self, bsz: int, segmented: bool = True, weights: Optional[torch.Tensor] = None, refiner_training: bool = False,
                         refiner_invert_schedule: bool = False, refiner_strength: float = 0.2):
        """weights: generate_timestep_weights (uniform by default); bsz > 1: one draw from each of bsz equal segments, high to low
        (segmented_timestep_selection, custom_schedule.py:18-58, same draw order as the reference); SDXL-refiner training restricts the range to
        the low-noise tail [0, strength*T) — or, inverted, to [strength*T, T) (:21-31).  Drawn on the host: no device sync."""
        T = self.config.num_train_timesteps
        weights = torch.ones(T) if weights is None else weights.clone()
        if bsz == 1 or not segmented:
            return torch.multinomial(weights, bsz, replacement=True).long()
        hi, lo = T - 1, 0
        if refiner_training:
            hi, lo = (T - 1, int(refiner_strength * T)) if refiner_invert_schedule else (int(T * refiner_strength) - 1, 0)
        seg = max((hi - lo + 1) // bsz, 1)
        out = []
        for i in range(bsz):
            start = hi - i * seg
            end = max(start - seg, lo) if i != bsz - 1 else lo
            w = weights[end:start + 1]
            w /= w.sum()                                   # in place on the slice, as the reference does (:50)
            out.append(end + int(torch.multinomial(w, 1).item()))
        return torch.tensor(out, dtype=torch.long)


DATA_BACKEND_CONFIGS = {}


def get_data_backend_config(backend_id) -> dict:
    """stand-in for StateTracker.get_data_backend_config (state_tracker.py): unknown / missing ids have an empty config"""
    src = DATA_BACKEND_CONFIGS
    cfg = src(backend_id) if callable(src) else src.get(backend_id)
    return cfg or {}


def _process_rank(accelerator=None) -> int:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(getattr(accelerator, "process_index", 0) or 0)


class ModelFoundation(ExplorativeModelingMixin):
    """the subset of common.py's ModelFoundation that the step loop touches (trainer.py:6951-7568)."""
    NAME = "foundation"
    PREDICTION_TYPE = PredictionTypes.FLOW_MATCHING
    MODEL_TYPE = ModelTypes.TRANSFORMER
    MODEL_CLASS = None
    MODEL_SUBFOLDER = "transformer"
    LATENT_CHANNEL_COUNT = 16
    DEFAULT_LORA_TARGET = ["to_k", "to_q", "to_v", "to_out.0"]
    DDP_FIND_UNUSED_PARAMETERS = False
    PIPELINE_CLASSES: Dict[str, Any] = {}        # validation pipelines are outside this tier (sampling.py holds the denoising loop)
    TEXT_ENCODER_CONFIGURATION: Dict[str, Any] = {}   # text encoders run offline into the embed cache (training/cache_io.py reads it)
    AUTOENCODER_CLASS = None                     # set per family below (lazy: the class needs the device library)
    VAE_CONFIG: Dict[str, Any] = {}              # constructor arguments of the family's AutoencoderKL (upstream `vae/config.json` values)

    def __init__(self, config, accelerator):
        self.config = config
        self.accelerator = accelerator
        self.model = None
        # components the reference Trainer reads / clears on the plugin (trainer.py:2592-2593, 2676-2677, 2914-2917, 3050, 4375): text encoders run
        # OFFLINE into the embed cache on this path (training/cache_io.py), so the lists stay empty and the unload hooks have nothing to move
        self.vae = None
        self.text_encoders: list = []
        self.tokenizers: list = []
        self.controlnet = None
        self.pipelines: dict = {}
        self.pipeline = None
        self.ema_model = None
        self.noise_schedule = None
        self._noise_step = 0            # noising passes issued (diagnostic)
        self._noise_offset = 0          # CUMULATIVE Philox counter position: every pass consumes its own, non-overlapping counter range whatever its shape
        self.xm_config = ExplorativeModelingConfig.from_config(config)     # common.py:578
        if getattr(config, "twinflow_enabled", False):                     # common.py:601 `_validate_twinflow_config`, then what this path does not take
            self.twinflow_value()

    # ---- latent encode seam (common.py:2653-2772, foundation_mixins.py:66-79) ----
    @classmethod
    def autoencoder_class(cls):
        if cls.AUTOENCODER_CLASS is None:
            from .vae.autoencoder_kl import AutoencoderKL
            return AutoencoderKL
        return cls.AUTOENCODER_CLASS

    def load_vae(self, state_dict=None, move_to_device: bool = True):
        """common.py:2663: build the family's AutoencoderKL (encoder half; diffusers state-dict keys).  Without a state dict the weights are
        synthetic (benchmarks, tests) — there is no hub access here."""
        vae = self.autoencoder_class()(device=self.accelerator.device, **self.VAE_CONFIG)
        vae.load_state_dict(state_dict if state_dict is not None else vae.synthetic_state_dict(int(getattr(self.config, "seed", 42) or 42), decoder=True))
        self.vae = vae
        return vae

    def get_vae(self):
        if getattr(self, "vae", None) is None:
            self.load_vae()
        return self.vae

    @torch.no_grad()
    def encode_with_vae(self, vae, samples):
        return vae.encode(samples)

    def scale_vae_latents_for_cache(self, latents, vae):
        """foundation_mixins.py:66-79: (z - shift) * scale when the VAE has a shift factor, z * scale otherwise"""
        if vae is None or not hasattr(vae, "config") or latents is None:
            return latents
        shift = getattr(vae.config, "shift_factor", None)
        scale = getattr(self, "AUTOENCODER_SCALING_FACTOR", getattr(vae.config, "scaling_factor", 1.0))
        if shift is not None:
            return (latents - shift) * scale
        if isinstance(latents, torch.Tensor) and hasattr(vae.config, "scaling_factor"):
            return latents * scale
        return latents

    # ---- prediction entry points; XM (off by default) expands the batch with K noise candidates first (flux/model.py:630-636, 940-946) ----
    def model_predict(self, prepared_batch: dict):
        if prepared_batch.get("scheduled_sampling_plan") is not None and not prepared_batch.get("_scheduled_sampling_rolled"):
            # a step loop that skips the rollout would train on the un-rolled batch with the plan's loss terms: refused, never a silently different computation
            raise RuntimeError("scheduled_sampling_max_step_offset: the batch carries a scheduled_sampling_plan but the rollout has not run — call "
                               "plugin.apply_scheduled_sampling_rollout(prepared_batch) between prepare_batch and model_predict (Trainer.train_step does)")
        return self._xm_wrapped(self._model_predict_single, prepared_batch)

    def controlnet_predict(self, prepared_batch: dict):
        return self._xm_wrapped(self._controlnet_predict_single, prepared_batch)

    def _xm_wrapped(self, predict, prepared_batch: dict):
        if self._xm_noise_candidates_enabled(prepared_batch):
            self._prepare_xm_noise_candidates(prepared_batch)
            out = predict(prepared_batch)
            out["xm_candidate_count"] = self.xm_config.candidate_count
            return out
        return predict(prepared_batch)

    def _model_predict_single(self, prepared_batch: dict):
        raise NotImplementedError

    def _controlnet_predict_single(self, prepared_batch: dict):
        raise NotImplementedError(f"{self.NAME} has no ControlNet path")

    # ---- component plumbing (common.py:3691, 3781) ----
    def get_trained_component(self, base_model: bool = False, unwrap_model: bool = True):
        return self.unwrap_model(self.model) if unwrap_model else self.model

    def set_prepared_model(self, model, base_model: bool = False):
        """common.py:3691 / trainer.py:4577: the trainer hands back what `accelerator.prepare` returned.  A torch DistributedDataParallel around an st355
        component gets the st355 communication hook (the component's own in-backward exchange, training.ddp_seam) unless it already has one; an
        `St355DistributedDataParallel` wrapper, or the bare component, is stored as is."""
        self.model = model
        if type(model).__name__ == "DistributedDataParallel" and hasattr(model, "register_comm_hook") and getattr(model, "_st355_seam", None) is None:
            from .training.ddp_seam import install_ddp_comm_hook
            install_ddp_comm_hook(model)

    @staticmethod
    def unwrap_model(model):
        """common.py:3700 (accelerator.unwrap_model): strip DDP-style wrappers (`.module`), however nested"""
        seen = 0
        while hasattr(model, "module") and isinstance(getattr(model, "module"), torch.nn.Module) and seen < 4:
            model, seen = model.module, seen + 1
        return model

    def _require_per_sample_timesteps(self, prepared_batch: dict, tokenwise_ok: bool = False, conditioning_ok: bool = False):
        """The reference's DiT plugins also accept TOKENWISE timesteps [B, S] (CREPA self-flow; tests/test_flux_model.py:213-241,
        tests/test_sd3_model.py:179-204, tests/test_pixart_model.py:91-115) and clean conditioning tokens appended at t=0 (Flux Kontext,
        tests/test_flux_model.py:243-272).  Both need per-token modulation rows.  Tokenwise timesteps are built for SD3, Flux and the PixArt trunk (`tokenwise_ok`: their engines run the AdaLN /
        gated-residual kernels with one modulation row per token); the PixArt ControlNet wrapper, and the reference-image tokens everywhere, refuse loudly instead of training on the wrong conditioning."""
        t = prepared_batch["timesteps"]
        if getattr(t, "ndim", 1) == 2 and tokenwise_ok:
            pass
        elif getattr(t, "ndim", 1) != 1:
            raise NotImplementedError(f"tokenwise timesteps {tuple(t.shape)} are not implemented on the st355 path (per-sample [B] only)")
        if prepared_batch.get("conditioning_packed_latents") is not None and not conditioning_ok:
            raise NotImplementedError("conditioning_packed_latents (reference-image tokens) are not implemented on the st355 path")

    # ---- lifecycle hooks the reference Trainer calls on `self.model` outside the step loop (trainer.py:329-330, 2618-2621, 2944, 3243-3292, 3353,
    #      4318, 4376, 4450, 4651, 5539, 6042, 7631-7642, 7749-7754).  tests/test_integration_contract_cpu.py AST-scans that file and fails on any
    #      `self.model.<name>` this class lacks.  Hooks whose feature lives outside the hot path are explicit no-ops or loud refusals. ----
    GLIGEN_LYCORIS_TARGET: list = []

    def check_user_config(self):
        """common.py:2137 (family overrides adjust config in place).  The st355 path checks what it cannot honour: bf16 compute only."""
        wd = getattr(self.config, "weight_dtype", BF16)
        if wd not in (BF16, "bf16", None):
            raise ValueError(f"{self.NAME} (st355): weight_dtype {wd} — the MI355X path computes in bf16 (mixed_precision=bf16)")

    def _mixflow_enabled(self) -> bool:
        return getattr(self.config, "mixflow_enabled", False) is True

    def validate_mixflow_config(self) -> None:
        """common.py:4923-4950: mixflow needs a flow-matching family and excludes the alternative sigma samplers"""
        if not self._mixflow_enabled():
            return
        if self.PREDICTION_TYPE is not PredictionTypes.FLOW_MATCHING:
            raise ValueError("mixflow_enabled requires a flow-matching model family.")
        self._mixflow_gamma()
        conflicts = {"flux_fast_schedule": bool(getattr(self.config, "flux_fast_schedule", False)),
                     "flow_use_uniform_schedule": bool(getattr(self.config, "flow_use_uniform_schedule", False)),
                     "flow_use_beta_schedule": bool(getattr(self.config, "flow_use_beta_schedule", False)),
                     "flow_custom_timesteps": getattr(self.config, "flow_custom_timesteps", None) not in (None, "", "None")}
        active = [k for k, v in conflicts.items() if v]
        if active:
            raise ValueError(f"mixflow_enabled cannot be combined with {', '.join(active)}.")

    def load_text_encoder(self, move_to_device: bool = True):
        """common.py:2949.  Text encoders are not part of the per-step path (embeddings come from the cache, caching/text_embeds.py): nothing is loaded"""
        self.text_encoders, self.tokenizers = [], []

    # ---- text-embed cache record -> validation-pipeline kwargs (the three members besides model_predict that the reference's ABC declares
    # abstract, common.py:1744-1766; a class registered into ModelRegistry must define them to be instantiable) -------------------------------------
    # (cache-record key, pipeline kwarg, rank WITH the batch dimension); per family as written in <family>/model.py `convert_text_embed_for_pipeline`
    TEXT_EMBED_FIELDS = (("prompt_embeds", "prompt_embeds", 3), ("pooled_prompt_embeds", "pooled_prompt_embeds", 2))

    def _convert_text_embed(self, text_embedding: dict, negative: bool) -> dict:
        out = {}
        for src, dst, rank in self.TEXT_EMBED_FIELDS:
            t = text_embedding[src]
            if t.dim() == rank - 1:                  # "Add batch dimension if missing" (e.g. sd3/model.py:392-396)
                t = t.unsqueeze(0)
            out[("negative_" + dst) if negative else dst] = t
        return out

    def convert_text_embed_for_pipeline(self, text_embedding: dict) -> dict:
        """e.g. sd3/model.py:387-401, sdxl/model.py:135-149, sd1x/model.py:112-122, pixart/model.py:194-208 (Flux overrides: prompt_mask)"""
        return self._convert_text_embed(text_embedding, negative=False)

    def convert_negative_text_embed_for_pipeline(self, text_embedding: dict) -> dict:
        """e.g. sd3/model.py:403-417: the same record under the `negative_*` kwarg names (the CFG half of the validation pair)"""
        return self._convert_text_embed(text_embedding, negative=True)

    def _encode_prompts(self, prompts: list, is_negative_prompt: bool = False):
        """common.py:1744-1750.  Running the CLIP / T5 text encoders is outside the per-step path (text-embed caching is offline
        preprocessing): the st355 plugins consume cached embeddings.  Under `integration.register()` with an importable SimpleTuner the registered
        class also derives from the reference's own family class, whose `_encode_prompts` is then the one that runs."""
        for base in type(self).__mro__:
            if base.__module__.startswith("simpletuner.") and "_encode_prompts" in base.__dict__ and not getattr(base.__dict__["_encode_prompts"], "__isabstractmethod__", False):
                return base.__dict__["_encode_prompts"](self, prompts, is_negative_prompt)
        raise NotImplementedError("text encoders are not part of the st355 per-step path: feed cached text embeddings (collate_fn / DirectCacheFeeder)")

    def get_text_encoder(self, index: int):
        """common.py:3130"""
        if self.text_encoders is not None:
            return self.text_encoders[index] if 0 <= index < len(self.text_encoders) else None
        return None

    def unload_text_encoder(self):
        """common.py:3134"""
        self.text_encoders, self.tokenizers = [], []

    def unload_vae(self):
        """common.py:2794"""
        self.vae = None

    def unload(self):
        """common.py:3214: drop every component (device memory returns to the allocator when the last reference dies)"""
        self.unload_vae()
        self.unload_text_encoder()
        self.model = None
        self.controlnet = None
        self.pipelines, self.pipeline = {}, None

    def freeze_components(self):
        """common.py:3700-3709.  Frozen-ness is structural here: base weights are `requires_grad=False` parameters by construction (LoRA) and the
        full fine-tune exposes exactly its arena views; the VAE / ControlNet trunk never carry gradients"""
        if "lora" in str(getattr(self.config, "model_type", "lora")) and self.model is not None:
            for n, p_ in self.unwrap_model(self.model).named_parameters():
                if ".lora_" not in n and ".lokr_" not in n and not (n.startswith(("internal_guidance_head.", "nextlat_predictor.", "crepa_projector.", "self_transcendence_projector.")) and p_.dtype == torch.float32):      # (the heads' fp32 masters train with the adapters)
                    p_.requires_grad_(False)
        elif str(getattr(self.config, "model_type", "lora")) == "full" and self.model is not None:
            # the reference leaves a full-rank model as diffusers loaded it — every parameter trainable — and `Trainer._get_trainable_parameters` collects
            # `requires_grad` parameters (trainer.py:3668-3673).  Here trainability is a mode of the component (gradient arena + full backward): entered at the same
            # point of the lifecycle, so an unmodified Trainer needs no extra call
            comp = self.unwrap_model(self.model)
            if hasattr(comp, "enable_full_finetune") and not getattr(comp, "full", False):
                comp.enable_full_finetune()

    def pre_ema_creation(self):
        """common.py:2125: the reference fuses qkv here so EMA shapes line up; fused storage is the only layout on this path"""
        self.fuse_qkv_projections()

    def post_ema_creation(self):
        """common.py:2131"""
        return None

    def post_model_load_setup(self):
        """common.py:3638 / 6704 (ImageModelFoundation).  The reference attaches its representation-alignment regularisers here (LayerSync, internal guidance,
        NextLat, CREPA / U-REPA: hooks into a diffusers module's blocks).  The three that need nothing outside the model are built for the components that expose
        their setter: LayerSync (`set_layersync`: Flux, SD3), Internal Guidance (`set_internal_guidance`: SD3) and NextLat (`set_nextlat`: SD3).  The REPA family
        needs an external vision encoder and is refused — defined here so that a reference flow calling it never reaches the reference's regulariser initialisers
        through the MRO."""
        self.self_flow = None
        for flag in ("crepa_enabled", "irepa_enabled", "urepa_enabled"):
            if getattr(self.config, flag, False):
                if flag == "crepa_enabled" and self._crepa_source() == "self_flow":
                    continue          # Self-Flow needs nothing outside the model: the EMA copy of the same model is the teacher (`set_self_flow`: SD3)
                raise NotImplementedError(f"{flag}: the REPA regularisers align with an external vision encoder hooked into diffusers modules and are not built on the st355 path")
        if getattr(self.config, "crepa_enabled", False):
            self._self_flow_init()
        self.layersync = None
        if getattr(self.config, "layersync_enabled", False):
            self._layersync_init()
        self.internal_guidance = None
        if getattr(self.config, "internal_guidance_enabled", False):
            self._internal_guidance_init()
        self.nextlat = None
        if getattr(self.config, "nextlat_enabled", False):
            self._nextlat_init()
        return None

    LORA_DROPOUT_BUILT = False          # families whose engine draws the LoRA-dropout masks (SD3)
    DORA_BUILT = False                  # families whose engine folds the DoRA row scale (SD3)

    def use_dora_value(self) -> bool:
        """`use_dora` (the reference builds every standard LoRA with LoraConfig(use_dora=...): common.py:1094-1104) as the family's add_lora_adapter takes it:
        False when absent; a full fine-tune and lora_type=lycoris ignore the flag, as the reference does; a standard LoRA of a family without the fold refuses it by
        name, and so do the combinations that are not built — never a silently different computation."""
        cfg = self.config
        v = getattr(cfg, "use_dora", False)
        on = v.strip().lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v)
        if not on or "lora" not in str(getattr(cfg, "model_type", "lora")) or str(getattr(cfg, "lora_type", "standard") or "standard").lower() != "standard":
            return False
        if not self.DORA_BUILT:
            raise NotImplementedError(f"use_dora: DoRA is not built for {self.NAME} on the st355 path (built: SD3); set --use_dora=false")
        p = float(getattr(cfg, "lora_dropout", 0.0) or 0.0)
        if p > 0.0:
            raise NotImplementedError(f"use_dora with lora_dropout={p}: peft then feeds the dropped x to the base term of the DoRA correction, a different "
                                      "computation that is not built on the st355 path; set --lora_dropout=0 or --use_dora=false")
        opt = str(getattr(cfg, "optimizer", "") or "")
        if opt in ("muon", "soap"):
            raise NotImplementedError(f"use_dora with optimizer '{opt}': the trainable arena then holds the magnitudes' 1-D tensors, which the matrix optimizers do "
                                      "not take (built: st355-adamw = torch-adamw, adamw_bf16, optimi-lion, torch-adafactor)")
        from .training.lora_keys import PEFTLoRAFormat, normalize_lora_format
        if normalize_lora_format(getattr(cfg, "lora_format", None)) == PEFTLoRAFormat.COMFYUI:
            raise NotImplementedError("use_dora with lora_format=comfyui: the ComfyUI export of a DoRA adapter is not built on the st355 path; set "
                                      "--lora_format=diffusers")
        return True

    LYCORIS_BUILT = False               # families whose engine folds the LoKr delta (SD3)
    LYCORIS_CLASSES = ("Attention", "FeedForward")          # the `target_module` entries with adapter sites
    _lycoris_alpha_logged = False

    def lycoris_value(self):
        """`lora_type=lycoris` (the reference hands `lycoris_config` to LyCORIS' create_lycoris: trainer.py:3390-3440) as the family's add_lora_adapter takes it: None
        for a standard LoRA or a full fine-tune; a family without the fold refuses the flag by name (it would otherwise train a standard LoRA under it); for SD3 the
        parsed JSON — {factors: {module class: factor}, multiplier, linear_dim, linear_alpha, init_norm, validation_strength} — with every option that is not built
        refused by its key and the value to set, never a silently different adapter."""
        cfg = self.config
        if "lora" not in str(getattr(cfg, "model_type", "lora")) or str(getattr(cfg, "lora_type", "standard") or "standard").lower() != "lycoris":
            return None
        if not self.LYCORIS_BUILT:
            raise NotImplementedError(f"lora_type=lycoris: LyCORIS adapters are not built for {self.NAME} on the st355 path (built: SD3); set --lora_type=standard")
        src = getattr(cfg, "lycoris_config", None)
        if isinstance(src, dict):
            lc = dict(src)
        elif src:
            import json
            with open(src, "r") as f:
                lc = json.load(f)
        else:
            raise ValueError("lora_type=lycoris needs lycoris_config: the path of the LyCORIS JSON (algo, multiplier, linear_dim, linear_alpha, factor, apply_preset)")
        refuse = lambda key, val, to: NotImplementedError(f"lycoris_config {key}={val}: not built on the st355 path (built: algo=lokr with both factors full, merged-weight "
                                                          f"forward); set {to}")
        algo = str(lc.get("algo", "lokr")).lower()
        if algo not in ("lokr", "tlora"):
            raise refuse("algo", algo, '"algo": "lokr"')
        for k in ("decompose_both", "use_tucker", "use_scalar", "weight_decompose", "rs_lora", "train_norm", "bypass_mode"):
            if lc.get(k):
                raise refuse(k, "true", f'"{k}": false')
        for k in ("dropout", "rank_dropout", "module_dropout"):
            if float(lc.get(k, 0.0) or 0.0) > 0.0:
                raise refuse(k, lc[k], f'"{k}": 0')
        from .training.lora_keys import PEFTLoRAFormat, normalize_lora_format
        if normalize_lora_format(getattr(cfg, "lora_format", None)) == PEFTLoRAFormat.COMFYUI:
            raise NotImplementedError("lora_type=lycoris with lora_format=comfyui: the ComfyUI export of a LoKr adapter is not built on the st355 path; set "
                                      "--lora_format=diffusers")
        if getattr(cfg, "init_lora", None):
            raise NotImplementedError(f"lora_type=lycoris with init_lora={cfg.init_lora}: starting a LoKr adapter from a file through init_lora is not built on the st355 "
                                      "path; unset --init_lora (resume_from_checkpoint restores the adapter)")
        preset = lc.get("apply_preset") or {}
        classes = list(preset.get("target_module", self.LYCORIS_CLASSES))
        for c in classes:
            if c not in self.LYCORIS_CLASSES:
                raise NotImplementedError(f"lycoris_config apply_preset.target_module entry {c!r}: not built for {self.NAME} on the st355 path; set target_module to a "
                                          f"subset of {list(self.LYCORIS_CLASSES)}")
        amap = preset.get("module_algo_map") or {}
        factors = {}
        for c in classes:
            sub = amap.get(c) or {}
            sub_algo = str(sub.get("algo", algo)).lower()
            if sub_algo not in ("lokr", "tlora"):
                raise refuse(f"apply_preset.module_algo_map.{c}.algo", sub["algo"], '"algo": "lokr"')
            if sub_algo != algo:
                raise NotImplementedError(f"lycoris_config apply_preset.module_algo_map.{c}.algo={sub_algo} beside algo={algo}: one component that mixes lokr and tlora "
                                          "adapters is not built on the st355 path; set the same algo for every module class")
            factors[c] = int(sub.get("factor", lc.get("factor", -1)))
        if algo == "tlora":
            return self._tlora_value(lc, classes, amap)
        linear_dim, linear_alpha = int(lc.get("linear_dim", 4)), lc.get("linear_alpha", None)
        if linear_alpha is not None and float(linear_alpha) != float(linear_dim) and not ModelFoundation._lycoris_alpha_logged:
            ModelFoundation._lycoris_alpha_logged = True
            import logging
            logging.getLogger(__name__).info("lycoris lokr: both factors are full matrices, so LyCORIS sets alpha = linear_dim and the scale is the multiplier; "
                                             "linear_alpha=%s has no effect", linear_alpha)
        init_norm = getattr(cfg, "init_lokr_norm", None)
        return dict(factors=factors, multiplier=float(lc.get("multiplier", 1.0)), linear_dim=linear_dim, linear_alpha=linear_alpha,
                    init_norm=None if init_norm in (None, False) else float(init_norm),
                    validation_strength=float(getattr(cfg, "validation_lycoris_strength", 1.0) or 1.0))

    def _tlora_value(self, lc: dict, classes, amap: dict) -> dict:
        """`algo: tlora` of lycoris_value: {algo, classes, multiplier, linear_dim, linear_alpha, min_rank, alpha, num_train_timesteps, validation_strength}.
        multiplier, linear_dim and linear_alpha go through int(), as the reference's create_lycoris call site does (trainer.py:3410-3412); the mask settings are
        `tlora_min_rank` (default 1) and `tlora_alpha` (default 1.0) of the JSON, T is the noise schedule's num_train_timesteps."""
        cfg = self.config
        for c in classes:
            for k in ("linear_dim", "linear_alpha", "tlora_min_rank", "tlora_alpha"):
                if k in (amap.get(c) or {}) and (k not in lc or amap[c][k] != lc[k]):
                    raise NotImplementedError(f"lycoris_config apply_preset.module_algo_map.{c}.{k}={amap[c][k]}: a per-class {k} is not built on the st355 path (one "
                                              f"rank table per component); set \"{k}\" at the top level only")
        linear_dim = int(lc.get("linear_dim", 4))
        linear_alpha = int(lc.get("linear_alpha", 1))
        min_rank, alpha = int(lc.get("tlora_min_rank", 1)), float(lc.get("tlora_alpha", 1.0))
        if not 1 <= min_rank <= linear_dim:
            raise ValueError(f"lycoris_config tlora_min_rank={min_rank}: must lie in [1, linear_dim = {linear_dim}]; set \"tlora_min_rank\" inside that range")
        if not alpha > 0.0:
            raise ValueError(f"lycoris_config tlora_alpha={alpha}: must be positive; set \"tlora_alpha\" above 0")
        from .scheduled_sampling import num_train_timesteps_of
        return dict(algo="tlora", classes=list(classes), multiplier=int(lc.get("multiplier", 1.0)), linear_dim=linear_dim, linear_alpha=linear_alpha,
                    min_rank=min_rank, alpha=alpha, num_train_timesteps=num_train_timesteps_of(getattr(self, "noise_schedule", None)),
                    validation_strength=float(getattr(cfg, "validation_lycoris_strength", 1.0) or 1.0))

    def _tlora_of_component(self):
        """the trained component's engine.TLora state, None without a T-LoRA adapter (or before the component exists)"""
        try:
            comp = self.get_trained_component()
        except Exception:
            comp = None
        return getattr(self.unwrap_model(comp), "lora_tlora", None) if comp is not None else None

    ROLLOUT_BATCH_KEYS = None           # families with the scheduled-sampling rollout (Flux, SD3): the per-sample batch entries their model_predict reads

    def twinflow_value(self) -> bool:
        """`twinflow_enabled` as the step takes it: False when absent (nothing is imported then); else the reference's checks with its texts
        (`_validate_twinflow_config`, common.py:5105-5140) and every configuration the teacher forwards / the kernels are not built for refused by the flag's name
        and the value to set (twinflow.refuse_unbuilt) — never a silently different computation.  Built: the flow-matching families with the rollout's batch
        keys (SD3, Flux), model_type=lora, standard LoRA."""
        if not getattr(self.config, "twinflow_enabled", False):
            return False
        from .twinflow import refuse_unbuilt
        flow = self.PREDICTION_TYPE is PredictionTypes.FLOW_MATCHING
        refuse_unbuilt(self.config, self.NAME, flow, flow and self.ROLLOUT_BATCH_KEYS is not None)
        return True

    def scheduled_sampling_value(self):
        """`scheduled_sampling_max_step_offset` / `scheduled_sampling_reflexflow` as the step takes them: (max offset, ReflexFlow on).  Applies the reference's
        default-on rule (`_maybe_enable_reflexflow_default`, common.py:5376-5397: a positive offset on a flow-matching family sets the flag unless the user set it),
        and refuses by the flag's name every configuration the rollout / the loss terms are not built for — never a silently different computation."""
        cfg = self.config
        try:
            offset = float(getattr(cfg, "scheduled_sampling_max_step_offset", 0) or 0)
        except Exception:
            offset = 0.0
        if (offset > 0 and getattr(cfg, "scheduled_sampling_reflexflow", None) is None and self.PREDICTION_TYPE is PredictionTypes.FLOW_MATCHING
                and self.ROLLOUT_BATCH_KEYS is not None):
            setattr(cfg, "scheduled_sampling_reflexflow", True)
        reflex = bool(getattr(cfg, "scheduled_sampling_reflexflow", False))
        if not (offset > 0 or reflex):
            return 0, False
        flag = f"scheduled_sampling_max_step_offset={getattr(cfg, 'scheduled_sampling_max_step_offset', 0)}" if offset > 0 else "scheduled_sampling_reflexflow"
        if self.PREDICTION_TYPE is not PredictionTypes.FLOW_MATCHING or self.ROLLOUT_BATCH_KEYS is None:
            raise NotImplementedError(f"{flag}: scheduled sampling is not built for {self.NAME} on the st355 path (built: Flux, SD3) — the epsilon / v rollout needs "
                                      "skrample's samplers; unset scheduled_sampling_max_step_offset and scheduled_sampling_reflexflow")
        if getattr(cfg, "hip_graph", False):
            raise NotImplementedError(f"{flag} with hip_graph: the rollout is host-driven and its length is drawn per step, it cannot be captured")
        tc = getattr(cfg, "tread_config", None)
        if tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)):
            raise NotImplementedError(f"{flag} with TREAD routing: the reference's rollout forwards are training-mode forwards that route tokens, which the no-grad "
                                      "route of the st355 path does not; not built")
        # (as lora_dropout_value: a full fine-tune and lora_type=lycoris ignore lora_dropout, so no dropout would run there)
        if (float(getattr(cfg, "lora_dropout", 0.0) or 0.0) > 0.0 and "lora" in str(getattr(cfg, "model_type", "lora"))
                and str(getattr(cfg, "lora_type", "standard") or "standard").lower() == "standard"):
            raise NotImplementedError(f"{flag} with lora_dropout={getattr(cfg, 'lora_dropout')}: the reference's rollout forwards are training-mode forwards that drop, "
                                      "which the no-grad route of the st355 path does not; not built")
        if self._tlora_of_component() is not None:
            raise NotImplementedError(f"{flag} with lycoris algo=tlora: the reference's rollout forwards run without the timestep rank mask, which every forward of a "
                                      "T-LoRA component of the st355 path applies; not built")
        if getattr(cfg, "twinflow_enabled", False):
            raise NotImplementedError(f"{flag} with twinflow_enabled: TwinFlow is not built on the st355 path")
        if getattr(cfg, "controlnet", False):
            raise NotImplementedError(f"{flag} with controlnet: the rollout through controlnet_predict is not built on the st355 path")
        return int(offset), reflex

    def _scheduled_sampling_refuse_tokenwise(self, batch: dict):
        t = batch.get("timesteps")
        if getattr(t, "ndim", 1) != 1:
            raise NotImplementedError(f"scheduled_sampling_max_step_offset / scheduled_sampling_reflexflow with tokenwise timesteps {tuple(t.shape)}: the rollout "
                                      "re-times whole samples and the ReflexFlow terms are per sample; not built on the st355 path")

    def apply_scheduled_sampling_rollout(self, prepared_batch: dict) -> dict:
        """trainer.py:6059 `apply_scheduled_sampling_rollout`, between prepare_batch and model_predict: a no-op without a plan"""
        if not prepared_batch or prepared_batch.get("scheduled_sampling_plan") is None:
            return prepared_batch
        self.scheduled_sampling_value()
        self._scheduled_sampling_refuse_tokenwise(prepared_batch)
        from .scheduled_sampling import apply_flow_rollout
        prepared_batch = apply_flow_rollout(self, prepared_batch, self.noise_schedule, self.config)
        prepared_batch["_scheduled_sampling_rolled"] = True
        return prepared_batch

    def lora_dropout_value(self) -> float:
        """`lora_dropout` (the reference builds every standard LoRA with LoraConfig(lora_dropout=...): common.py:1094-1104) as the family's add_lora_adapter takes
        it: 0.0 when absent; a full fine-tune and lora_type=lycoris ignore the flag, as the reference does; a standard LoRA of a family without the masked kernels
        refuses a positive value by name — never a silently different computation."""
        cfg = self.config
        if getattr(cfg, "distillation_method", None):          # safety_check.py:23-49: a distillation method trains its adapters without dropout (self_transcendence included)
            from .flow_dpo import adapter_dropout_override, method_of
            if method_of(cfg) is not None:
                adapter_dropout_override(cfg)
        p = float(getattr(cfg, "lora_dropout", 0.0) or 0.0)
        if "lora" not in str(getattr(cfg, "model_type", "lora")) or str(getattr(cfg, "lora_type", "standard") or "standard").lower() != "standard":
            return 0.0
        if not 0.0 <= p < 1.0:
            raise ValueError(f"lora_dropout must lie in [0, 1), got {p}")
        if p > 0.0 and not self.LORA_DROPOUT_BUILT:
            raise NotImplementedError(f"lora_dropout={p}: LoRA dropout is not built for {self.NAME} on the st355 path (built: SD3); set --lora_dropout=0")
        return p

    def _crepa_source(self) -> str:
        """crepa.py `CrepaFeatureSource.from_config` (its ValueErrors included); imported only under `crepa_enabled`"""
        from .self_flow import feature_source
        return feature_source(self.config)

    SELF_FLOW_BUILT = False             # families whose engine runs the teacher capture and the alignment tap (SD3)

    def _self_flow_init(self):
        """common.py `_validate_crepa_configuration` + crepa.py `attach_to_model`: the reference's checks with its texts, then what this path does not take, refused
        by the flag's name; the component was told its blocks when it was built (`set_self_flow`, ahead of the adapter arena)"""
        from .self_flow import WeightSchedule, mask_ratio, validate
        cfg = self.config
        validate(cfg, self.NAME, True)
        if getattr(cfg, "crepa_block_index", None) is None:
            raise ValueError("crepa_block_index must be set when CREPA is enabled.")
        comp = self.get_trained_component()
        comp = None if comp is None else self.unwrap_model(comp)
        if not self.SELF_FLOW_BUILT or comp is None or not hasattr(comp, "set_self_flow"):
            raise NotImplementedError(f"crepa_enabled: Self-Flow (crepa_feature_source=self_flow) is not built for {self.NAME} on the st355 path (built: SD3 LoRA)")
        no = lambda what: NotImplementedError(f"crepa_enabled (self_flow) {what} is not built on the st355 path")
        if "lora" not in str(getattr(cfg, "model_type", "lora")):
            raise no("under a full fine-tune (tokenwise timesteps need per-token modulation gradients)")
        if str(getattr(cfg, "lora_type", "standard") or "standard").lower() != "standard":
            raise no("with lora_type=lycoris (LoKr / T-LoRA: the teacher forward packs standard LoRA operands from the EMA shadow; T-LoRA refuses tokenwise timesteps)")
        if any(getattr(b, "dual", False) for b in getattr(comp, "blocks", ())):
            raise no("with SD3.5 dual-attention blocks (they refuse tokenwise timesteps)")
        if getattr(cfg, "use_dora", False):
            raise no("with use_dora (the DoRA fold does not take the EMA shadow)")
        if float(getattr(cfg, "lora_dropout", 0.0) or 0.0) > 0.0:
            raise no(f"with lora_dropout={getattr(cfg, 'lora_dropout')} (the teacher forward is a no-grad forward that does not drop)")
        for flag, name in (("layersync_enabled", "LayerSync"), ("internal_guidance_enabled", "Internal Guidance"), ("nextlat_enabled", "NextLat")):
            if getattr(cfg, flag, False):
                raise no(f"together with {flag} ({name} refuses tokenwise timesteps or claims the same arena tail)")
        if getattr(cfg, "hip_graph", False):
            raise NotImplementedError("hip_graph: Self-Flow (crepa_enabled) reads its similarity on the host every step and cannot be captured")
        tc = getattr(cfg, "tread_config", None)
        if tc and (tc.get("routes", None) if isinstance(tc, dict) else getattr(tc, "routes", None)):
            raise no("with TREAD routing (tokenwise timesteps under a route)")
        if getattr(getattr(self, "xm_config", None), "enabled", False):
            raise ValueError(f"{self.NAME} XM noise-candidate training is not compatible with CREPA self-flow.")
        try:
            ss = float(getattr(cfg, "scheduled_sampling_max_step_offset", 0) or 0) > 0 or bool(getattr(cfg, "scheduled_sampling_reflexflow", False))
        except Exception:
            ss = False
        if ss:
            raise no("with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow: the rollout re-times whole samples)")
        if getattr(cfg, "distillation_method", None):
            raise no(f"with distillation_method={getattr(cfg, 'distillation_method')} (Flow-DPO doubles the batch with per-sample timesteps)")
        if getattr(cfg, "mixflow_enabled", False) is True:
            raise no("with mixflow_enabled (MixFlow re-draws the per-sample sigmas the views are built from)")
        if not getattr(comp, "lora_groups", None) or getattr(comp, "_sf", None) is None:
            # an ordering requirement of this path: the projector lives at the tail of the adapter arena, which add_lora_adapter lays out after load_model told the
            # component its blocks
            raise NotImplementedError("crepa_enabled: post_model_load_setup while the component has no adapter arena with the projector yet is not built on the st355 "
                                      "path — load_model, then add the LoRA adapters, then set Self-Flow up")
        comp.set_self_flow(cfg.crepa_block_index, cfg.crepa_teacher_block_index)          # (the projector exists: validates, and moves the taps)
        self.self_flow = SimpleNamespace(block_index=int(cfg.crepa_block_index), teacher_block_index=int(cfg.crepa_teacher_block_index), mask_ratio=mask_ratio(cfg),
                                         schedule=WeightSchedule(cfg, int(getattr(cfg, "max_train_steps", 0) or 0)), patch_size=int(getattr(comp.config, "patch_size", 2)))

    def _self_flow_views(self, batch: dict, state: dict, lat, noise, sig):
        """common.py `_prepare_image_crepa_self_flow_batch` on one kernel pass (ops.self_flow_views): a second (sigma, timestep) draw, the token mask's uniforms, then
        the student's mixed view with its [B, S_img] timesteps and the teacher's cleaner homogeneous view.  Nothing is read on the host."""
        sf, dev = self.self_flow, lat.device
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        t0 = f32(batch["timesteps"])
        alt_s, alt_t = batch.get("crepa_alt_sigmas"), batch.get("crepa_alt_timesteps")          # (tests / parity runs inject the draws, like the noise)
        if alt_s is None or alt_t is None:
            alt_s, alt_t = self.sample_flow_sigmas(batch=batch, state=state)
        B, _, H, W = lat.shape
        p = sf.patch_size
        u = batch.get("crepa_self_flow_uniforms")
        if u is None:
            u = torch.rand(B, max(H // p, 1), max(W // p, 1), device=dev, dtype=torch.float32)
        noisy_s, noisy_t, tok, sig_T, t_T, _ = ops.self_flow_views(lat, noise, sig, f32(alt_s), t0, f32(alt_t), u.to(device=dev, dtype=torch.float32).contiguous(),
                                                                   sf.mask_ratio, p)
        batch["noisy_latents"], batch["timesteps"] = noisy_s, tok
        batch["sigmas"] = None          # (the reference leaves the student's [B, 1, H, W] sigma grid here; nothing reads it on this path, so it is not written)
        batch["crepa_teacher_noisy_latents"], batch["crepa_teacher_timesteps"], batch["crepa_teacher_sigmas"] = noisy_t, t_T, sig_T
        batch["crepa_global_step"] = int(state.get("global_step", 0))
        return batch

    def _nextlat_init(self):
        """common.py:5197-5220 `_init_nextlat_regularizer` + nextlat.py:95-116: the configuration checks in the reference's order and with its texts, then the
        trained component is told which block output feeds the predictor (the predictor itself was laid out with the component's arenas)"""
        cfg = self.config
        if self.MODEL_TYPE is not ModelTypes.TRANSFORMER:
            raise ValueError("NextLat is only supported for transformer model families.")
        if str(getattr(cfg, "lora_type", "standard") or "standard").lower() == "lycoris":
            raise ValueError("NextLat requires standard PEFT LoRA or full-model training so its predictor is optimized and saved.")
        comp = self.get_trained_component()
        if comp is None:
            raise ValueError("NextLat requires an attached transformer component.")
        comp = self.unwrap_model(comp)
        if not hasattr(comp, "set_nextlat"):
            raise NotImplementedError(f"nextlat_enabled: NextLat is not built for {self.NAME} on the st355 path (built: SD3)")
        if not (getattr(comp, "lora_groups", None) or getattr(comp, "full", False)):
            # an ordering requirement of this path, not one of the reference's checks: NextLat is set up once the arena that trains exists (adapters added, or the
            # full fine-tune enabled); set-up ahead of it is refused by the flag's name, like every configuration this path does not take
            raise NotImplementedError("nextlat_enabled: post_model_load_setup while the component has no trainable arena yet is not built on the st355 path — add the "
                                      "LoRA adapters (or enable the full fine-tune) first, then set NextLat up")
        weight = float(getattr(cfg, "nextlat_weight", None) or 0.0)
        if weight <= 0:
            raise ValueError("nextlat_weight must be greater than zero when NextLat is enabled.")
        from .engine import nextlat_index
        idx = nextlat_index(getattr(cfg, "nextlat_block_index", None), int(comp.config.num_layers))          # (the rule, the range check and its text live there)
        state_loss = str(getattr(cfg, "nextlat_state_loss", None) or "smooth_l1")
        if state_loss not in ("smooth_l1", "mse"):
            raise ValueError("nextlat_state_loss must be 'smooth_l1' or 'mse'.")
        kl = float(getattr(cfg, "nextlat_kl_weight", None) or 0.0)
        if kl < 0:
            raise ValueError("nextlat_kl_weight must be non-negative.")
        if kl > 0:          # nextlat.py:171-173: no diffusion family puts a logits head into its model output, so the reference raises this at the first step
            raise ValueError("nextlat_kl_weight requires model_output['nextlat_logits_head'].")
        if getattr(cfg, "internal_guidance_enabled", False):
            raise NotImplementedError("nextlat_enabled together with internal_guidance_enabled is not built on the st355 path (both heads claim the tail of the arena that trains)")
        tc = getattr(cfg, "tread_config", None)
        if tc and tc.get("routes", None):
            raise NotImplementedError("nextlat_enabled with TREAD routing (the routed block's token rows are no longer neighbours in the sequence) is not built on the st355 path")
        if getattr(getattr(self, "xm_config", None), "enabled", False):
            raise NotImplementedError("nextlat_enabled with XM noise candidates is not built on the st355 path")
        comp.set_nextlat(getattr(cfg, "nextlat_block_index", None), state_loss)
        self.nextlat = SimpleNamespace(weight=weight, block_index=idx, state_loss=state_loss)

    def internal_guidance_block_index(self, n_blocks: int) -> int:
        """internal_guidance.py:194-197: `internal_guidance_block_index` as it is (0-based), default max(0, n_blocks // 4)"""
        from .engine import internal_guidance_index
        configured = getattr(self.config, "internal_guidance_block_index", None)
        return internal_guidance_index(configured if configured is not None else max(0, n_blocks // 4), n_blocks)          # (the range check and its text live there)

    def _internal_guidance_init(self):
        """common.py:5166-5195 `_init_internal_guidance_regularizer` + internal_guidance.py:186-199: the configuration checks in the reference's order and with its
        texts, then the trained component is told which block output feeds the head (the head itself was laid out with the component's arenas)"""
        cfg = self.config
        if self.MODEL_TYPE is not ModelTypes.TRANSFORMER:
            raise ValueError("Internal Guidance is only supported for diffusion transformer models.")
        if getattr(self.PREDICTION_TYPE, "value", None) == "autoregressive_next_token":          # (no st355 family has it; a registered reference family may)
            raise ValueError("Internal Guidance is not defined for autoregressive next-token models.")
        if str(getattr(cfg, "lora_type", "standard") or "standard").lower() == "lycoris":
            raise ValueError("Internal Guidance requires standard PEFT LoRA or full-model training so its auxiliary head is optimized and saved.")
        comp = self.unwrap_model(self.get_trained_component()) if self.get_trained_component() is not None else None
        if comp is None or not hasattr(comp, "set_internal_guidance"):
            raise NotImplementedError(f"internal_guidance_enabled: Internal Guidance is not built for {self.NAME} on the st355 path (built: SD3)")
        weight = float(getattr(cfg, "internal_guidance_loss_weight", 0.5) or 0.0)
        if weight <= 0:
            raise ValueError("internal_guidance_loss_weight must be greater than zero.")
        tc = getattr(cfg, "tread_config", None)
        if tc and tc.get("routes", None):
            raise NotImplementedError("internal_guidance_enabled with TREAD routing (the routed block's token count no longer matches the diffusion target) is not built on the st355 path")
        if getattr(getattr(self, "xm_config", None), "enabled", False):
            raise NotImplementedError("internal_guidance_enabled with XM noise candidates is not built on the st355 path")
        idx = self.internal_guidance_block_index(int(comp.config.num_layers))
        comp.set_internal_guidance(idx)
        self.internal_guidance = SimpleNamespace(weight=weight, block_index=idx)

    @staticmethod
    def _layersync_resolve(idx, role: str, n_blocks: int) -> int:
        """layersync.py:72-93 `_resolve_layer` over the layers the reference captures for it (common.py:5237-5243: idx and idx - 1): an index i > 0 names the
        0-based block i - 1 (depths start at 1), 0 names block 0"""
        if idx is None:
            raise ValueError(f"LayerSync could not find {role} layer because no index was provided.")
        try:
            i = int(idx)
        except Exception as exc:
            raise ValueError(f"LayerSync {role} index {idx!r} is not an int.") from exc
        candidates = ([i - 1] if i > 0 else []) + [i]
        for cand in candidates:
            if 0 <= cand < n_blocks:
                return cand
        raise ValueError(f"LayerSync could not find {role} layer at indices {candidates}.")

    def _layersync_init(self):
        """layersync.py:14-25 (LayerSyncRegularizer.__init__) + the index resolution, then the trained component is told which two block outputs to align"""
        cfg = self.config
        comp = self.unwrap_model(self.get_trained_component()) if self.get_trained_component() is not None else None
        if comp is None or not hasattr(comp, "set_layersync"):
            raise NotImplementedError(f"layersync_enabled: LayerSync is not built for {self.NAME} on the st355 path (built: Flux, SD3)")
        tc = getattr(cfg, "tread_config", None)
        if tc and tc.get("routes", None):
            raise NotImplementedError("layersync_enabled with TREAD routing (the student and the teacher block would see different token subsets) is not built on the st355 path")
        student, teacher = getattr(cfg, "layersync_student_block", None), getattr(cfg, "layersync_teacher_block", None)
        weight = float(getattr(cfg, "layersync_lambda", 0.2) or 0.2)          # "match LayerSync paper default when enabled"
        if student is None:
            raise ValueError("layersync_student_block must be set when LayerSync is enabled.")
        if weight <= 0:
            raise ValueError("layersync_lambda must be greater than zero when LayerSync is enabled.")
        n = int(comp.config.num_layers) + int(getattr(comp.config, "num_single_layers", 0) or 0)
        s = self._layersync_resolve(student, "student", n)
        t = self._layersync_resolve(teacher if teacher is not None else student, "teacher", n)
        comp.set_layersync(s, t)
        self.layersync = SimpleNamespace(weight=weight, student=s, teacher=t)

    def post_quantization_setup(self):
        """common.py:3650"""
        return None

    def before_accelerator_prepare(self):
        """common.py:3697"""
        return None

    def refresh_representation_alignment_projectors(self):
        """common.py:939: CREPA / U-REPA projectors are not built on this path (no regulariser is attached): nothing to refresh"""
        return None

    def supports_grounding(self) -> bool:
        """common.py:1452.  GLIGEN grounding layers are out of the hot path: never advertised"""
        return False

    SUPPORTS_MUON_CLIP = False          # models/common.py: families opt in (the reference sets it on Flux only among the families built here)

    def enable_muon_clip_logging(self):
        """Flux publishes per-head max logits keyed by the base layer's `attn.to_q.weight` name (flux/transformer.py:192, training/qk_clip_logging.py).
        Under LoRA none of them names a trained parameter, so St355Muon's QK-clip never acts and nothing has to be collected: a no-op for the
        families that support Muon; the rest never reach it (the trainer refuses 'muon' for them first)"""
        if not self.SUPPORTS_MUON_CLIP:
            raise NotImplementedError(f"optimizer 'muon' is not supported by {type(self).__name__} on the st355 path")
        return None

    def configure_assistant_lora_for_training(self):
        if getattr(self.config, "assistant_lora_path", None) not in (None, "", "None"):
            raise NotImplementedError("assistant LoRA (schnell) is not implemented on the st355 path")

    def configure_group_offload(self):
        raise NotImplementedError("group offload targets small-memory cards; the st355 path keeps everything resident in the 288 GB of HBM")

    def _ramtorch_base_deferred_until_after_quantization(self) -> bool:
        return False

    def apply_ramtorch_to_transformer(self) -> bool:
        return False

    def apply_ramtorch_to_controlnet(self) -> bool:
        return False

    def controlnet_init(self, *a, **k):
        raise NotImplementedError(f"{self.NAME} has no ControlNet path on st355 (PixArt-Sigma has: pixart/model.py)")

    def tread_init(self):
        """<family>/model.py `tread_init` (e.g. sd3/model.py:326-347): hand the trained component a TREADRouter seeded from the run seed and the routes of
        `config.tread_config`.  Built for the components that expose `set_router` (SD3, Flux, the PixArt trunk under LoRA; training/tread.py); the others refuse — never a silent no-op."""
        tc = getattr(self.config, "tread_config", None)
        if not tc or tc.get("routes", None) is None:
            raise ValueError("TREAD training requires you to configure the routes in the TREAD config")
        comp = self.get_trained_component()
        if comp is None or not hasattr(comp, "set_router"):
            raise NotImplementedError(f"tread_init: TREAD routing is not implemented for {self.NAME} on the st355 path (built: SD3, Flux, the PixArt trunk)")
        from .training.tread import TREADRouter
        comp.set_router(TREADRouter(seed=getattr(self.config, "seed", None) or 42, device=self.accelerator.device), tc["routes"])

    def diffusion_blocks_init(self) -> None:
        if getattr(self.config, "diffusion_blocks_config", None):
            raise NotImplementedError("diffusion_blocks_config is not implemented on the st355 path")

    def apply_diffusion_blocks_trainable_filter(self) -> None:
        return None

    def get_pipeline(self, pipeline_type=None, load_base_model: bool = True):
        """common.py:4448.  Validation pipelines are diffusers objects (out of scope); the family-agnostic denoising loop over this plugin's own forward
        is simpletuner_amd.sampling.flow_match_euler_sample"""
        raise NotImplementedError("diffusers pipelines are not built on the st355 path; use simpletuner_amd.sampling.flow_match_euler_sample")

    def configure_gradient_checkpointing(self):
        """trainer.py:3635-3646 + common.py:3604-3636: `gradient_checkpointing` turns recomputation on for the trained component,
        `gradient_checkpointing_interval` (> 1) / `gradient_checkpointing_segment_stride` select the segmented modes, the backend must be the plain
        recompute one.  A family whose engine has no recompute path refuses instead of silently keeping every activation."""
        if not getattr(self.config, "gradient_checkpointing", False):
            return
        comp = self.get_trained_component()
        if comp is None or not hasattr(comp, "enable_gradient_checkpointing") or not hasattr(comp, "_checkpoint_segments"):
            raise NotImplementedError(f"gradient_checkpointing: {self.NAME} has no recompute path on the st355 path (built: Flux, SD3, PixArt-Sigma + its "
                                      f"ControlNet branch, the SDXL / SD1.x UNet); with 288 GB of HBM the step keeps its activations — drop the flag")
        comp.enable_gradient_checkpointing()
        interval = getattr(self.config, "gradient_checkpointing_interval", None)
        if interval is not None and int(interval) > 1:
            comp.set_gradient_checkpointing_interval(int(interval))
        stride = getattr(self.config, "gradient_checkpointing_segment_stride", None)
        if stride is not None:
            comp.set_gradient_checkpointing_segment_stride(int(stride))
        comp.set_gradient_checkpointing_backend(str(getattr(self.config, "gradient_checkpointing_backend", "torch") or "torch"))

    # ---- API parity with the reference plugin surface (common.py:3691-3781) ----
    def fuse_qkv_projections(self):
        """no-op: projections that share an input are ALWAYS stored and executed as one matrix on this path; the per-projection diffusers
        keys are views into it (PackedJointAttnProcessor2_0's fused to_qkv, packed_attention_processors.py:126-187)"""
        return None

    def unfuse_qkv_projections(self):
        return None

    # ---- LoRA checkpoints: the reference's layout (save_hooks.py:850-895 -> pipeline.save_lora_weights) ----
    LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"

    def lora_state_dict(self, component=None):
        """peft.get_peft_model_state_dict layout: `<module>.lora_A.weight` / `<module>.lora_B.weight` (the adapter name is dropped)"""
        comp = component if component is not None else self.get_trained_component()
        src = comp.lora_state_dict().items() if hasattr(comp, "lora_state_dict") else ((n, p.detach()) for n, p in comp.named_parameters() if ".lora_" in n)
        # (a component whose working layout pads the adapter factors — PixArt's 72 -> 96 head lanes — hands out the true peft shapes itself)
        # (a DoRA adapter's magnitudes: `<module>.lora_magnitude_vector.weight`, fp32 [out_features] — the spelling the reference's loader reads, adapter.py:170, 204-207)
        sd = {n.replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B.").replace(self.DORA_KEY + ".default.", self.DORA_KEY + "."): p for n, p in src}
        sd.update(self._internal_guidance_head_state(comp, next(iter(sd.values())).dtype if sd else torch.float32))
        sd.update(self._nextlat_predictor_state(comp, next(iter(sd.values())).dtype if sd else torch.float32))
        sd.update(self._self_flow_projector_state(comp, next(iter(sd.values())).dtype if sd else torch.float32))
        sd.update(self._self_transcendence_projector_state(comp, next(iter(sd.values())).dtype if sd else torch.float32))
        return sd

    DORA_KEY = ".lora_magnitude_vector"            # peft's DoraLinearLayer parameter, per adapted module

    IG_PREFIX = "internal_guidance_head."          # internal_guidance.py:184 MODULE_NAME; in an adapter file under `transformer.`

    @staticmethod
    def _internal_guidance_head_state(comp, dtype) -> dict:
        """the Internal Guidance head as the reference saves it with the adapter (its module's state dict under `internal_guidance_head.`): the four tensors in the
        dtype the adapter tensors are saved in and `block_index` as an int64 scalar.  Empty when the component trains no head with its adapters."""
        head = getattr(comp, "_ig", None)
        if head is None or not getattr(comp, "lora_groups", None):
            return {}
        own = dict(comp.named_parameters())
        out = {ModelFoundation.IG_PREFIX + nm: own[ModelFoundation.IG_PREFIX + nm].detach().to(dtype) for nm in ("norm.weight", "norm.bias", "proj.weight", "proj.bias")}
        out[ModelFoundation.IG_PREFIX + "block_index"] = torch.tensor(int(head.block), dtype=torch.int64)
        return out

    NEXTLAT_PREFIX = "nextlat_predictor."          # nextlat.py:93 MODULE_NAME; in an adapter file under `transformer.`

    @staticmethod
    def _nextlat_predictor_state(comp, dtype) -> dict:
        """the NextLat predictor as the reference saves it with the adapter (common.py:924-937 `modules_to_save`; here: its module's state dict under
        `nextlat_predictor.`, a layout not pinned against peft): the six tensors in the dtype the adapter tensors are saved in and `block_index` as an int64
        scalar.  Empty when the component trains no predictor with its adapters."""
        from .engine import NEXTLAT_NAMES
        head = getattr(comp, "_nl", None)
        if head is None or not getattr(comp, "lora_groups", None):
            return {}
        own = dict(comp.named_parameters())
        out = {ModelFoundation.NEXTLAT_PREFIX + nm: own[ModelFoundation.NEXTLAT_PREFIX + nm].detach().to(dtype) for nm in NEXTLAT_NAMES}
        out[ModelFoundation.NEXTLAT_PREFIX + "block_index"] = torch.tensor(int(head.block), dtype=torch.int64)
        return out

    COMFYUI_LORA_PRESERVE_COMPONENT_PREFIXES = None     # common.py:524; Flux / SD3 / PixArt keep their `transformer.` prefix in ComfyUI files
    AUTO_LORA_FORMAT_DETECTION = False                  # flux/model.py:56: a diffusers-configured run still recognises a ComfyUI file on load

    SELF_FLOW_PREFIX = "crepa_projector."          # crepa.py `attach_to_model`: setattr(model, "crepa_projector", nn.Sequential(LayerNorm, Linear)); under `transformer.` in a file

    @staticmethod
    def _self_flow_projector_state(comp, dtype) -> dict:
        """Self-Flow's projector as the reference saves it with the adapter (common.py:924-937 `get_lora_save_layers` names `crepa_projector` among the
        `modules_to_save`; here: the nn.Sequential's state dict under `crepa_projector.`, the route of the two heads above): `0.weight`, `0.bias`, `1.weight`,
        `1.bias` in the dtype the adapter tensors are saved in.  Empty when the component trains no projector."""
        from .engine import SELF_FLOW_NAMES
        if getattr(comp, "_sf", None) is None or not getattr(comp, "lora_groups", None):
            return {}
        own = dict(comp.named_parameters())
        return {ModelFoundation.SELF_FLOW_PREFIX + nm: own[ModelFoundation.SELF_FLOW_PREFIX + nm].detach().to(dtype) for nm in SELF_FLOW_NAMES}

    ST_PREFIX = "self_transcendence_projector."          # distiller.py PROJECTOR_NAME; under `transformer.` in a file

    @staticmethod
    def _self_transcendence_projector_state(comp, dtype) -> dict:
        """Self-Transcendence's projector as the reference saves it with the adapter (common.py:924-937 `get_lora_save_layers` names
        `self_transcendence_projector` among the `modules_to_save`; here: the module's state dict under that name): `net.{0,2,4}.{weight,bias}` in the dtype the
        adapter tensors are saved in.  Empty when the component trains no projector."""
        from .engine import ST_NAMES
        if getattr(comp, "_st", None) is None or not getattr(comp, "lora_groups", None):
            return {}
        own = dict(comp.named_parameters())
        return {ModelFoundation.ST_PREFIX + nm: own[ModelFoundation.ST_PREFIX + nm].detach().to(dtype) for nm in ST_NAMES}

    def _lora_adapter_metadata(self) -> dict:
        """what peft records for the adapter (LoraConfig r / lora_alpha): alpha defaults to the rank (common.py:1049-1128)"""
        r = int(getattr(self.config, "lora_rank", 0) or 0)
        alpha = getattr(self.config, "lora_alpha", None)
        return {"r": r, "lora_alpha": float(alpha if alpha is not None else r)}

    def _convert_lora_state_dict_to_comfyui(self, weights: dict, *, adapter_metadata=None, component_adapter_metadata=None) -> dict:
        from .training.lora_keys import convert_diffusers_to_comfyui
        return convert_diffusers_to_comfyui(weights, adapter_metadata=adapter_metadata,
                                            preserve_component_prefixes=self.COMFYUI_LORA_PRESERVE_COMPONENT_PREFIXES)

    def _convert_lora_state_dict_from_comfyui(self, weights: dict, *, target_prefix: str):
        from .training.lora_keys import convert_comfyui_to_diffusers
        return convert_comfyui_to_diffusers(weights, target_prefix=target_prefix)

    def save_lora_weights(self, output_dir, **layers):
        """writes `pytorch_lora_weights.safetensors` with diffusers' component prefix (`transformer.` / `unet.`), as the diffusers pipelines'
        save_lora_weights the reference calls (common.py:2072-2120); `layers` = {"<subfolder>_lora_layers": state} or nothing (= the trained
        component).  `config.lora_format == "comfyui"` converts the keys on the way out (ComfyUI / kohya names + one `.alpha` tensor per module); that export
        DROPS an Internal Guidance head / a NextLat predictor (`internal_guidance_head.*`, `nextlat_predictor.*`: ComfyUI has no module to load them into) — keep the diffusers-format file to resume or to sample
        with the head."""
        import os

        from safetensors.torch import save_file

        from .training.lora_keys import PEFTLoRAFormat, normalize_lora_format
        if not layers and getattr(self.unwrap_model(self.get_trained_component()), "lora_tlora", None) is not None:
            if normalize_lora_format(getattr(self.config, "lora_format", None)) == PEFTLoRAFormat.COMFYUI:
                raise NotImplementedError("lora_type=lycoris with lora_format=comfyui: the ComfyUI export of a T-LoRA adapter is not built on the st355 path; save with "
                                          "--lora_format=diffusers")
            os.makedirs(output_dir, exist_ok=True)
            path = os.path.join(output_dir, self.LORA_WEIGHT_NAME)
            save_file({k: v.detach().to("cpu").contiguous() for k, v in self.tlora_state_dict().items()}, path, metadata={"format": "pt"})
            return path
        if not layers and getattr(self.unwrap_model(self.get_trained_component()), "lora_lokr", False):
            if normalize_lora_format(getattr(self.config, "lora_format", None)) == PEFTLoRAFormat.COMFYUI:
                raise NotImplementedError("lora_type=lycoris with lora_format=comfyui: the ComfyUI export of a LoKr adapter is not built on the st355 path; save with "
                                          "--lora_format=diffusers")
            os.makedirs(output_dir, exist_ok=True)
            path = os.path.join(output_dir, self.LORA_WEIGHT_NAME)
            save_file({k: v.detach().to("cpu").contiguous() for k, v in self.lokr_state_dict().items()}, path, metadata={"format": "pt"})
            return path
        if not any(k.endswith("_lora_layers") for k in layers):
            layers = dict(layers, **{f"{self.MODEL_SUBFOLDER}_lora_layers": self.lora_state_dict()})
        flat, meta, comp_meta = {}, {}, {}
        for key, state in layers.items():
            if key.endswith("lora_adapter_metadata") and isinstance(state, dict):
                comp_meta[key[:-len("_lora_adapter_metadata")]] = state
                meta.update(state)
                continue
            if state is None or not key.endswith("_lora_layers"):
                continue
            prefix = key[:-len("_lora_layers")]
            for k, v in state.items():
                flat[f"{prefix}.{k}"] = v.detach().to("cpu").contiguous()
        fmt = normalize_lora_format(getattr(self.config, "lora_format", None))
        if fmt == PEFTLoRAFormat.COMFYUI and any(self.DORA_KEY in k for k in flat):
            raise NotImplementedError("use_dora: the ComfyUI export of a DoRA adapter (its magnitude vectors) is not built on the st355 path; save with "
                                      "--lora_format=diffusers")
        if fmt == PEFTLoRAFormat.COMFYUI and not getattr(self, "NATIVE_COMFYUI_LORA_SUPPORT", False):
            flat = {k: v for k, v in flat.items() if self.IG_PREFIX not in k and self.NEXTLAT_PREFIX not in k and self.SELF_FLOW_PREFIX not in k and self.ST_PREFIX not in k}
            flat = self._convert_lora_state_dict_to_comfyui(flat, adapter_metadata=meta or self._lora_adapter_metadata(), component_adapter_metadata=comp_meta)
            flat = {k: v.contiguous() for k, v in flat.items()}
        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir, self.LORA_WEIGHT_NAME)
        save_file(flat, path, metadata={"format": "pt"})
        return path

    LYCORIS_PREFIX = "lycoris_"                    # LyCORIS' module naming: `lycoris_` + the module path with '.' -> '_'
    LOKR_KEYS = (".lokr_w1", ".lokr_w2")

    def lokr_state_dict(self, component=None) -> dict:
        """a LoKr adapter as a LyCORIS file holds it: per adapted module `lycoris_<module path, '.' -> '_'>.lokr_w1`, `.lokr_w2` (fp32) and `.alpha` (a scalar,
        = linear_dim: with both factors full LyCORIS sets alpha = linear_dim).  The lay-out is restated from LyCORIS' naming rule, not pinned against the package."""
        comp = self.unwrap_model(component if component is not None else self.get_trained_component())
        sd = {}
        for n, p in comp.named_parameters():
            for key in self.LOKR_KEYS:
                if n.endswith(key):
                    mod = self.LYCORIS_PREFIX + n[:-len(key)].replace(".", "_")
                    sd[mod + key] = p.detach()
                    sd[mod + ".alpha"] = torch.tensor(float(getattr(comp, "lokr_linear_dim", 10000)), dtype=torch.float32)
        return sd

    def _load_lokr_weights(self, comp, flat: dict):
        """strict both ways: every factor of the component is in the file with its shape, and the file holds nothing else"""
        own = {}
        for n, p in comp.named_parameters():
            for key in self.LOKR_KEYS:
                if n.endswith(key):
                    own[self.LYCORIS_PREFIX + n[:-len(key)].replace(".", "_") + key] = p
        alphas = {k[:-len(key)] + ".alpha" for k in own for key in self.LOKR_KEYS if k.endswith(key)}
        missing = [k for k in list(own) + sorted(alphas) if k not in flat]
        if missing:
            raise KeyError(f"LyCORIS checkpoint is missing {len(missing)} adapter tensors, e.g. {missing[:3]}")
        extra = [k for k in flat if k not in own and k not in alphas]
        if extra:
            raise KeyError(f"LyCORIS checkpoint holds {len(extra)} tensors the adapter has no place for, e.g. {extra[:3]}; the lycoris_config (target_module) must match "
                           "the one the file was trained with")
        for k, p in own.items():
            if tuple(flat[k].shape) != tuple(p.shape):
                raise ValueError(f"LyCORIS checkpoint tensor {k} has shape {tuple(flat[k].shape)}, the adapter's is {tuple(p.shape)}: the lycoris_config factor must match "
                                 "the one the file was trained with")
        want = float(getattr(comp, "lokr_linear_dim", 10000))
        for k in sorted(alphas):
            if float(flat[k]) != want:
                raise ValueError(f"LyCORIS checkpoint alpha {float(flat[k])} ({k}) differs from the configured linear_dim {want}; set linear_dim to match the file")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(flat[k].to(device=p.device, dtype=p.dtype))
        return comp

    TLORA_KEYS = (".lora_down.weight", ".lora_up.weight")

    def tlora_state_dict(self, component=None) -> dict:
        """a T-LoRA adapter as a LyCORIS file holds a LoCon module: per adapted module `lycoris_<module path, '.' -> '_'>.lora_down.weight` [r, in],
        `.lora_up.weight` [out, r] (fp32) and `.alpha` (a scalar = linear_alpha).  The lay-out is restated from LyCORIS' naming rule, not pinned against the package."""
        comp = self.unwrap_model(component if component is not None else self.get_trained_component())
        sd = {}
        for n, p in comp.named_parameters():
            for key in self.TLORA_KEYS:
                if n.endswith(key):
                    mod = self.LYCORIS_PREFIX + n[:-len(key)].replace(".", "_")
                    sd[mod + key] = p.detach()
                    sd[mod + ".alpha"] = torch.tensor(float(comp.tlora_linear_alpha), dtype=torch.float32)
        return sd

    def _load_tlora_weights(self, comp, flat: dict):
        """strict both ways: every matrix of the component is in the file with its shape, the file holds nothing else, and every alpha is the configured one"""
        own = {}
        for n, p in comp.named_parameters():
            for key in self.TLORA_KEYS:
                if n.endswith(key):
                    own[self.LYCORIS_PREFIX + n[:-len(key)].replace(".", "_") + key] = p
        alphas = {k[:-len(key)] + ".alpha" for k in own for key in self.TLORA_KEYS if k.endswith(key)}
        missing = [k for k in list(own) + sorted(alphas) if k not in flat]
        if missing:
            raise KeyError(f"LyCORIS checkpoint is missing {len(missing)} adapter tensors, e.g. {missing[:3]}; the lycoris_config (target_module) must match the one "
                           "the file was trained with")
        extra = [k for k in flat if k not in own and k not in alphas]
        if extra:
            raise KeyError(f"LyCORIS checkpoint holds {len(extra)} tensors the adapter has no place for, e.g. {extra[:3]}; the lycoris_config (target_module) must match "
                           "the one the file was trained with")
        for k, p in own.items():
            if tuple(flat[k].shape) != tuple(p.shape):
                raise ValueError(f"LyCORIS checkpoint tensor {k} has shape {tuple(flat[k].shape)}, the adapter's is {tuple(p.shape)}: the lycoris_config linear_dim must "
                                 "match the one the file was trained with")
        want = float(comp.tlora_linear_alpha)
        for k in sorted(alphas):
            if float(flat[k]) != want:
                raise ValueError(f"LyCORIS checkpoint alpha {float(flat[k])} ({k}) differs from the configured linear_alpha {want}; set linear_alpha to match the file")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(flat[k].to(device=p.device, dtype=p.dtype))
        return comp

    def _kohya_name_map(self) -> dict:
        """kohya module name -> this component's module path, built forwards from the adapters that exist (the underscore-joined kohya spelling
        cannot be split back into a dotted path on its own)"""
        out = {}
        for n, _p in self.get_trained_component().named_parameters():
            if ".lora_A." in n:
                module = n[:n.index(".lora_A.")]
                out["lora_unet_" + module.replace(".processor.", ".").replace(".", "_")] = module
        return out

    def load_lora_weights(self, models=None, input_dir=None):
        """common.py:1875-2047: read the file back into the adapters of the trained component (strict on the adapter keys).  ComfyUI-dialect files
        (configured, or detected when AUTO_LORA_FORMAT_DETECTION) are converted first; a per-module alpha that disagrees with the configured
        adapter scale is an error here — the adapters' alpha/r scale is fixed at construction, loading must not silently change the model.  An Internal Guidance
        head is read back strictly from a diffusers-format file; a ComfyUI-dialect file cannot carry one and is refused while a head is configured."""
        import os

        from safetensors.torch import load_file

        from .training.lora_keys import PEFTLoRAFormat, detect_state_dict_format, normalize_lora_format, to_peft_keys
        comp = self.get_trained_component()
        flat = load_file(os.path.join(input_dir, self.LORA_WEIGHT_NAME))
        prefix = f"{self.MODEL_SUBFOLDER}."
        file_tlora = any(k.startswith(self.LYCORIS_PREFIX) and k.endswith(self.TLORA_KEYS) for k in flat)
        own_tlora = getattr(self.unwrap_model(comp), "lora_tlora", None) is not None
        if own_tlora and any(k.endswith(self.LOKR_KEYS) for k in flat):
            raise ValueError("lycoris_config algo=tlora is set but the checkpoint carries LyCORIS LoKr factors (lokr_w1 / lokr_w2): set \"algo\": \"lokr\" in the "
                             "lycoris_config to load it")
        if file_tlora and not own_tlora:
            if getattr(self.unwrap_model(comp), "lora_lokr", False):
                raise ValueError("lycoris_config algo=lokr is set but the checkpoint carries LyCORIS low-rank pairs (lora_down / lora_up: a T-LoRA file): set "
                                 "\"algo\": \"tlora\" in the lycoris_config to load it")
            raise ValueError("LoRA checkpoint carries LyCORIS low-rank pairs (lycoris_*.lora_down / lora_up: a T-LoRA file) but the adapter was built as a standard "
                             "LoRA: set --lora_type=lycoris (and a lycoris_config with \"algo\": \"tlora\") before loading it")
        if own_tlora and not file_tlora:
            raise ValueError("lycoris_config algo=tlora is set but the checkpoint carries no LyCORIS low-rank pairs (lycoris_*.lora_down / lora_up): it is a standard "
                             "LoRA file; set --lora_type=standard to load it")
        if own_tlora:
            return self._load_tlora_weights(self.unwrap_model(comp), flat)
        file_lokr, own_lokr = any(k.endswith(self.LOKR_KEYS) for k in flat), bool(getattr(self.unwrap_model(comp), "lora_lokr", False))
        if file_lokr and not own_lokr:
            raise ValueError("LoRA checkpoint carries LyCORIS LoKr factors (lokr_w1 / lokr_w2) but the adapter was built as a standard LoRA: set --lora_type=lycoris "
                             "(and lycoris_config) before loading it")
        if own_lokr and not file_lokr:
            raise ValueError("lora_type=lycoris is set but the checkpoint carries no LoKr factors (lokr_w1 / lokr_w2): it is a standard LoRA file; set "
                             "--lora_type=standard to load it")
        if own_lokr:
            return self._load_lokr_weights(self.unwrap_model(comp), flat)
        fmt = normalize_lora_format(getattr(self.config, "lora_format", None))
        if fmt == PEFTLoRAFormat.DIFFUSERS and self.AUTO_LORA_FORMAT_DETECTION and detect_state_dict_format(flat) == PEFTLoRAFormat.COMFYUI:
            fmt = PEFTLoRAFormat.COMFYUI
        if fmt == PEFTLoRAFormat.COMFYUI:
            alphas = {}
            if any(k.startswith("lora_unet_") for k in flat):                 # kohya names (SD / SDXL export)
                back, conv = self._kohya_name_map(), {}
                for k, v in flat.items():
                    name, _, tail = k.partition(".")
                    if name not in back:
                        continue
                    if tail == "alpha":
                        alphas[f"{prefix}{back[name]}.alpha"] = float(v)
                    else:
                        conv[f"{prefix}{back[name]}." + {"lora_down.weight": "lora_A.weight", "lora_up.weight": "lora_B.weight"}[tail]] = v
                flat = conv
            else:
                flat, alphas = self._convert_lora_state_dict_from_comfyui(flat, target_prefix=self.MODEL_SUBFOLDER)
                flat = to_peft_keys(flat)
            want = self._lora_adapter_metadata()["lora_alpha"]
            bad = {k: a for k, a in alphas.items() if want and abs(a - want) > 1e-6}
            if bad:
                k0 = next(iter(bad))
                raise ValueError(f"LoRA file alpha {bad[k0]} for {k0} differs from the configured lora_alpha {want}; set lora_alpha to match the file")
        own = {n.replace(".lora_A.default.", ".lora_A.").replace(".lora_B.default.", ".lora_B.").replace(self.DORA_KEY + ".default.", self.DORA_KEY + "."): p
               for n, p in comp.named_parameters() if ".lora_" in n}
        # DoRA: the magnitudes travel as `<module>.lora_magnitude_vector.weight` (also accepted: the key without `.weight`); a file and a component must agree
        flat = {(k + ".weight" if k.endswith(self.DORA_KEY) else k): v for k, v in flat.items()}
        file_dora, own_dora = any(self.DORA_KEY in k for k in flat), any(self.DORA_KEY in k for k in own)
        if file_dora and not own_dora:
            raise ValueError("LoRA checkpoint carries DoRA magnitude vectors (lora_magnitude_vector) but the adapter was built without them: set --use_dora=true "
                             "before loading it")
        if own_dora and not file_dora:
            raise ValueError("use_dora is set but the LoRA checkpoint carries no DoRA magnitude vectors (lora_magnitude_vector): it is a plain LoRA file; set "
                             "--use_dora=false to load it")
        # an Internal Guidance head / a NextLat predictor travels with the adapter (diffusers-format files): read back strictly — every tensor of it when one is
        # configured, and a file that carries one needs a component that has one
        for pre, attr, a, name, flag, key in ((self.IG_PREFIX, "_ig", "an", "Internal Guidance head", "internal_guidance_enabled", "internal_guidance_block_index"),
                                              (self.NEXTLAT_PREFIX, "_nl", "a", "NextLat predictor", "nextlat_enabled", "nextlat_block_index"),
                                              (self.SELF_FLOW_PREFIX, "_sf", "a", "Self-Flow projector", "crepa_enabled", None),
                                              (self.ST_PREFIX, "_st", "a", "Self-Transcendence projector", "distillation_method=self_transcendence", None)):
            in_file = sorted(k for k in flat if pre in k)
            head = getattr(comp, attr, None)
            if in_file and (head is None or not getattr(comp, "lora_groups", None)):
                raise ValueError(f"LoRA checkpoint carries {a} {name} ({in_file[0]}, ...) but none is configured: set {flag} (and the "
                                 f"file's {key or ('student_block' if attr == '_st' else 'crepa_block_index')}) before loading it")
            if head is not None and getattr(comp, "lora_groups", None) and fmt != PEFTLoRAFormat.DIFFUSERS:
                raise ValueError(f"a ComfyUI-format LoRA file cannot carry the {name} (the export drops it): load the diffusers-format file, or turn "
                                 f"{flag} off to load the adapters alone")
            if head is not None and getattr(comp, "lora_groups", None):
                own.update({n: p for n, p in comp.named_parameters() if n.startswith(pre)})
                if key is None:          # (the reference's nn.Sequential projector carries no block index)
                    continue
                bi = flat.get(prefix + pre + "block_index")
                if bi is None:
                    raise KeyError(f"LoRA checkpoint is missing the {name}'s block index ({prefix}{pre}block_index)")
                if int(bi.item()) != int(head.block):
                    raise ValueError(f"LoRA checkpoint's {name} was trained on block {int(bi.item())}, the configured {key} is {int(head.block)}")
        missing = [k for k in own if prefix + k not in flat]
        if missing:
            raise KeyError(f"LoRA checkpoint is missing {len(missing)} adapter tensors, e.g. {missing[:3]}")
        with torch.no_grad():
            if hasattr(comp, "load_lora_state_dict"):              # working layout differs from the peft shapes (PixArt's head padding)
                comp.load_lora_state_dict({k: flat[prefix + k] for k in own})
            else:
                for k, p in own.items():
                    p.copy_(flat[prefix + k].to(device=p.device, dtype=p.dtype))
        return comp

    def uses_noise_schedule(self) -> bool:
        return self.PREDICTION_TYPE is not PredictionTypes.FLOW_MATCHING

    def setup_training_noise_schedule(self):
        """common.py:4518-4556: the TRAINING schedule — DDPM coefficients for epsilon / v families; for flow matching the Euler scheduler with the
        static shift, its bounds reset to the unshifted ones (fix_flow_match_euler_schedule_bounds)"""
        if self.PREDICTION_TYPE is not PredictionTypes.FLOW_MATCHING:
            self.noise_schedule = DDPMSchedule(prediction_type=self.PREDICTION_TYPE.value, device=self.accelerator.device,
                                               rescale_betas_zero_snr=bool(getattr(self.config, "rescale_betas_zero_snr", False)))
            if getattr(self.config, "diff2flow_enabled", False):
                self.diff2flow_value()                               # common.py:563-564: the bridge (and its refusals) when the schedule is set up
        else:
            from .sampling import FlowMatchEulerDiscreteScheduler, fix_flow_match_euler_schedule_bounds
            self.noise_schedule = fix_flow_match_euler_schedule_bounds(
                FlowMatchEulerDiscreteScheduler(shift=float(getattr(self.config, "flow_schedule_shift", None) or 1.0)))
        return self.noise_schedule

    def flow_matching_target_direction(self) -> float:
        return 1.0

    def diff2flow_value(self):
        """`diff2flow_enabled` as the step takes it (setup_diff2flow_bridge, common.py:4558-4574): the Diff2FlowBridge over the training schedule on an epsilon / v
        family with the flag set, else None — on a flow-matching family the flag (and `diff2flow_loss`) does nothing.  diffusers' DDPM schedule always carries
        alphas_cumprod; a schedule without it switches the flag off with the reference's warning.  Refuses, by the flags' names, what the tables cannot carry."""
        if not getattr(self.config, "diff2flow_enabled", False) or self.PREDICTION_TYPE not in (PredictionTypes.EPSILON, PredictionTypes.V_PREDICTION):
            return None
        from .diff2flow import resolve_bridge
        return resolve_bridge(self)

    # ---- sigma / timestep sampling (common.py:4994-5090) ----
    def sample_flow_sigmas(self, batch: dict, state: dict):
        """common.py:4994-5090: mixflow | custom timestep list (fixed-list / round-robin) | sigmoid-normal (default) | uniform | Beta | the
        "fast" discrete schedule | cubic-spline density (flow_cubic_schedule_weights, training/sigma_density.py)"""
        cfg = self.config
        bsz = batch["latents"].shape[0]
        dev = self.accelerator.device
        shape_ref = batch.get("noise_shape_ref", batch.get("noise", batch["latents"]))
        if getattr(cfg, "mixflow_enabled", False) is True:
            # sigma increases toward noise: the paper's t ~ Beta(2,1) becomes sigma = 1 - sqrt(U) ~ Beta(1,2)   (common.py:5001-5007)
            sigmas = 1.0 - torch.sqrt(torch.rand((bsz,), device=dev))
            sigmas = apply_flow_schedule_shift(cfg, self.noise_schedule, sigmas, shape_ref)
            return sigmas, sigmas * 1000.0
        custom = self._normalize_flow_custom_timesteps(getattr(cfg, "flow_custom_timesteps", None))
        if custom is not None:
            mode = str(getattr(cfg, "flow_timesteps_mode", "fixed-list") or "fixed-list").replace("_", "-")
            if mode not in {"fixed-list", "round-robin"}:
                raise ValueError("flow_timesteps_mode must be either 'fixed-list' or 'round-robin'.")
            if torch.max(custom) <= 1.0:                                   # values <= 1 are sigmas, otherwise timesteps in [0, 1000]
                base_s = custom.clamp(0.0, 1.0); base_t = base_s * 1000.0
            else:
                base_t = custom.clamp(0.0, 1000.0); base_s = (base_t / 1000.0).clamp(0.0, 1.0)
            if base_t.numel() == 1:
                return base_s.expand(bsz), base_t.expand(bsz)
            if mode == "round-robin":
                world = int(getattr(self.accelerator, "num_processes", 1) or 1)
                rank = int(getattr(self.accelerator, "process_index", 0) or 0)
                gather = getattr(self.accelerator, "gather", None)
                if world > 1 and callable(gather):                          # ranks may hold different batch sizes (distributed batch layout)
                    sizes = [int(v) for v in gather(torch.tensor([bsz], device=dev)).reshape(-1).tolist()]
                    global_bsz, offset = sum(sizes), sum(sizes[:rank])
                else:
                    global_bsz, offset = bsz * world, bsz * rank
                if not hasattr(self, "_flow_custom_timestep_cursor"):
                    resume = getattr(self, "_flow_custom_timestep_resume_step", None)
                    done = int(resume if resume is not None else state.get("global_step", 0) or 0)
                    self._flow_custom_timestep_cursor = (done * global_bsz) % base_t.numel()
                    if resume is not None:
                        delattr(self, "_flow_custom_timestep_resume_step")
                cursor = int(self._flow_custom_timestep_cursor)
                idx = (torch.arange(bsz, device=dev) + cursor + offset) % base_t.numel()
                self._flow_custom_timestep_cursor = (cursor + global_bsz) % base_t.numel()
            else:
                idx = torch.randint(0, base_t.numel(), (bsz,), device=dev)
            return base_s[idx], base_t[idx]
        if self._uses_flow_cubic_schedule():                                 # common.py:5058-5061: ahead of every other distribution switch
            sigmas = self._sample_flow_cubic_values(bsz, dev)
            sigmas = apply_flow_schedule_shift(cfg, self.noise_schedule, sigmas, shape_ref)
            return sigmas, sigmas * 1000.0
        if getattr(cfg, "flux_fast_schedule", False) and not (getattr(cfg, "flow_use_beta_schedule", False) or getattr(cfg, "flow_use_uniform_schedule", False)):
            import random
            sigmas = torch.tensor(random.choices([1.0] * 7 + [0.75, 0.5, 0.25], k=bsz), device=dev)      # no schedule shift on this branch
            return sigmas, sigmas * 1000.0
        if getattr(cfg, "flow_use_uniform_schedule", False):
            sigmas = torch.rand((bsz,), device=dev)
        elif getattr(cfg, "flow_use_beta_schedule", False):
            dist = torch.distributions.Beta(cfg.flow_beta_schedule_alpha, cfg.flow_beta_schedule_beta)
            sigmas = dist.sample((bsz,)).to(device=dev)
        else:
            normal = torch.randn((bsz,), device=dev)
            offset = self._get_dataset_timestep_sampling_offset(batch)      # per-dataset bias of the logit-normal mean (common.py:5069-5071)
            if offset:
                normal = normal + offset
            sigmas = torch.sigmoid(getattr(cfg, "flow_sigmoid_scale", 1.0) * normal)
        sigmas = apply_flow_schedule_shift(cfg, self.noise_schedule, sigmas, shape_ref)
        return sigmas, sigmas * 1000.0

    # resolution-dependent shift for schedulers with dynamic shifting (common.py:4730-4797)
    def _get_patch_size_for_dynamic_shift(self, noise_scheduler):
        try:
            comp = self.get_trained_component()
        except Exception:
            comp = None
        for holder in (getattr(comp, "config", None), getattr(noise_scheduler, "config", None), self.config):
            ps = getattr(holder, "patch_size", None) if holder is not None else None
            if ps is not None:
                return ps
        return None

    def calculate_dynamic_shift_mu(self, noise_scheduler, latents):
        """mu(seq_len): the line through (base_image_seq_len, base_shift) and (max_image_seq_len, max_shift); seq_len counts patches (x frames
        for [B,C,F,H,W] latents)"""
        sc = getattr(noise_scheduler, "config", None)
        if latents is None or sc is None:
            return None
        need = ("base_image_seq_len", "max_image_seq_len", "base_shift", "max_shift")
        absent = [f for f in need if getattr(sc, f, None) is None]
        if absent:
            raise ValueError(f"Cannot compute dynamic timestep shift; scheduler is missing config values: {', '.join(absent)}")
        ps = self._get_patch_size_for_dynamic_shift(noise_scheduler)
        if ps is None or ps <= 0:
            raise ValueError("Cannot compute dynamic timestep shift because no valid `patch_size` was found.")
        frames = latents.shape[-3] if latents.ndim == 5 else 1
        seq_len = frames * (int(latents.shape[-2]) // int(ps)) * (int(latents.shape[-1]) // int(ps))
        return calculate_shift(seq_len, sc.base_image_seq_len, sc.max_image_seq_len, sc.base_shift, sc.max_shift)

    # cubic-spline sigma density (common.py:4840-4854)
    def _flow_cubic_schedule_weights(self):
        from .training.sigma_density import parse_cubic_spline_weights
        return parse_cubic_spline_weights(getattr(self.config, "flow_cubic_schedule_weights", None))

    def _uses_flow_cubic_schedule(self) -> bool:
        return self._flow_cubic_schedule_weights() is not None

    def _sample_flow_cubic_values(self, batch_size: int, device) -> torch.Tensor:
        from .training.sigma_density import CubicSplineDistribution
        knots = self._flow_cubic_schedule_weights()
        if knots is None:
            raise ValueError("flow_cubic_schedule_weights must be configured before sampling its distribution.")
        key = (knots, str(device))
        if getattr(self, "_flow_cubic_distribution_cache_key", None) != key:       # the table is built once per (knots, device)
            self._flow_cubic_distribution = CubicSplineDistribution(knots, device=device)
            self._flow_cubic_distribution_cache_key = key
        return self._flow_cubic_distribution.sample((batch_size,))

    def _normalize_flow_custom_timesteps(self, raw):
        """common.py:4799-4838: comma / semicolon separated string, JSON list, or array -> finite 1-D fp32 tensor (None when empty)"""
        import json
        if raw in (None, "", "None"):
            return None
        cand = raw
        if isinstance(cand, str):
            st_ = cand.strip()
            if st_ == "":
                return None
            try:
                cand = json.loads(st_)
            except Exception:
                try:
                    cand = [float(seg.strip()) for seg in st_.replace(";", ",").split(",") if seg.strip()]
                except Exception:
                    return None
        try:
            t = torch.as_tensor(cand, device=self.accelerator.device, dtype=torch.float32).flatten()
        except Exception:
            return None
        t = t[torch.isfinite(t)]
        return t if t.numel() else None

    def reset_flow_custom_timestep_cursor(self, global_step: int = 0) -> None:
        if hasattr(self, "_flow_custom_timestep_cursor"):
            delattr(self, "_flow_custom_timestep_cursor")
        self._flow_custom_timestep_resume_step = int(global_step or 0)

    # round-robin cursor in checkpoints (common.py:4861-4912): one small JSON per rank next to the optimizer state
    def _flow_custom_timestep_state_path(self, ckpt_dir: str) -> str:
        import os
        rank = _process_rank(self.accelerator)
        return os.path.join(ckpt_dir, "flow_custom_timestep_state.json" if rank == 0 else f"flow_custom_timestep_state-{rank}.json")

    def save_flow_custom_timestep_state(self, ckpt_dir: str) -> None:
        import json
        import os
        mode = str(getattr(self.config, "flow_timesteps_mode", "fixed-list") or "fixed-list").replace("_", "-")
        if mode != "round-robin" or self._normalize_flow_custom_timesteps(getattr(self.config, "flow_custom_timesteps", None)) is None:
            return
        state = {"rank": _process_rank(self.accelerator)}
        if hasattr(self, "_flow_custom_timestep_cursor"):
            state["cursor"] = int(self._flow_custom_timestep_cursor)
        elif hasattr(self, "_flow_custom_timestep_resume_step"):
            state["resume_step"] = int(self._flow_custom_timestep_resume_step)
        else:
            return
        os.makedirs(ckpt_dir, exist_ok=True)
        path = self._flow_custom_timestep_state_path(ckpt_dir)
        with open(path + ".tmp", "w", encoding="utf-8") as fh:
            json.dump(state, fh)
        os.replace(path + ".tmp", path)                                     # atomic: a crash never leaves a half-written cursor

    def load_flow_custom_timestep_state(self, ckpt_dir: str, fallback_global_step: int = 0) -> bool:
        import json
        import os
        own = self._flow_custom_timestep_state_path(ckpt_dir)
        shared = os.path.join(ckpt_dir, "flow_custom_timestep_state.json")
        for path in dict.fromkeys((own, shared)):
            if not os.path.exists(path):
                continue
            with open(path, "r", encoding="utf-8") as fh:
                state = json.load(fh)
            if state.get("cursor") is not None:
                self._flow_custom_timestep_cursor = int(state["cursor"])
                if hasattr(self, "_flow_custom_timestep_resume_step"):
                    delattr(self, "_flow_custom_timestep_resume_step")
                return True
            if state.get("resume_step") is not None:
                self.reset_flow_custom_timestep_cursor(int(state["resume_step"]))
                return True
        self.reset_flow_custom_timestep_cursor(fallback_global_step)
        return False

    def _get_dataset_timestep_sampling_offset(self, batch: dict) -> float:
        """common.py:4915-4918: `timestep_sampling_offset` of the dataset the batch came from.  The reference asks its StateTracker; the drop-in
        asks `DATA_BACKEND_CONFIGS` (a plain {backend_id: config} map the data side fills, or a callable `id -> config`)."""
        return float(get_data_backend_config(batch.get("data_backend_id")).get("timestep_sampling_offset", 0.0))

    def _mixflow_gamma(self) -> float:
        gamma = float(getattr(self.config, "mixflow_gamma", 0.8))
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("mixflow_gamma must be between 0.0 and 1.0.")
        return gamma

    def _mixflow_interpolation_sigmas(self, sigmas, slowdown_factors=None):
        """common.py:4966-4977: the INTERPOLATION time is slowed toward noise, the model still sees `sigmas`"""
        sv = sigmas.reshape(sigmas.shape[0], -1)[:, 0]
        gamma = self._mixflow_gamma()
        if gamma == 0.0:
            return sv
        if slowdown_factors is None:
            slowdown_factors = torch.rand_like(sv)
        return sv + slowdown_factors * gamma * (1.0 - sv)

    # ---- prepare_batch (common.py:5862-6041) ----
    def prepare_batch(self, batch: dict, state: dict) -> dict:
        if not batch:
            return batch
        dev, wd = self.accelerator.device, self.config.weight_dtype
        if wd != BF16:
            raise NotImplementedError("the st355 path computes in bf16 (mixed_precision=bf16)")
        if batch.get("prompt_embeds") is not None and hasattr(batch["prompt_embeds"], "to"):
            batch["encoder_hidden_states"] = batch["prompt_embeds"].to(device=dev, dtype=wd)
        pooled = batch.get("add_text_embeds")
        time_ids = batch.get("batch_time_ids")
        batch["added_cond_kwargs"] = {}
        if pooled is not None and hasattr(pooled, "to"):
            batch["added_cond_kwargs"]["text_embeds"] = pooled.to(device=dev, dtype=wd)
        if time_ids is not None and hasattr(time_ids, "to"):
            batch["added_cond_kwargs"]["time_ids"] = time_ids.to(device=dev, dtype=wd)
        latents = batch.get("latent_batch")
        if not hasattr(latents, "to"):
            raise ValueError("Received invalid value for latents.")
        batch["latents"] = latents.to(device=dev, dtype=wd).contiguous()
        mask = batch.get("encoder_attention_mask")
        if mask is not None and hasattr(mask, "to"):
            batch["encoder_attention_mask"] = mask.to(device=dev, dtype=wd)
        perturb = getattr(self.config, "input_perturbation", 0) or 0

        lat = batch["latents"]
        batch["noise_shape_ref"] = lat
        if self.PREDICTION_TYPE is PredictionTypes.FLOW_MATCHING:
            batch["sigmas"], batch["timesteps"] = self.sample_flow_sigmas(batch=batch, state=state)
            sig = batch["sigmas"].to(device=dev, dtype=torch.float32).contiguous()
            if getattr(self.config, "mixflow_enabled", False) is True:          # _prepare_flow_noisy_latents (common.py:4979-4992)
                gamma = self._mixflow_gamma()
                slow = torch.rand_like(sig) if gamma > 0.0 else torch.zeros_like(sig)
                sig = self._mixflow_interpolation_sigmas(sig, slow).contiguous()
                batch["mixflow_slowdown_factors"], batch["mixflow_interpolation_sigmas"] = slow, sig
            given = batch.get("noise")          # tests / parity runs inject the reference's noise; else Philox in-kernel
            seed = int(getattr(self.config, "seed", 42) or 0) + 1_000_003 * int(getattr(self.accelerator, "process_index", 0))
            seed = self.__dict__.get("_eval_noise_seed", seed)          # the evaluation pass's own noise stream (training/evaluation.py sets and removes it)
            per_call = (lat.numel() + 3) // 4
            noisy, target, noise = ops.flow_noise_mix(lat, sig, noise=given, seed=seed, offset=self._noise_offset)
            self._noise_step += 1
            self._noise_offset += per_call          # mixed aspect buckets / varying batch: ranges of different steps never overlap
            input_noise = noise
            steps_ = getattr(self.config, "input_perturbation_steps", None)
            if perturb != 0 and (not steps_ or state.get("global_step", 0) < steps_):
                # common.py:5957-5968 + _prepare_flow_noisy_latents (:4975-4992): the INPUT noise is perturbed — x_t = (1 - sigma) x + sigma (n + p e) — while the target
                # keeps the un-perturbed n - x (get_prediction_target reads batch["noise"], :4610-4611).  The first pass above produced n and the target; the mix is
                # redone with the perturbed noise (an option off by default: one extra streaming pass when it is on)
                p_ = float(perturb) * ((1.0 - state.get("global_step", 0) / steps_) if steps_ else 1.0)
                input_noise = (noise + p_ * torch.randn_like(lat)).to(noise.dtype)
                noisy, _, _ = ops.flow_noise_mix(lat, sig, noise=input_noise)
            batch["noise"] = noise
            batch["input_noise"] = input_noise
            batch["noisy_latents"] = noisy
            batch["flow_target"] = target      # n - x (common.py:4610-4611), consumed by get_prediction_target
            if getattr(self, "self_flow", None) is not None and torch.is_grad_enabled():          # Self-Flow (common.py:5974-5976); evaluation batches stay homogeneous
                self._self_flow_views(batch, state, lat, input_noise, sig)
            else:
                self.expand_sigmas(batch)
                if getattr(self.config, "twinflow_enabled", False) and self.twinflow_value():          # common.py:5979-5980, after the noisy latents exist
                    from .twinflow import prepare_metadata
                    prepare_metadata(batch)
        else:
            # DDPM families (common.py:5983-6002): discrete timesteps (segmented selection when bsz > 1, custom_schedule.py:18-58), noise =
            # randn_like(latents) (or injected), x_t = sqrt(acp_t) x + sqrt(1 - acp_t) n in fp32 then cast (DDPMScheduler.add_noise)
            if self.noise_schedule is None:
                self.setup_training_noise_schedule()
            sched = self.noise_schedule
            bsz = lat.shape[0]
            given_t = batch.get("timesteps")
            if given_t is None:
                given_t = sched.sample_timesteps(bsz, segmented=not getattr(self.config, "disable_segmented_timestep_sampling", False),
                                                 weights=DDPMSchedule.timestep_weights(self.config, sched.config.num_train_timesteps),
                                                 refiner_training=bool(getattr(self.config, "refiner_training", False)),
                                                 refiner_invert_schedule=bool(getattr(self.config, "refiner_training_invert_schedule", False)),
                                                 refiner_strength=float(getattr(self.config, "refiner_training_strength", 0.2)))
            batch["timesteps"] = given_t.to(device=dev).long()
            noise = batch.get("noise")
            if noise is None:
                noise = torch.randn_like(lat)
                if getattr(self.config, "offset_noise", False):                       # common.py:5940-5949 ([B,C,1,1] offset, drawn with a probability)
                    import random
                    prob = float(getattr(self.config, "noise_offset_probability", 1.0))
                    if prob == 1.0 or random.random() < prob:
                        noise = noise + float(getattr(self.config, "noise_offset", 0.1)) * torch.randn(lat.shape[0], lat.shape[1], 1, 1, device=dev, dtype=lat.dtype)
            noise = noise.to(device=dev, dtype=wd)
            input_noise = noise
            steps_ = getattr(self.config, "input_perturbation_steps", None)
            if perturb != 0 and (not steps_ or state.get("global_step", 0) < steps_):     # common.py:5957-5968: perturb the INPUT noise only
                p_ = float(perturb) * ((1.0 - state.get("global_step", 0) / steps_) if steps_ else 1.0)
                input_noise = noise + p_ * torch.randn_like(lat)
            a, b = sched.mix_coefficients(batch["timesteps"])
            noisy, _ = ops.ddpm_noise_mix(lat, input_noise, a, b, want_v=False)
            batch["noise"] = noise
            batch["input_noise"] = input_noise
            batch["noisy_latents"] = noisy
            if self.PREDICTION_TYPE is PredictionTypes.V_PREDICTION:                  # get_velocity uses the un-perturbed noise (common.py:4649-4653)
                batch["velocity_target"] = ops.ddpm_noise_mix(lat, noise, a, b, want_v=True)[1]
            if getattr(self.config, "diff2flow_enabled", False) and self.diff2flow_value() is not None:
                # common.py:5952-5955: noise - latents from the UN-perturbed noise, in the weight dtype, one rounding (the target output of the flow noising pass)
                # (the zero sigmas are held per batch size: no fill launch per step.  The pass still writes a noisy output nobody reads — a target-only mode
                # of the noising kernel is the follow-up)
                zeros = self.__dict__.setdefault("_diff2flow_zero_sigmas", {})
                if (bsz, str(dev)) not in zeros:
                    zeros[(bsz, str(dev))] = torch.zeros(bsz, dtype=torch.float32, device=dev)
                batch["flow_target"] = ops.flow_noise_mix(lat, zeros[(bsz, str(dev))], noise=noise)[1]
        batch.pop("noise_shape_ref", None)
        ss_offset, ss_reflex = self.scheduled_sampling_value()                          # common.py:6013-6037: after the noisy latents exist
        if ss_offset > 0 or ss_reflex:
            self._scheduled_sampling_refuse_tokenwise(batch)
        if ss_offset > 0 and batch.get("scheduled_sampling_plan") is None:              # (tests / parity runs inject a plan, like the noise)
            from .scheduled_sampling import build_rollout_schedule, effective_probability, num_train_timesteps_of
            batch["scheduled_sampling_plan"] = build_rollout_schedule(
                num_train_timesteps=num_train_timesteps_of(self.noise_schedule), batch_size=lat.shape[0], max_step_offset=ss_offset, device=dev,
                base_timesteps=batch["timesteps"], strategy=getattr(self.config, "scheduled_sampling_strategy", "uniform"),
                apply_probability=effective_probability(self.config, state.get("global_step", 0)))
        return self.prepare_batch_conditions(batch=batch, state=state)

    def expand_sigmas(self, batch: dict) -> dict:
        s = batch["sigmas"]
        batch["sigmas"] = s.reshape(s.shape[0], *([1] * (batch["latents"].dim() - 1)))
        return batch

    def prepare_batch_conditions(self, batch: dict, state: dict) -> dict:
        return batch

    # ---- targets / loss (common.py:4635-4658, 6217-6430) ----
    def get_prediction_target(self, prepared_batch: dict):
        if prepared_batch.get("target") is not None:
            return prepared_batch["target"]
        if self.PREDICTION_TYPE is PredictionTypes.FLOW_MATCHING:
            t = prepared_batch.get("flow_target")
            if t is None:
                # (noise - latents), one extra streaming pass only when the fused target was not kept
                _, t, _ = ops.flow_noise_mix(prepared_batch["latents"], torch.zeros(prepared_batch["latents"].shape[0],
                                             device=prepared_batch["latents"].device), noise=prepared_batch["noise"])
            return t
        if self.PREDICTION_TYPE is PredictionTypes.EPSILON:
            return prepared_batch["noise"]
        if self.PREDICTION_TYPE is PredictionTypes.V_PREDICTION:
            return prepared_batch["velocity_target"]        # noise_schedule.get_velocity (common.py:4649-4653), fused into the noising pass
        if self.PREDICTION_TYPE is PredictionTypes.SAMPLE:
            return prepared_batch["latents"]
        raise ValueError(f"Unknown prediction type {self.PREDICTION_TYPE}.")

    def loss(self, prepared_batch: dict, model_output, apply_conditioning_mask: bool = True, _per_sample_only: bool = False, _row_weight=None, _logs=None):
        """common.py:6217-6430.  The two private switches serve XM (xm.py): `_per_sample_only` returns (weighted per-row losses [B] fp32, the row
        weights or None) without touching autograd; `_row_weight` replaces the row weights (it already carries the min-SNR factor)."""
        target = self.get_prediction_target(prepared_batch)
        model_pred = model_output["model_prediction"]
        if target is None:
            raise ValueError("Target is None. Cannot compute loss.")
        if getattr(self.config, "diff2flow_loss", False):                             # common.py:6231-6248: before loss_type / snr_gamma / snr_weight are read
            bridge = self.diff2flow_value()
            if bridge is not None:
                return self._diff2flow_loss(prepared_batch, model_pred, bridge, apply_conditioning_mask, _per_sample_only, _row_weight)
        loss_type = getattr(self.config, "loss_type", "l2")
        if loss_type not in ("l2", "huber", "smooth_l1"):
            raise NotImplementedError(f"Unsupported Loss Type {loss_type}")
        emask = self._conditioning_loss_mask(prepared_batch, model_pred, apply_conditioning_mask)      # common.py:6402-6424
        weight = None
        if self.PREDICTION_TYPE in (PredictionTypes.EPSILON, PredictionTypes.V_PREDICTION):
            gamma = getattr(self.config, "snr_gamma", None)
            if gamma is not None and gamma > 0:                                    # min-SNR weighting (common.py:6363-6397)
                weight = self.noise_schedule.min_snr_weights(prepared_batch["timesteps"], gamma, self.PREDICTION_TYPE is PredictionTypes.V_PREDICTION)
                weight = weight.to(device=model_pred.device, dtype=torch.float32).contiguous()
            elif loss_type == "l2" and float(getattr(self.config, "snr_weight", 1.0)) != 1.0:
                weight = torch.full((model_pred.shape[0],), float(self.config.snr_weight), dtype=torch.float32, device=model_pred.device)
        if _row_weight is not None:
            weight = _row_weight.to(device=model_pred.device, dtype=torch.float32).contiguous()
        huber_c = None
        if loss_type != "l2":
            # huber / smooth_l1 (common.py:6248-6281): one huber_c per sample — constant, or scheduled on the timestep (common.py:6168-6216)
            huber_c = self.compute_scheduled_huber_c(prepared_batch["timesteps"]).to(device=model_pred.device, dtype=torch.float32)
            huber_c = huber_c.reshape(-1).expand(model_pred.shape[0]).contiguous()
        if _per_sample_only:
            with torch.no_grad():
                p_, t_ = model_pred.detach().to(BF16), target.to(BF16)
                per = ops.cond_loss(p_, t_, loss_type, huber_c, weight=weight, want_grad=False, emask=emask)[1]
            return per, weight
        if self.PREDICTION_TYPE is PredictionTypes.FLOW_MATCHING and getattr(self.config, "scheduled_sampling_reflexflow", False):
            self.scheduled_sampling_value()                                            # (the refusals, by the flag's name)
            self._scheduled_sampling_refuse_tokenwise(prepared_batch)
            return self._reflexflow_loss(prepared_batch, model_pred, target, loss_type, huber_c, emask, _logs)
        if loss_type == "l2" and emask is None:
            return _MSELossFn.apply(model_pred, target, weight)
        return _CondLossFn.apply(model_pred, target, loss_type, huber_c, weight, emask)

    def _diff2flow_loss(self, prepared_batch: dict, model_pred, bridge, apply_conditioning_mask: bool, per_sample_only: bool = False, row_weight=None):
        """common.py:6231-6248 + 6402-6429 (xm_mixin.py:175-192 for the two XM passes): the prediction converted to a flow-matching field at the noisy latents and
        the timestep, held to `flow_target` = noise - latents by a plain squared error, then the mask, the per-sample mean and the batch mean — one pass of
        ops.diff2flow_loss, the coefficient pair gathered on the device.  loss_type, snr_gamma and snr_weight are not read on this branch (logged once): the
        base row weight is None."""
        bridge.log_ignored_once(self.config)
        dev = model_pred.device
        tau = prepared_batch.get("flow_target")
        if tau is None:                                                                # get_flow_target (common.py:4660-4666)
            lat = prepared_batch["latents"]
            tau = ops.flow_noise_mix(lat, torch.zeros(lat.shape[0], dtype=torch.float32, device=lat.device), noise=prepared_batch["noise"])[1]
        emask = self._conditioning_loss_mask(prepared_batch, model_pred, apply_conditioning_mask)      # common.py:6402-6424
        noisy = prepared_batch["noisy_latents"].to(device=dev, dtype=BF16)
        tau = tau.to(device=dev, dtype=BF16)
        t = prepared_batch["timesteps"].to(device=dev).long()
        table, mode = bridge.table(self.PREDICTION_TYPE.value), bridge.mode(self.PREDICTION_TYPE.value)
        weight = None if row_weight is None else row_weight.to(device=dev, dtype=torch.float32).contiguous()
        if per_sample_only:
            with torch.no_grad():
                per = ops.diff2flow_loss(model_pred.detach().to(BF16), noisy, tau, t, table, mode, weight=weight, want_grad=False, emask=emask)[1]
            return per, None
        return _Diff2FlowLossFn.apply(model_pred, noisy, tau, t, table, mode, weight, emask)

    def _reflexflow_loss(self, prepared_batch: dict, model_pred, target, loss_type, huber_c, emask, logs=None):
        """common.py:6287-6318 + 6426-6429, the flow-matching branch with `scheduled_sampling_reflexflow` truthy: the exposure weight from the rollout's cached
        predictions (when both exist and alpha != 0), beta2, the mask, the per-sample mean, the ADR term against tau = noisy_latents - latents (post-rollout; present
        with the flag alone, without a plan), the batch mean.  alpha / beta1 / beta2 are read with the reference's `or` idiom: alpha None / 0 -> 0, beta1 None / 0 -> 0,
        beta2 None -> 1.  `logs` (a dict, loss_with_logs passes one): receives the ADR term's batch mean and the mean |exposure weight - 1| as device scalars."""
        cfg = self.config
        beta2 = getattr(cfg, "scheduled_sampling_reflexflow_beta2", 1.0)
        beta2 = 1.0 if beta2 is None else float(beta2)
        alpha = float(getattr(cfg, "scheduled_sampling_reflexflow_alpha", 1.0) or 0.0)
        beta1 = float(getattr(cfg, "scheduled_sampling_reflexflow_beta1", 10.0) or 0.0)
        clean, biased = prepared_batch.get("_reflexflow_clean_pred"), prepared_batch.get("_reflexflow_biased_pred")
        if clean is None or biased is None:
            clean = biased = None
        noisy, latents = prepared_batch.get("noisy_latents"), prepared_batch.get("latents")
        if noisy is None or latents is None:                                           # common.py:6308: the term needs both
            beta1 = 0.0
        loss, adr, stats = _ReflexFlowLossFn.apply(model_pred, target, noisy, latents, clean, biased, loss_type, huber_c, emask, alpha, beta1, beta2)
        if logs is not None:
            logs["reflexflow_adr"] = adr.mean()
            if clean is not None and alpha != 0.0:
                s_e = stats[:, 0]
                logs["reflexflow_weight_deviation"] = (abs(alpha) * s_e / s_e.clamp_min(1e-6)).mean() / float(model_pred.numel() // model_pred.shape[0])
        return loss

    def _conditioning_loss_mask(self, prepared_batch: dict, model_pred, apply_conditioning_mask: bool):
        """common.py:6402-6424: `loss_mask_type` (legacy: `conditioning_type`) "mask" multiplies the elementwise loss by the first channel of
        `conditioning_pixel_values`, area-resized to the latent grid and mapped from [-1,1] to [0,1]; "segmentation" — with probability
        `masked_loss_probability` — by the binarised channel mean.  Returns the fp32 [B, H*W] element mask the fused loss kernel broadcasts over the
        channels, or None.  (The area resize of a one-channel image is input preparation, done with torch like the reference does.)"""
        kind = prepared_batch.get("loss_mask_type")
        if not kind:
            legacy = prepared_batch.get("conditioning_type")
            kind = legacy if legacy in ("mask", "segmentation") else None
        if kind not in ("mask", "segmentation") or not apply_conditioning_mask:
            return None
        if model_pred.dim() != 4:
            raise NotImplementedError("conditioning-mask losses are built for [B,C,H,W] predictions")
        cpv = prepared_batch["conditioning_pixel_values"].to(device=model_pred.device, dtype=torch.float32)
        if kind == "mask":
            m = cpv[:, 0].unsqueeze(1)
        else:
            import random
            if not random.random() < float(getattr(self.config, "masked_loss_probability", 1.0)):
                return None
            m = torch.sum(cpv, dim=1, keepdim=True) / 3
        m = torch.nn.functional.interpolate(m, size=model_pred.shape[2:], mode="area") / 2 + 0.5
        if kind == "segmentation":
            m = (m > 0).to(torch.float32)
        return m.reshape(m.shape[0], -1).contiguous()

    def compute_scheduled_huber_c(self, timesteps: torch.Tensor) -> torch.Tensor:
        """common.py:6168-6216 (flow-matching branch of the "snr" schedule: sigma = ((1 - t/1000) / (t/1000 + 1e-4))^0.5)"""
        import math
        schedule = getattr(self.config, "huber_schedule", "constant")
        base = float(getattr(self.config, "huber_c", 0.1))
        t = timesteps.to(torch.float32)
        if schedule == "constant":
            return torch.full_like(t, base)
        if schedule == "exponential":
            sched_cfg = getattr(getattr(self, "noise_schedule", None), "config", None)          # common.py:6187: self.noise_schedule.config.num_train_timesteps
            alpha = -math.log(base) / float(getattr(sched_cfg, "num_train_timesteps", getattr(self.config, "num_train_timesteps", 1000)))
            return torch.exp(-alpha * t)
        if schedule == "snr":
            if self.PREDICTION_TYPE != PredictionTypes.FLOW_MATCHING:      # DDPM: sigma = sqrt((1 - acp_t) / acp_t) (common.py:6199-6205)
                a = self.noise_schedule.acp_on(timesteps.device)[timesteps.long()].float()
                s_ = ((1.0 - a) / a) ** 0.5
                return (1 - base) / (1 + s_) ** 2 + base
            s = t / 1000
            s = ((1.0 - s) / (s + 0.0001)) ** 0.5
            return (1 - base) / (1 + s) ** 2 + base
        raise NotImplementedError(f"Unknown Huber loss schedule {schedule}")

    def loss_with_logs(self, prepared_batch: dict, model_output, apply_conditioning_mask: bool = True):
        """xm_mixin.py:476-485"""
        k = model_output.get("xm_candidate_count") if isinstance(model_output, dict) else None
        if k:
            return self._xm_noise_loss_with_logs(prepared_batch, model_output, candidate_count=int(k), apply_conditioning_mask=apply_conditioning_mask)
        logs = {}          # (ReflexFlow fills it with device scalars; read here as host floats, like auxiliary_loss's logs)
        loss = self.loss(prepared_batch, model_output, apply_conditioning_mask, _logs=logs)
        return loss, ({k: v.item() for k, v in logs.items()} or None)

    def auxiliary_loss(self, model_output, prepared_batch: dict, loss: torch.Tensor):
        """common.py:5364-5374 `_apply_layersync_regularizer`: loss - lambda * similarity, the two logs as host floats (layersync.py:55-58).  The similarity and its
        gradient come from the engine (model_output["layersync_similarity"]); the `.item()` reads happen here, outside it."""
        logs = {}
        if getattr(self.config, "twinflow_enabled", False) and self.twinflow_value():
            # common.py:6448-6459, ahead of every regulariser (the reference's order): the RCGM base term + the real-velocity term on the training prediction, the
            # teacher's forwards and the two logs' ONE host read inside twinflow.compute_losses
            from .twinflow import compute_losses
            twin, twin_logs = compute_losses(self, prepared_batch, model_output.get("model_prediction") if isinstance(model_output, dict) else None)
            loss = loss + twin
            logs.update(twin_logs)
        ig = getattr(self, "internal_guidance", None)
        if ig is not None:
            # common.py:6461-6469 / internal_guidance.py:229-254, before the LayerSync term (the reference's order): weight * the plugin's own loss() on the head's
            # prediction (model_output["internal_guidance_prediction"], from the engine's tap), the two logs as host floats
            pred = model_output.get("internal_guidance_prediction") if isinstance(model_output, dict) else None
            if pred is None:
                raise ValueError("Internal Guidance is enabled but the model did not return a hidden-state buffer.")
            inter = self.loss(prepared_batch, {"model_prediction": pred}, apply_conditioning_mask=True)
            weighted = inter * ig.weight
            loss = loss + weighted
            logs.update(internal_guidance_loss=weighted.detach().item(), internal_guidance_unweighted_loss=inter.detach().item())
        nl = getattr(self, "nextlat", None)
        if nl is not None:
            # common.py:6471-6475 / nextlat.py:134-156, between the Internal Guidance and LayerSync terms (the reference's order): weight * the state loss the
            # engine's tap left on the device (model_output["nextlat_state_loss"]), the two logs as host floats
            state = model_output.get("nextlat_state_loss") if isinstance(model_output, dict) else None
            if state is None:
                raise ValueError("NextLat is enabled but the model did not return a hidden-state buffer.")
            nl_loss = state * nl.weight
            loss = loss + nl_loss
            logs.update(nextlat_loss=nl_loss.detach().item(), nextlat_state_loss=state.detach().item())
        sf = getattr(self, "self_flow", None)
        if sf is not None and isinstance(model_output, dict) and (model_output.get("crepa_similarity") is not None or torch.is_grad_enabled()):
            # common.py:6850-6881 / crepa.py `compute_loss` (self_flow, image mode: one frame, so the alignment score IS the self similarity): -w * sim with w from
            # the scheduler on this step's similarity — ONE host read; w == 0 (cutoff) adds nothing to the loss and switches the tap's backward off
            sim = model_output.get("crepa_similarity")
            if sim is None:
                raise ValueError("CREPA is enabled but no intermediate hidden states were provided.")
            score = sim.detach().item()
            w = sf.schedule.weight(int(prepared_batch.get("crepa_global_step", 0)), similarity=score)
            if w == 0:
                self.unwrap_model(self.get_trained_component()).self_flow_cutoff()
                logs.update(crepa_loss=0.0, crepa_alignment_score=score, crepa_similarity_self=score, crepa_weight=0.0, crepa_cutoff=True)
            else:
                loss = loss + (-sim * w)
                logs.update(crepa_loss=-score * w, crepa_alignment_score=score, crepa_similarity_self=score, crepa_weight=w, crepa_cutoff=False)
            if sf.schedule.ema is not None:
                logs["crepa_alignment_score_ema"] = sf.schedule.ema
        ls = getattr(self, "layersync", None)
        if ls is not None:
            sim = model_output.get("layersync_similarity") if isinstance(model_output, dict) else None
            if sim is None:
                raise ValueError("LayerSync enabled but no hidden state buffer was provided.")          # layersync.py:33-34: the prediction did not come from a training forward
            ls_loss = -sim * ls.weight
            loss = loss + ls_loss
            logs.update(layersync_loss=ls_loss.detach().item(), layersync_similarity=sim.detach().item())
        return loss, (logs or None)


class _ReflexFlowLossFn(torch.autograd.Function):
    """the ReflexFlow loss (ops.reflexflow_stats + ops.reflexflow_loss), gradient from the same kernel pass; also returns the ADR terms [B] and the stats [B, 4]"""

    @staticmethod
    def forward(ctx, pred, target, noisy, latents, clean, biased, loss_type, huber_c, emask, alpha, beta1, beta2):
        to = lambda t: None if t is None else t.detach().to(BF16)
        p_, n_, l_, c_, b_ = to(pred), to(noisy), to(latents), to(clean), to(biased)
        if n_ is None or l_ is None:                     # (beta1 is 0 then: the kernels still take the operands' places)
            n_ = l_ = p_
        stats = ops.reflexflow_stats(p_, n_, l_, c_, b_)
        loss, _per, adr, dpred = ops.reflexflow_loss(p_, to(target), n_, l_, stats, loss_type, huber_c, clean=c_, biased=b_, alpha=alpha, beta1=beta1, beta2=beta2,
                                                     want_grad=True, emask=emask)
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(adr, stats)
        return loss.reshape(()), adr, stats

    @staticmethod
    def backward(ctx, g, _gadr, _gstats):
        (dpred,) = ctx.saved_tensors
        return ((dpred.float() * g).to(dpred.dtype) if g.numel() == 1 else dpred,) + (None,) * 11


class _Diff2FlowLossFn(torch.autograd.Function):
    """the Diff2Flow loss (ops.diff2flow_loss), gradient from the same kernel pass; the prediction is read in place (PixArt's leading channel half)"""

    @staticmethod
    def forward(ctx, pred, noisy, tau, timesteps, table, mode, weight=None, emask=None):
        loss, _per, dpred = ops.diff2flow_loss(pred.detach().to(BF16), noisy, tau, timesteps, table, mode, weight=weight, want_grad=True, emask=emask)
        ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        # g is the upstream scalar (1.0, or the loss scale); fold it without a host sync
        return ((dpred.float() * g).to(dpred.dtype) if g.numel() == 1 else dpred,) + (None,) * 7


class _CondLossFn(torch.autograd.Function):
    """huber / smooth_l1 (conditional_loss) -> per-sample mean -> batch mean, gradient from the same kernel pass"""

    @staticmethod
    def forward(ctx, pred, target, loss_type, huber_c, weight=None, emask=None):
        loss, _per, dpred = ops.cond_loss(pred.to(BF16), target.to(BF16), loss_type, huber_c, weight=weight, want_grad=True, emask=emask)
        ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred.float() * g).to(dpred.dtype) if g.numel() == 1 else dpred, None, None, None, None, None


class _MSELossFn(torch.autograd.Function):
    """mean_b(mean_chw((pred - target)^2)) in fp32 with the gradient produced by the same kernel pass (K13)."""

    @staticmethod
    def forward(ctx, pred, target, weight=None):
        loss, _per, dpred = ops.mse_loss(pred.to(BF16), target.to(BF16), weight=weight, want_grad=True)
        ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        # g is the upstream scalar (1.0, or the loss scale); fold it without a host sync
        return (dpred.float() * g).to(dpred.dtype) if g.numel() == 1 else dpred, None, None

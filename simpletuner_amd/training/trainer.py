"""Minimal host harness that replays the reference's step order — `Trainer.train()` inner loop,
simpletuner/helpers/training/trainer.py:6951-7568 — around the plugin surface, so the drop-in boundary
can be exercised where SimpleTuner itself cannot be imported.  Where SimpleTuner is installed, its own
Trainer drives the same plugin / optimizer / EMA objects.

    prepare_batch -> model_predict -> loss_with_logs -> auxiliary_loss -> (gather avg loss) -> backward
      -> grad norm / clip -> optimizer.step -> zero_grad -> lr_scheduler.step -> ema.step

Differences from the reference, all on purpose (SURVEY.md §3.3 "per-step host syncs"): no per-step `.item()` — the loss
stays a device scalar and is read back only when logged; no barriers in the step; the 1/world averaging and the clip
coefficient are folded into the optimizer kernel (grad_scale) instead of extra passes over the gradients.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace
from typing import Callable, Iterable, Optional

import torch
import torch.distributed as dist

from .. import ops
from .ema import EMAModel
from .grad_sync import GradSync, sync_module_states
from .multi_process import gather_sample_weighted_scalar
from .optimizer import OPTIMIZER_CHOICE, St355Adafactor, St355AdamW, St355AdamWBF16, St355Lion, St355Muon, St355Soap, flat_view, optimizer_settings


class St355Accelerator:
    """the slice of accelerate.Accelerator the step path touches (device, ranks, backward, sync flags)."""

    def __init__(self, device=None, gradient_accumulation_steps: int = 1):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.gradient_accumulation_steps = gradient_accumulation_steps
        self.sync_gradients = True
        self.is_dist = dist.is_available() and dist.is_initialized()
        self.process_index = dist.get_rank() if self.is_dist else 0
        self.num_processes = dist.get_world_size() if self.is_dist else 1
        self.is_main_process = self.process_index == 0

    def backward(self, loss: torch.Tensor):
        loss.backward()

    def wait_for_everyone(self):
        if self.is_dist:
            dist.barrier()


def default_config(**over) -> SimpleNamespace:
    """the config keys the drop-in honours (SURVEY.md §5 'Config / flags'), with the examples' defaults"""
    cfg = dict(model_family="flux", model_type="lora", lora_rank=32, lora_alpha=None, mixed_precision="bf16",
               weight_dtype=torch.bfloat16, base_weight_dtype=torch.bfloat16, optimizer="st355-adamw", learning_rate=1e-4,
               adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, adam_weight_decay=1e-2, use_ema=False, ema_decay=0.9999,
               ema_update_interval=None, ema_device="accelerator", ema_cpu_only=False, flow_schedule_shift=3.0,
               flow_schedule_auto_shift=False, flow_sigmoid_scale=1.0, flow_use_uniform_schedule=False, flow_use_beta_schedule=False,
               flux_fast_schedule=False, flux_guidance_mode="constant", flux_guidance_value=1.0, flux_attention_masked_training=False,
               flux_lora_target="default", snr_gamma=None, loss_type="l2", max_grad_norm=0.0, grad_clip_method="norm",
               gradient_accumulation_steps=1, train_batch_size=1, gradient_checkpointing=False, input_perturbation=0,
               offset_noise=False, seed=42, lora_init_b_std=0.0, layersync_enabled=False, layersync_student_block=None, layersync_teacher_block=None,
               layersync_lambda=None, internal_guidance_enabled=False, internal_guidance_loss_weight=0.5, internal_guidance_block_index=None,
               validation_internal_guidance_scale=1.0, nextlat_enabled=False, nextlat_weight=None, nextlat_block_index=None, nextlat_state_loss=None,
               nextlat_kl_weight=None, crepa_enabled=False)
    cfg.update(over)
    return SimpleNamespace(**cfg)


def _safe_load(path: str, allow_pickle: bool = False):
    """torch.load with `weights_only=True` plus the numpy allow-list accelerate itself uses for its RNG-state files (accelerate.utils.other.load:
    arrays and dtypes are numbers, not code).  `allow_pickle` (config.allow_unsafe_checkpoint_pickles) is the explicit opt-in for legacy files."""
    if allow_pickle:
        return torch.load(path, map_location="cpu", weights_only=False)
    import numpy as np
    from _codecs import encode
    np_core = getattr(np, "_core", None) or np.core
    allow = [np_core.multiarray._reconstruct, np.ndarray, np.dtype, encode]
    if hasattr(np, "dtypes") and hasattr(np.dtypes, "UInt32DType"):
        allow.append(np.dtypes.UInt32DType)
    with torch.serialization.safe_globals(allow):
        return torch.load(path, map_location="cpu", weights_only=True)


def _diffusers_config(comp) -> dict:
    """a diffusers-style config.json for the trained component: `_class_name` + every JSON-representable field of `comp.config`"""
    import json
    cfg = getattr(comp, "config", None)
    items = dict(vars(cfg)) if cfg is not None and hasattr(cfg, "__dict__") else dict(cfg or {})
    out = {"_class_name": type(comp).__name__, "_diffusers_version": "0.36.0"}
    for k, v in items.items():
        if isinstance(v, tuple):
            v = list(v)
        try:
            json.dumps(v)
        except TypeError:
            continue
        out[k] = v
    return out


class Trainer:
    def __init__(self, config, model_plugin, accelerator: Optional[St355Accelerator] = None, lr_lambda: Optional[Callable] = None, eval_sets=None):
        self.config = config
        self.accelerator = accelerator or model_plugin.accelerator
        self.model = model_plugin
        comp = self.model.get_trained_component()
        # arena order when the component exposes it (fused one-launch optimizer step), else registration order
        self.params = (comp.trainable_parameters() if hasattr(comp, "trainable_parameters")
                       else [p for p in comp.parameters() if p.requires_grad])
        # optimizer_param.py:76-96 registry semantics: name -> class (+ default settings)
        opt_name = getattr(config, "optimizer", "st355-adamw")
        if opt_name not in ("adamw_bf16", "st355-adamw", "torch-adamw", "muon", "optimi-lion", "soap", "torch-adafactor"):   # never a silently different optimizer
            raise NotImplementedError(f"optimizer '{opt_name}' is not built on the st355 path (adamw_bf16, muon, optimi-lion, soap, torch-adafactor, st355-adamw = torch-adamw semantics)")
        if opt_name in ("muon", "soap") and getattr(config, "internal_guidance_enabled", False):
            raise NotImplementedError(f"optimizer '{opt_name}' with internal_guidance_enabled: the trainable arena then holds the head's 1-D tensors, which the "
                                      "matrix optimizers do not take (built: st355-adamw = torch-adamw, adamw_bf16, optimi-lion)")
        if opt_name in ("muon", "soap") and getattr(config, "nextlat_enabled", False):
            raise NotImplementedError(f"optimizer '{opt_name}' with nextlat_enabled: the trainable arena then holds the predictor's 1-D tensors, which the "
                                      "matrix optimizers do not take (built: st355-adamw = torch-adamw, adamw_bf16, optimi-lion)")
        if opt_name in ("muon", "soap") and getattr(config, "crepa_enabled", False):
            raise NotImplementedError(f"optimizer '{opt_name}' with crepa_enabled: the trainable arena then holds the projector's 1-D tensors, which the "
                                      "matrix optimizers do not take (built: st355-adamw = torch-adamw, adamw_bf16, optimi-lion)")
        self._bf16_shadow = None
        if opt_name == "muon":
            if not getattr(self.model, "SUPPORTS_MUON_CLIP", False):                   # trainer.py:332-339
                raise ValueError(f"Optimizer 'muon' is not supported by model family {getattr(config, 'model_family', None)}. "
                                 "Choose a supported optimizer or enable MuonClip explicitly on the model.")
            if getattr(comp, "full", False):
                raise NotImplementedError("optimizer 'muon' is built for LoRA adapters only: a full-rank matrix has a short side up to 3072 (the kernel "
                                          "takes at most 128), and QK-clip would then act on trained q/k weights, which needs per-head max logits "
                                          "from the attention forward")
            if hasattr(self.model, "enable_muon_clip_logging"):
                self.model.enable_muon_clip_logging()
            self.optimizer = St355Muon(self.params, lr=config.learning_rate, **optimizer_settings("muon", config))
        elif opt_name == "soap":
            if getattr(comp, "full", False):
                raise NotImplementedError("optimizer 'soap' is built for LoRA adapters only: a full-rank matrix or a full fine-tune has short sides up to "
                                          "3072 (the kernel preconditions a rank side of at most 128)")
            if getattr(config, "hip_graph", False):
                raise NotImplementedError("optimizer 'soap' cannot run under hip_graph: the eigenbasis refresh changes the launch sequence on some steps")
            self.optimizer = St355Soap(self.params, lr=config.learning_rate, **optimizer_settings("soap", config))
        elif opt_name == "adamw_bf16":
            opt_params = self.params
            if any(p.dtype != torch.bfloat16 for p in self.params):
                opt_params = self._make_bf16_shadow()
            self.optimizer = St355AdamWBF16(opt_params, lr=config.learning_rate, betas=(config.adam_beta1, config.adam_beta2),
                                            eps=OPTIMIZER_CHOICE["adamw_bf16"]["default_settings"]["eps"], weight_decay=config.adam_weight_decay,
                                            seed=int(getattr(config, "seed", 0) or 0))
        elif opt_name == "torch-adafactor":
            # every LoRA arena (2-D fp32) and the transformer full arenas (bf16; 1-D tensors and batched small matrices included).  No fused EMA: EMAModel.step
            # runs after the step.  The UNet full fine-tune is refused: in the reference's layout its convolutions are [Cout, Cin, 3, 3], i.e. 3 x 3 factors on the
            # untuned small-matrix path.  The class-name test is the one that fires for the real component (UNet2DConditionModel keeps a convolution as [Cout, 9 Cin]
            # rows, so its parameters do not show the 3 x 3 shape — and would factor differently from the reference if they were stepped); the shape test
            # catches a component that does expose checkpoint-shaped convolutions
            unet = type(comp).__name__.startswith("UNet") or any(p.dim() == 4 and tuple(p.shape[-2:]) == (3, 3) for p in self.params)
            if getattr(comp, "full", False) and unet:
                raise NotImplementedError("optimizer 'torch-adafactor' is not built for the SDXL / SD 1.5 UNet full fine-tune: the reference factors its "
                                          "[Cout, Cin, 3, 3] convolutions as 3 x 3 matrices, which only the untuned small-matrix path would serve")
            self.optimizer = St355Adafactor(self.params, lr=config.learning_rate, **optimizer_settings("torch-adafactor", config))
        elif opt_name == "optimi-lion":
            # fp32 adapter arena or bf16 full-fine-tune arena (Kahan-compensated there), one launch either way; no override_lr_scheduler in the registry entry
            self.optimizer = St355Lion(self.params, lr=config.learning_rate, **optimizer_settings("optimi-lion", config))
        else:
            self.optimizer = St355AdamW(self.params, lr=config.learning_rate, betas=(config.adam_beta1, config.adam_beta2),
                                        eps=config.adam_epsilon, weight_decay=config.adam_weight_decay)
        self.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lr_lambda) if lr_lambda else None
        if self.lr_scheduler is None and getattr(config, "lr_scheduler", None):             # the reference's named schedules (custom_schedule.py:481-557)
            from .lr_schedule import get_lr_scheduler
            self.lr_scheduler = get_lr_scheduler(config, self.optimizer, self.accelerator, None, 0)
        self.ema_model = None
        if getattr(config, "use_ema", False):
            self.ema_model = EMAModel(config, self.accelerator, self.params, decay=config.ema_decay)
        if hasattr(self.model, "configure_gradient_checkpointing"):
            self.model.configure_gradient_checkpointing()                # trainer.py:3573 / 6792
        # hip_graph: predict + loss + backward of one (shape-keyed) step are captured once into a hipGraph and replayed — the UNet step is
        # ~7000 short launches and otherwise bound by the host's launch rate.  No gradient accumulation, fixed shapes per key.  With N > 1 ranks the
        # gradient exchange runs right AFTER the replay, stream-ordered on the flat gradient buffer (the same code as the boundary step of a gradient
        # accumulation below), unless ST355_GRAPH_CAPTURE_COMM=1 and the backend can be captured (RCCL): then GradSync's collectives — issued on the
        # comm stream behind events of the capture stream — become nodes of the graph and overlap the captured backward like the eager path's do.
        self._use_graph = bool(getattr(config, "hip_graph", False))
        import os as _os
        from .ddp_seam import capture_safe
        self._graph_comm_in_graph = (self._use_graph and self.accelerator.num_processes > 1 and _os.environ.get("ST355_GRAPH_CAPTURE_COMM") == "1"
                                     and capture_safe())
        self._overlapped_sync = config.gradient_accumulation_steps == 1 and (not self._use_graph or self._graph_comm_in_graph
                                                                            or self.accelerator.num_processes == 1)
        if self.accelerator.num_processes > 1:
            sync_module_states(comp)                                     # replicas start from rank 0's weights (DDP construction semantics)
            if self.ema_model is not None:                               # ... and so does every replica's shadow (Self-Flow forwards through it: one teacher on all ranks)
                with torch.no_grad():
                    for s_, p_ in zip(self.ema_model.shadow_params, self.params):
                        s_.copy_(p_.data.to(s_.dtype))
        # ST355_COMM_SINGLE_RANK=1 under an initialised process group of ONE rank: the exchange is set up and issued anyway (GradSync.single_rank_exchange) — how a
        # 1-GPU box runs this step's collectives over RCCL itself; a 1-rank SUM changes nothing, so the step's numbers are those of the plain single-process step
        single_rank = self.accelerator.num_processes == 1 and dist.is_available() and dist.is_initialized() and _os.environ.get("ST355_COMM_SINGLE_RANK", "0") not in ("", "0")
        if (self.accelerator.num_processes > 1 or single_rank) and self._overlapped_sync:
            # replicas: bucketed all-reduce of the flat gradient arena, overlapped with the hand-written backward
            import os
            comm = None
            if os.environ.get("ST355_COMM") == "native":                  # the st355_comm_* C ABI over RCCL instead of torch.distributed's collectives
                from .rccl_comm import St355Comm
                comm = St355Comm.from_process_group()
            if getattr(comp, "full", False) and getattr(comp, "grad_arena", None) is not None:
                comp.grad_sync = GradSync(comp.grad_arena, bucket_bytes=128 << 20, comm=comm)
            elif getattr(comp, "lora_grad_flat", None) is not None:
                comp.grad_sync = GradSync(comp.lora_grad_flat, comm=comm)
        if self._use_graph and config.gradient_accumulation_steps != 1:
            raise NotImplementedError("hip_graph: gradient_accumulation_steps == 1 only")
        if self._use_graph and getattr(getattr(model_plugin, "xm_config", None), "enabled", False):
            raise NotImplementedError("hip_graph: XM noise candidates read their logs on the host every step and cannot be captured")
        tlora = getattr(comp, "lora_tlora", None)
        if tlora is not None and getattr(getattr(model_plugin, "xm_config", None), "enabled", False):
            raise NotImplementedError("lycoris algo=tlora with XM noise candidates: the candidate forwards would need the rank mask of the candidate's own timestep; not "
                                      "built on the st355 path")
        if self._use_graph and getattr(config, "layersync_enabled", False):
            raise NotImplementedError("hip_graph: LayerSync (layersync_enabled) reads its logs on the host every step and cannot be captured")
        if getattr(config, "internal_guidance_enabled", False):
            if self._use_graph:
                raise NotImplementedError("hip_graph: Internal Guidance (internal_guidance_enabled) reads its logs on the host every step and cannot be captured")
            if getattr(getattr(model_plugin, "xm_config", None), "enabled", False):
                raise NotImplementedError("internal_guidance_enabled with XM noise candidates is not built on the st355 path")
        if getattr(config, "nextlat_enabled", False):
            if self._use_graph:
                raise NotImplementedError("hip_graph: NextLat (nextlat_enabled) reads its logs on the host every step and cannot be captured")
            if getattr(getattr(model_plugin, "xm_config", None), "enabled", False):
                raise NotImplementedError("nextlat_enabled with XM noise candidates is not built on the st355 path")
        if getattr(config, "crepa_enabled", False):
            if self._use_graph:
                raise NotImplementedError("hip_graph: Self-Flow (crepa_enabled) reads its similarity on the host every step and cannot be captured")
            self.model.ema_model = self.ema_model          # Self-Flow's teacher: the plugin packs the adapters from the EMA's flat shadow (common.py `_ema_teacher_weights_context`)
        if getattr(config, "twinflow_enabled", False) and hasattr(self.model, "twinflow_value"):
            self.model.twinflow_value()                                  # TwinFlow: the reference's checks, then the refusals by the flag's name
            self.model.ema_model = self.ema_model                        # its teacher: the plugin packs the adapters from the EMA's flat shadow
        if hasattr(self.model, "scheduled_sampling_value"):
            self.model.scheduled_sampling_value()                        # scheduled sampling / ReflexFlow: the default-on rule, and the refusals by the flag's name
        self.distiller = None
        self._self_transcendence = False
        if getattr(config, "distillation_method", None):                 # trainer.py:init_distillation: Self-Transcendence, Flow-DPO, LCM (every other method is refused by name)
            from ..flow_dpo import create_distiller, method_of
            if method_of(config) == "self_transcendence":
                from ..self_transcendence import create_distiller
                self._self_transcendence = True
            elif method_of(config) == "lcm":
                from ..lcm import create_distiller
            self.distiller = create_distiller(self.model)
            if self._self_transcendence:
                self.model.self_transcendence = self.distiller           # the plugin's training forward asks it what the tap is trained to
        self._loop_step = None         # the training loop's own step counter (trainer.py:6876, 6955): what a distiller's pre_training_step is handed
        # evaluation loss (trainer.py:7480-7495): built only when an interval is set and eval_loss_disable is false — otherwise nothing is imported, allocated or launched.
        # `eval_sets`: {name: re-iterable of raw batches}, the seam of the reference's _type="eval" backends
        self.evaluation = None
        self.last_eval_logs = None     # {"loss/val/<name>": float} of the eval that ran after the last step of train(), else None; a logger merges it with last_aux_logs
        self.last_eval_table = None    # {name: {timestep: [one loss per eval batch]}} of the last eval
        self.eval_history = []         # (global_step, logs) of every eval train() ran
        if not getattr(config, "eval_loss_disable", False) and any(getattr(config, f, None) not in (None, "", "None", 0, 0.0, False)
                                                                   for f in ("eval_steps_interval", "eval_epoch_interval")):
            from . import evaluation as _ev
            if _ev.schedule_configured(config):
                _ev.refuse_unbuilt(config, self.model, eval_sets)
                self.evaluation = _ev.Evaluation(config, self.accelerator, eval_sets)
        self._graphs = {}
        self._graph_warm = {}
        self.state = {"global_step": 0, "micro_step": 0}
        # (LoRA dropout: the component's call counter starts where add_lora_adapter(dropout_calls=) put it — 0, the micro-step count of a fresh run; load_state
        # restores it)
        self.last_loss = None          # device scalar, no host sync
        self.last_grad_norm = None
        self.last_grad_absmax = None
        self.last_aux_logs = None      # auxiliary_loss's logs of the last micro-step (LayerSync: layersync_loss / layersync_similarity as floats)

    def _make_bf16_shadow(self):
        """adamw_bf16 over an fp32 adapter arena (LoRA): the reference's example trains bf16 adapter weights with bf16 gradients under AdamWBF16
        (simpletuner/examples/sd3.peft-lora/config.json: optimizer adamw_bf16, mixed_precision bf16; optimizers/adamw_bfloat16/__init__.py:66 asserts bf16).
        The trained values live in a bf16 arena that the optimizer steps (compensated stochastic-rounding update, its `shift` buffer); the engine's fp32
        arena mirrors it exactly (every value is a bf16 number), and the fp32 rank-space gradients are rounded to bf16 once per step — what autograd hands
        a bf16 parameter.  Returns the bf16 parameters the optimizer owns (same order, same shapes)."""
        flat32 = flat_view([p.data for p in self.params])
        if flat32 is None:
            raise NotImplementedError("adamw_bf16 over fp32 trainables needs them as one flat arena (the LoRA adapter arena)")
        n = flat32.numel()
        master = flat32.to(torch.bfloat16)
        flat32.copy_(master)                                  # the engine computes with exactly the values the optimizer holds
        grad16 = torch.zeros(n, dtype=torch.bfloat16, device=flat32.device)
        shadow, off = [], 0
        for p in self.params:
            k = p.numel()
            q = torch.nn.Parameter(master[off:off + k].view_as(p))
            q.grad = grad16[off:off + k].view_as(p)
            shadow.append(q)
            off += k
        self._bf16_shadow = SimpleNamespace(flat32=flat32, master=master, grad16=grad16, params=shadow, n=n)
        return shadow

    def check_pending_loss(self) -> None:
        """The reference raises `RuntimeError("Non-finite training loss detected …")` right after the loss is computed (trainer.py:7102-7110), which
        costs a host sync in the middle of every step.  Here the check is opt-in (`config.check_finite_loss`) and DEFERRED: the loss of step i is
        inspected at the start of step i+1 (or by calling this), when it has long been computed — same exception, same message fields, one step
        late, no stall of the launch queue."""
        pending, self._pending_loss = getattr(self, "_pending_loss", None), None
        if pending is None:
            return
        loss, step, filepaths, backend = pending
        if not bool(torch.isfinite(loss).all()):
            raise RuntimeError(f"Non-finite training loss detected (loss={loss.item()}, data_backend_id={backend}, filepaths={filepaths}, "
                               f"loss_logs={{}}) at optimizer step {step}.")

    def train_step(self, raw_batch: dict) -> torch.Tensor:
        cfg, acc = self.config, self.accelerator
        if getattr(cfg, "check_finite_loss", False):
            self.check_pending_loss()
        comp = self.model.get_trained_component()
        prepared = self.model.prepare_batch(raw_batch, self.state)                       # trainer.py:6964
        self.state["micro_step"] += 1
        boundary = self.state["micro_step"] % cfg.gradient_accumulation_steps == 0       # accelerator.accumulate (:7009)
        acc.sync_gradients = boundary
        sync = getattr(comp, "grad_sync", None)
        if sync is not None:
            sync.enabled = boundary
        if self._use_graph:
            loss = self._graph_forward_backward(prepared)
            self.last_loss = gather_sample_weighted_scalar(loss, prepared["latents"].shape[0], acc)
        elif self._self_transcendence:
            # Self-Transcendence (trainer.py:7000, 6119-6131): pre_training_step with the loop's own counter, the plain step's forward (the projector runs at its
            # block, inside it), the plugin's loss and auxiliary_loss, then the distill loss
            self._loop_step = (self.state["global_step"] if self._loop_step is None else self._loop_step) + 1
            self.distiller.pre_training_step(self.model, self._loop_step)
            pred = self.model.model_predict(prepared)
            loss, loss_logs = self.model.loss_with_logs(prepared, pred)
            self.distiller.prepare_model_output(pred)
            loss, self.last_aux_logs = self.model.auxiliary_loss(pred, prepared, loss)
            loss, distill_logs = self.distiller.compute_distill_loss(prepared, pred, loss)
            self.last_aux_logs = {**(loss_logs or {}), **(self.last_aux_logs or {}), **distill_logs}
            if cfg.gradient_accumulation_steps > 1:
                loss = loss / cfg.gradient_accumulation_steps
            self.last_loss = gather_sample_weighted_scalar(loss, prepared["latents"].shape[0], acc)
            acc.backward(loss)
        elif self.distiller is not None:
            # Flow-DPO (trainer.py:6432-6434, 6109-6132): the distiller's prepare_batch, ONE training forward over the doubled batch (preferred rows, then
            # rejected), the plugin's own loss on the preferred rows, then the distill loss (its reference forward runs inside, adapters off, no grad)
            prepared = self.distiller.prepare_batch(prepared, self.model, self.state)
            pred = self.model.model_predict(self.distiller.policy_batch(prepared))
            loss, self.last_aux_logs = self.distiller.compute_distill_loss(prepared, pred, self.distiller.original_loss(prepared, pred))
            loss, gen_logs = self.distiller.generator_loss_step(prepared, pred, loss)
            self.last_aux_logs.update(gen_logs)
            if cfg.gradient_accumulation_steps > 1:
                loss = loss / cfg.gradient_accumulation_steps
            self.last_loss = gather_sample_weighted_scalar(loss, prepared["latents"].shape[0], acc)
            acc.backward(loss)
        else:
            prepared = self.model.apply_scheduled_sampling_rollout(prepared)             # :6059 (a no-op without a plan)
            pred = self.model.model_predict(prepared)                                    # :7097 -> :6085
            loss, loss_logs = self.model.loss_with_logs(prepared, pred)
            loss, self.last_aux_logs = self.model.auxiliary_loss(pred, prepared, loss)
            if loss_logs and not (isinstance(pred, dict) and pred.get("xm_candidate_count")):      # ReflexFlow's logs, ahead of the regularisers' (XM's candidate logs stay where they were)
                self.last_aux_logs = {**loss_logs, **(self.last_aux_logs or {})}
            if cfg.gradient_accumulation_steps > 1:
                loss = loss / cfg.gradient_accumulation_steps
            self.last_loss = gather_sample_weighted_scalar(loss, prepared["latents"].shape[0], acc)   # :7114 (C2)
            acc.backward(loss)                                                           # :7126
        if getattr(cfg, "check_finite_loss", False):
            self._pending_loss = (loss.detach(), self.state["global_step"], prepared.get("filepaths"), prepared.get("data_backend_id"))
        if not boundary:
            return self.last_loss
        grad_scale = getattr(comp, "grad_scale_from_sync", 1.0) if sync is not None else 1.0
        if acc.num_processes > 1 and not self._overlapped_sync:
            # gradient accumulation: reduce the ACCUMULATED .grad once at the boundary (DDP no_sync semantics, trainer.py:7009)
            gflat = flat_view([p.grad for p in self.params])
            if gflat is None:
                raise RuntimeError("accumulated gradients are not one flat arena")
            dist.all_reduce(gflat, op=dist.ReduceOp.SUM)
            grad_scale = 1.0 / acc.num_processes
        if getattr(cfg, "max_grad_norm", 0) and cfg.max_grad_norm > 0:                   # :7138-7217
            # the flat view is built from the gradients autograd actually holds: with gradient accumulation AccumulateGrad adds later micro-steps IN
            # PLACE into the first micro-step's buffer, so `p.grad` (not the component's last backward buffer) is what gets clipped, reduced and stepped
            gflat = flat_view([p.grad for p in self.params])
            if gflat is None:
                raise NotImplementedError("gradient clipping needs the trainable gradients as one flat arena (every parameter with a gradient, back to back)")
            method = getattr(cfg, "grad_clip_method", "norm")
            if method == "value":                                                        # accelerator.clip_grad_value_ (:7209-7213)
                ops.grad_clamp_(gflat, cfg.max_grad_norm / grad_scale)                   # gradients are rank SUMS here; 1/world lives in grad_scale
            elif method == "norm":
                stats = ops.grad_norm(gflat)
                self.last_grad_norm = stats[0].sqrt() * grad_scale                       # device scalars, read only when logged
                self.last_grad_absmax = stats[1] * grad_scale          # `_max_grad_value` (trainer.py:6376-6407): same pass
                ops.grad_clip_norm_(gflat, stats, cfg.max_grad_norm, pre_scale=grad_scale)   # coefficient computed and applied on the device: no host sync
            else:
                raise ValueError(f"Unknown grad clip method: {method}. Supported methods: value, norm")
        self.optimizer.grad_scale = grad_scale
        ema_fused = False
        sh = self._bf16_shadow
        if sh is not None:                                                               # adamw_bf16 over the fp32 adapter arena: bf16 gradients in, bf16 weights out
            gflat = flat_view([p.grad for p in self.params])
            if gflat is None:
                raise RuntimeError("adamw_bf16 (LoRA): the adapter gradients are not one flat arena")
            sh.grad16.copy_(gflat)
            if any(q.grad is None for q in sh.params):      # (a zero_grad(set_to_none=True) by the caller must not detach the optimizer's parameters from their gradient arena)
                off = 0
                for q in sh.params:
                    q.grad = sh.grad16[off:off + q.numel()].view_as(q)
                    off += q.numel()
            self.optimizer.step()
            sh.flat32.copy_(sh.master)
            if not self._use_graph:
                for p in self.params:
                    p.grad = None
        else:
            # EMA fused into the optimizer's launch (north star: "fused AdamW, EMA update"): the decay of ema_model.step(params, global_step + 1) depends on the
            # step count alone (ema.py:322-349), so it is known here; the kernel applies s -= (1 - d)(s - p_new) to the element it just updated — the same
            # arithmetic as the separate pass (ema.py:393-433), minus its 3 x 2 B/param of HBM traffic and one launch
            ema_decay = None
            if self.ema_model is not None and getattr(self.optimizer, "fuses_ema", False):
                ema_decay = self.ema_model.fused_decay(self.params, self.state["global_step"] + 1)
            if ema_decay is not None:
                self.optimizer.ema_shadow_flat, self.optimizer.ema_decay, self.optimizer.ema_applied = self.ema_model.shadow_flat, float(ema_decay), False
            self.optimizer.step()                                                        # :7239
            if ema_decay is not None:
                self.optimizer.ema_shadow_flat = None
                ema_fused = bool(self.optimizer.ema_applied)
            if not self._use_graph:                                                      # graph mode: the captured backward re-writes the same .grad tensors
                self.optimizer.zero_grad(set_to_none=True)                               # :7253
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()                                                     # :7293
        self.state["global_step"] += 1
        if self.ema_model is not None:
            if ema_fused:
                self.ema_model.commit_fused(self.state["global_step"], ema_decay)
            else:
                self.ema_model.step(self.params, self.state["global_step"])              # :7352
        return self.last_loss

    # ------------------------------------------------------------------------------------------------
    def _eager_forward_backward(self, prepared):
        pred = self.model.model_predict(prepared)
        loss, _ = self.model.loss_with_logs(prepared, pred)
        loss, _ = self.model.auxiliary_loss(pred, prepared, loss)
        self.accelerator.backward(loss)
        return loss

    def release_graphs(self) -> None:
        """drop every captured step and the shared capture pool (their activations go back to the allocator): before eager steps that need the memory"""
        import gc
        self._graphs.clear()
        self._graph_pool = None
        gc.collect()
        torch.cuda.empty_cache()

    def _graph_forward_backward(self, prepared):
        def tensors(d, prefix=""):
            for k, v in d.items():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    yield prefix + k, v
                elif isinstance(v, dict):
                    yield from tensors(v, prefix + k + "/")

        def clone_tree(d):
            return {k: (v.clone() if isinstance(v, torch.Tensor) and v.is_cuda else clone_tree(v) if isinstance(v, dict) else v) for k, v in d.items()}

        def shallow(d):          # plugins may replace entries of the batch dict (Flux divides `timesteps` by 1000): never let that touch `static`
            return {k: (shallow(v) if isinstance(v, dict) else v) for k, v in d.items()}

        key = tuple((k, tuple(v.shape), v.dtype) for k, v in tensors(prepared))
        entry = self._graphs.get(key)
        if entry is None:
            # warm-up ON A SIDE STREAM (workspaces, kernel attributes, allocator pools, and AccumulateGrad nodes bound to the capture-side stream:
            # a node created on the default stream and kept alive breaks capture), then capture one step
            static = clone_tree(prepared)
            static_inputs = dict(tensors(static))          # name -> the tensors the captured kernels read; filled from each step's batch
            self.last_loss = None
            # ONE side stream for every capture: the caching allocator keys its free blocks by stream, so a fresh stream per bucket shape made every capture take a
            # new ~40 GB of the shared pool instead of the blocks the previous capture had freed (r6 probe: reserved +25 GiB per bucket at batch 4, allocated flat)
            if getattr(self, "_graph_stream", None) is None:
                self._graph_stream = torch.cuda.Stream()
            side = self._graph_stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    for p in self.params:
                        p.grad = None
                    loss = self._eager_forward_backward(shallow(static))
                    del loss
            torch.cuda.current_stream().wait_stream(side)
            for p in self.params:
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()               # the eager warm-up's cached blocks go back before the capture builds its own pool
            if os.environ.get("ST355_GRAPH_MEM_DEBUG"):
                print(f"[graph] before capture: allocated {torch.cuda.memory_allocated() / 2**30:.1f} GiB, reserved {torch.cuda.memory_reserved() / 2**30:.1f} GiB, "
                      f"peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", file=sys.stderr)
            g = torch.cuda.CUDAGraph()
            # one memory pool for every captured shape (mixed aspect buckets: one graph per bucket): the graphs never run concurrently, so the activations of
            # one capture are the next capture's free blocks — five private ~40 GB pools did not fit next to the model (r5), one shared pool does
            if getattr(self, "_graph_pool", None) is None:
                self._graph_pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(g, pool=self._graph_pool, stream=side):      # the SAME stream as the warm-up: the parameters' AccumulateGrad nodes are bound to it
                loss = self._eager_forward_backward(shallow(static))
            entry = self._graphs[key] = (g, static_inputs, loss.detach(), [p.grad for p in self.params])
        g, st, loss, grads = entry
        for k, v in tensors(prepared):
            st[k].copy_(v)
        g.replay()
        for p, gr in zip(self.params, grads):
            p.grad = gr
        return loss.clone()        # the static tensor is overwritten by the next replay: callers keep their own value

    # ---- checkpoints: the files of the reference's save hooks + accelerate.save_state, in one directory (save_hooks.py:368-443, 850-1305) ----
    def save_state(self, checkpoint_dir: str) -> None:
        """`<dir>/optimizer.bin`, `scheduler.bin`, `random_states_<rank>.pkl` (accelerate's names and pickled keys), the trained weights
        (`pytorch_lora_weights.safetensors` for adapters, `<subfolder>/diffusion_pytorch_model.safetensors` for a full fine-tune),
        `<subfolder>_ema/ema_model.pt`, `training_state.json` (StateTracker.save_training_state keys) and the round-robin timestep cursor.
        Rank 0 writes the shared files; every rank writes its own RNG / cursor files."""
        import json
        import os
        import random

        import numpy as np
        acc, plug = self.accelerator, self.model
        rank = int(getattr(acc, "process_index", 0) or 0)
        os.makedirs(checkpoint_dir, exist_ok=True)
        rng = {"random_state": random.getstate(), "numpy_random_seed": np.random.get_state(), "torch_manual_seed": torch.get_rng_state(),
               "torch_cuda_manual_seed": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None,
               "st355_noise_step": int(getattr(plug, "_noise_step", 0)),
               "st355_noise_offset": int(getattr(plug, "_noise_offset", 0))}    # the in-kernel Philox counter position of the noising pass (cumulative, shape-independent)
        torch.save(rng, os.path.join(checkpoint_dir, f"random_states_{rank}.pkl"))     # accelerate's save_accelerator_state: torch.save under the .pkl name
        plug.save_flow_custom_timestep_state(checkpoint_dir)
        ts = {"global_step": self.state["global_step"], "epoch_step": self.state.get("epoch_step", 0), "epoch": self.state.get("epoch", 1),
              "exhausted_backends": list(self.state.get("exhausted_backends", [])), "repeats": dict(self.state.get("repeats", {})),
              "micro_step": self.state["micro_step"]}
        drop = getattr(plug.get_trained_component(), "lora_dropout", None)
        if drop is not None:                      # LoRA dropout: the mask sequence's position (the device-resident call counter), with the step counters
            ts["lora_dropout_calls"] = drop.calls()
        tlora = getattr(plug.get_trained_component(), "lora_tlora", None)
        if tlora is not None:                     # T-LoRA: the three mask settings, so that a resumed run can hold its config against them
            ts["tlora"] = {"min_rank": tlora.Rmin, "alpha": tlora.alpha, "num_train_timesteps": tlora.T}
        if rank != 0:                                                                   # save_hooks.py:369-373: non-zero ranks write their own state file
            with open(os.path.join(checkpoint_dir, f"training_state-rank{rank}.json"), "w") as fh:
                json.dump(ts, fh)
        if rank != 0:
            return
        host = lambda sd: {"state": {k: {n: (v.detach().to("cpu") if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()},
                           "param_groups": sd["param_groups"]}
        torch.save(host(self.optimizer.state_dict()), os.path.join(checkpoint_dir, "optimizer.bin"))
        if self.lr_scheduler is not None:
            torch.save(self.lr_scheduler.state_dict(), os.path.join(checkpoint_dir, "scheduler.bin"))
        comp = plug.get_trained_component()
        if getattr(comp, "full", False) and hasattr(comp, "diffusers_state_dict"):
            from safetensors.torch import save_file
            sub = os.path.join(checkpoint_dir, plug.MODEL_SUBFOLDER)
            os.makedirs(sub, exist_ok=True)
            save_file({k: v.detach().to("cpu").contiguous() for k, v in comp.diffusers_state_dict().items()},
                      os.path.join(sub, "diffusion_pytorch_model.safetensors"), metadata={"format": "pt"})
            # `unwrapped_model.save_pretrained` (save_hooks.py:1128) also writes config.json: without it neither diffusers' from_pretrained nor the
            # reference's resume path can open the folder
            with open(os.path.join(sub, "config.json"), "w") as fh:
                json.dump(_diffusers_config(comp), fh, indent=2, sort_keys=True)
        else:
            plug.save_lora_weights(checkpoint_dir)
        if self.ema_model is not None:
            self.ema_model.save_state_dict(os.path.join(checkpoint_dir, f"{plug.MODEL_SUBFOLDER}_ema", "ema_model.pt"))
        with open(os.path.join(checkpoint_dir, "training_state.json"), "w") as fh:
            json.dump(ts, fh)

    def load_state(self, checkpoint_dir: str) -> None:
        """the inverse of save_state; a missing per-rank RNG file falls back to rank 0's (resuming on more GPUs than the run was saved with)"""
        import json
        import os
        import random

        import numpy as np
        acc, plug = self.accelerator, self.model
        rank = int(getattr(acc, "process_index", 0) or 0)
        comp = plug.get_trained_component()
        full_path = os.path.join(checkpoint_dir, plug.MODEL_SUBFOLDER, "diffusion_pytorch_model.safetensors")
        if getattr(comp, "full", False) and os.path.exists(full_path):
            from safetensors.torch import load_file
            comp.load_diffusers_state(load_file(full_path))
        else:
            plug.load_lora_weights(input_dir=checkpoint_dir)
            sh = self._bf16_shadow
            if sh is not None:                    # adamw_bf16 over the adapter arena: the optimizer's bf16 values follow the loaded weights (the saved adapters ARE bf16 numbers
                sh.master.copy_(sh.flat32)        # when this trainer wrote them; a foreign file is rounded once, as at construction), and the engine's arena mirrors them
                sh.flat32.copy_(sh.master)
        unsafe = bool(getattr(self.config, "allow_unsafe_checkpoint_pickles", False))     # explicit opt-in only: the default never executes a pickle
        self.optimizer.load_state_dict(_safe_load(os.path.join(checkpoint_dir, "optimizer.bin"), unsafe))
        sched = os.path.join(checkpoint_dir, "scheduler.bin")
        if self.lr_scheduler is not None and os.path.exists(sched):
            self.lr_scheduler.load_state_dict(_safe_load(sched, unsafe))
        if self.ema_model is not None:
            self.ema_model.load_state_dict(os.path.join(checkpoint_dir, f"{plug.MODEL_SUBFOLDER}_ema", "ema_model.pt"))
        ts_path = os.path.join(checkpoint_dir, "training_state.json" if rank == 0 else f"training_state-rank{rank}.json")
        if not os.path.exists(ts_path):                                                  # save_hooks.py:1276-1279: fall back to the default name
            ts_path = os.path.join(checkpoint_dir, "training_state.json")
        with open(ts_path) as fh:
            ts = json.load(fh)
        self.state.update({k: ts[k] for k in ("global_step", "epoch_step", "epoch", "exhausted_backends", "repeats") if k in ts})
        self.state["micro_step"] = int(ts.get("micro_step", self.state["global_step"] * self.config.gradient_accumulation_steps))
        self._loop_step = None                    # (the loop's own counter restarts from the loaded global step, trainer.py:6876)
        tlora = getattr(comp, "lora_tlora", None)
        if tlora is not None and "tlora" in ts:   # T-LoRA: a resumed run trains under the mask the checkpoint was trained under
            own = {"min_rank": tlora.Rmin, "alpha": tlora.alpha, "num_train_timesteps": tlora.T}
            diff = [f"{k}: checkpoint {ts['tlora'].get(k)}, configured {v}" for k, v in own.items() if ts["tlora"].get(k) != v]
            if diff:
                raise ValueError("the checkpoint was trained under other T-LoRA mask settings (" + "; ".join(diff) + "): set tlora_min_rank / tlora_alpha in the "
                                 "lycoris_config (and the noise schedule's num_train_timesteps) to the checkpoint's values")
        drop = getattr(comp, "lora_dropout", None)
        if drop is not None:                      # a resumed run continues the mask sequence (a state file from before the counter: the micro-step count)
            drop.set_calls(int(ts.get("lora_dropout_calls", self.state["micro_step"])))
        plug.load_flow_custom_timestep_state(checkpoint_dir, fallback_global_step=self.state["global_step"])
        for name in (f"random_states_{rank}.pkl", "random_states_0.pkl"):
            path = os.path.join(checkpoint_dir, name)
            if not os.path.exists(path):
                continue
            rng = _safe_load(path, unsafe)
            random.setstate(rng["random_state"])
            np.random.set_state(rng["numpy_random_seed"])
            torch.set_rng_state(rng["torch_manual_seed"])
            if rng.get("torch_cuda_manual_seed") is not None and torch.cuda.is_available():
                torch.cuda.set_rng_state_all(rng["torch_cuda_manual_seed"])
            plug._noise_step = int(rng.get("st355_noise_step", 0))
            plug._noise_offset = int(rng.get("st355_noise_offset", 0))
            break

    def evaluate(self) -> dict:
        """One evaluation-loss pass over the eval sets with the training weights (the reference swaps in no EMA copy): {"loss/val/<name>": mean over all (timestep,
        batch) entries}; `last_eval_table` keeps the per-dataset, per-timestep losses.  Ranks other than the main one return {} and issue no collective.  Training's
        random streams, noise counters and round-robin cursor are where they were afterwards."""
        if self.evaluation is None or not self.accelerator.is_main_process:
            return {}
        table = self.evaluation.execute_eval(self.model, self.evaluation.noise_scheduler_of(self.model))
        self.last_eval_table = table
        self.last_eval_logs = self.evaluation.generate_tracker_table(table) if table else {}
        return self.last_eval_logs

    def train(self, batches: Iterable[dict], max_steps: int):
        losses = []
        for i, b in enumerate(batches):
            if i >= max_steps:
                break
            losses.append(self.train_step(b))
            if self.evaluation is not None:                                              # trainer.py:7480-7495: after the step
                self.last_eval_logs = None
                if self.evaluation.would_evaluate(self.state):
                    self.eval_history.append((self.state["global_step"], self.evaluate()))
        return losses

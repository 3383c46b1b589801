"""Self-Flow: the reference's CREPA regulariser with `crepa_feature_source=self_flow` (documentation/experimental/SELF_FLOW.md; helpers/training/crepa.py,
helpers/models/common.py `_validate_crepa_configuration`), the plugin side.  Imported only when `crepa_enabled` is set.

  * `feature_source(config)`: the configured teacher source — "encoder", "backbone" or "self_flow" — from `crepa_feature_source` (aliases external / internal /
    selfflow) and the legacy flags `crepa_use_backbone_features` / `crepa_self_flow`, with the reference's conflict errors.
  * `validate(config, name, supported)`: the self_flow checks in the reference's order and with its texts.
  * `WeightSchedule`: crepa.py's `CrepaScheduler` restated — the coefficient per step (linear warm-up, constant / linear / cosine / polynomial decay towards
    `crepa_lambda_end`), the step cutoff, the similarity-EMA threshold and the permanent / recoverable modes.  Its state (the EMA, the trigger) is NOT persisted:
    the reference does not persist it either, so a resumed run starts it afresh.
  * `mask_ratio(config)`: `crepa_self_flow_mask_ratio` as the batch preparation reads it (default 0.1, None / 0 -> 0).
"""
from __future__ import annotations

import math
from typing import Optional

SOURCES = ("encoder", "backbone", "self_flow")          # the reference's enum values, in its order (the "Expected one of" text)
_ALIASES = {"encoder": "encoder", "external": "encoder", "backbone": "backbone", "internal": "backbone", "self_flow": "self_flow", "selfflow": "self_flow"}


def feature_source(config) -> str:
    raw = getattr(config, "crepa_feature_source", None)
    backbone, self_flow = bool(getattr(config, "crepa_use_backbone_features", False)), bool(getattr(config, "crepa_self_flow", False))
    src = None
    if raw is not None:
        src = _ALIASES.get(str(raw).strip().lower())
        if src is None:
            raise ValueError(f"Unsupported crepa_feature_source={raw!r}. Expected one of: {', '.join(SOURCES)}.")
    if backbone and self_flow:
        raise ValueError("crepa_use_backbone_features and crepa_self_flow cannot both be enabled.")
    if src is not None and backbone and src != "backbone":
        raise ValueError("crepa_use_backbone_features conflicts with crepa_feature_source. Set crepa_feature_source=backbone or disable the legacy flag.")
    if src is not None and self_flow and src != "self_flow":
        raise ValueError("crepa_self_flow conflicts with crepa_feature_source. Set crepa_feature_source=self_flow or disable the legacy flag.")
    if src is not None:
        return src
    return "self_flow" if self_flow else "backbone" if backbone else "encoder"


def mask_ratio(config) -> float:
    return float(getattr(config, "crepa_self_flow_mask_ratio", 0.1) or 0.0)


def validate(config, name: str, supported: bool) -> str:
    """-> the feature source; for self_flow the reference's checks, in its order"""
    src = feature_source(config)
    if src == "self_flow":
        if not supported:
            raise ValueError(f"CREPA self_flow mode is not implemented for {name}.")
        if not getattr(config, "use_ema", False):
            raise ValueError("CREPA self_flow mode requires an EMA teacher; enable use_ema.")
        if getattr(config, "crepa_teacher_block_index", None) is None:
            raise ValueError("CREPA self_flow mode requires crepa_teacher_block_index to be set.")
        if not 0.0 <= mask_ratio(config) <= 0.5:
            raise ValueError("CREPA self_flow mode requires crepa_self_flow_mask_ratio to be within [0.0, 0.5].")
        if getattr(config, "twinflow_enabled", False):
            raise ValueError("CREPA self_flow mode is not yet compatible with TwinFlow.")
    return src


class WeightSchedule:
    KINDS = ("constant", "linear", "cosine", "polynomial")

    def __init__(self, config, max_train_steps: int):
        g = lambda k, d=None: getattr(config, k, d)
        self.kind = str(g("crepa_scheduler", "constant") or "constant").lower()
        self.base = float(g("crepa_lambda", 0.5) or 0.0)
        self.warmup = int(g("crepa_warmup_steps", 0) or 0)
        decay = int(g("crepa_decay_steps", 0) or 0)
        self.decay = decay if decay > 0 else max_train_steps
        self.end = float(g("crepa_lambda_end", 0.0) or 0.0)
        self.cutoff_step = int(g("crepa_cutoff_step", 0) or 0)
        thr = g("crepa_similarity_threshold")
        self.threshold = None if thr is None else float(thr)
        d = g("crepa_similarity_ema_decay")
        self.ema_decay = 0.99 if d is None else float(d)
        self.mode = str(g("crepa_threshold_mode", "permanent") or "permanent").lower()
        self.power = float(g("crepa_power", 1.0) or 1.0)
        self.ema: Optional[float] = None
        self.triggered = False

    def scheduled(self, step: int) -> float:
        """the coefficient at `step` without the cutoff"""
        if self.warmup > 0 and step < self.warmup:
            return self.base * (step / self.warmup)
        if self.kind not in ("linear", "cosine", "polynomial"):
            return self.base
        progress = min((step - self.warmup) / max(self.decay - self.warmup, 1), 1.0)
        if self.kind == "linear":
            return self.base + (self.end - self.base) * progress
        if self.kind == "cosine":
            return self.end + (self.base - self.end) * (1 + math.cos(math.pi * progress)) / 2
        return (self.base - self.end) * ((1 - progress) ** self.power) + self.end

    def weight(self, step: int, similarity: Optional[float] = None) -> float:
        """the coefficient of this step; `similarity` first enters the EMA the threshold is tested on"""
        if similarity is not None:
            self.ema = similarity if self.ema is None else self.ema_decay * self.ema + (1 - self.ema_decay) * similarity
        if self.triggered and self.mode == "permanent":
            return 0.0
        if (self.cutoff_step > 0 and step >= self.cutoff_step) or (self.threshold is not None and self.ema is not None and self.ema >= self.threshold):
            if self.mode == "permanent":
                self.triggered = True
            return 0.0
        if self.mode == "recoverable":
            self.triggered = False
        return self.scheduled(step)

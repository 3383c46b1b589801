"""Tensor-level wrappers over the C ABI (include/st355.h).

torch is used here only as the owner of device memory and of the HIP stream: every wrapper validates
shapes/dtypes, allocates the outputs, and passes raw device pointers + the current stream to libst355.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import lib as _l
from .lib import EPI_ADD, EPI_GATE_RESIDUAL, EPI_GEGLU, EPI_GEGLU_GRAD, EPI_GELU, EPI_HEADS, EPI_MUL_GELU_GRAD, EPI_NONE, EPI_QK_NORM_ROPE, GemmArgs, Heads, QkRope  # noqa: F401

BF16 = torch.bfloat16
F32 = torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _l.St355Error(f"{name}: expected a device tensor (the train step has no CPU path)")
    if t.dtype != dtype:
        raise _l.St355Error(f"{name}: expected dtype {dtype}, got {t.dtype}")


def _dev(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise _l.St355Error(f"{name}: expected a device tensor (the train step has no CPU path)")


def _rows(t: torch.Tensor, name: str) -> int:
    """leading dimension (elements) of a 2-D row-major view"""
    if t.dim() != 2 or t.stride(1) != 1:
        raise _l.St355Error(f"{name}: expected a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.stride(0)


def _seg(t: torch.Tensor, name: str):
    """A GEMM / skinny operand is either a 2-D row-major view or a 3-D view [segments, rows, cols] with unit inner stride whose segment stride is a
    whole number of rows: the per-sample row blocks of a joint [B, S, *] buffer, e.g. `qkv.view(B, S, 3 * D)[:, St:]` (st355_gemm_args.seg_rows).
    Returns (rows_total, cols, ld, seg_rows, seg_stride_rows); seg_rows = 0 for a plain 2-D operand."""
    if t.dim() == 2:
        return t.shape[0], t.shape[1], _rows(t, name), 0, 0
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) <= 0 or t.stride(0) % t.stride(1) != 0:
        raise _l.St355Error(f"{name}: expected a 2-D row-major view or a 3-D [segments, rows, cols] view whose segment stride is a whole number of rows, "
                            f"got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0] * t.shape[1], t.shape[2], t.stride(1), t.shape[1], t.stride(0) // t.stride(1)


def _seg_join(cur: int, new: int, name: str) -> int:
    if new and cur and new != cur:
        raise _l.St355Error(f"{name}: segmented operands of one problem must share seg_rows ({new} vs {cur})")
    return cur or new


# ------------------------------------------------------------------------------------------------
# device scratch
# ------------------------------------------------------------------------------------------------
# One scratch per (name, device), not per (device, stream) as grad_norm's (its key= is the stream): no caller issues skinny products, or any other scratch user
# but grad_norm, on two streams at once.  LoraGroup.grads and the block megakernels run on the training stream; the trainer's graph warm-up / capture stream is
# joined with wait_stream before and after, so the two never overlap; grad_sync's comm stream runs collectives only.  A caller that does overlap them must bring
# its own workspace through the C ABI.
_scratch_bufs = {}
_scratch_retired = []       # outgrown scratch buffers stay alive: a captured hipGraph may still hold their addresses


def _scratch(name: str, dev, nbytes: int, key=()):
    """caller-owned device scratch of at least nbytes bytes (uint8; the kernels only receive the pointer); libst355 never allocates.  Grow-only; an outgrown
    buffer is retired, never freed (a hipGraph captured earlier keeps its address), and growing DURING a capture is refused (the capture would bake in a pointer
    of its private pool).  A first allocation is allowed inside a capture."""
    k = (name, dev.type, dev.index) + key
    ws = _scratch_bufs.get(k)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            if torch.cuda.is_current_stream_capturing():
                raise _l.St355Error(f"the {name} scratch would have to grow ({ws.numel()} -> {nbytes} bytes) inside a hipGraph capture: run one eager step first")
            _scratch_retired.append(ws)
        ws = _scratch_bufs[k] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


# ------------------------------------------------------------------------------------------------
# streaming ops
# ------------------------------------------------------------------------------------------------
def flow_noise_mix(x, sigma, noise=None, seed: int = 0, offset: int = 0, want_target: bool = True):
    """x_t = (1-σ)x + σn ; target = n - x   (common.py:4975-4992, 4610-4611).  Returns (x_t, target, noise)."""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(sigma, F32, "sigma")
    x = x.contiguous()
    B = x.shape[0]
    per = x.numel() // B
    x_t = torch.empty_like(x)
    target = torch.empty_like(x) if want_target else None
    if noise is not None:
        _chk(noise, BF16, "noise")
        noise = noise.contiguous()
        noise_out = None
    else:
        noise_out = torch.empty_like(x)
    _l.check(L.st355_flow_noise_mix(_stream(), _ptr(x), _ptr(noise), _ptr(sigma), _ptr(x_t), _ptr(target), _ptr(noise_out),
                                    B, per, seed, offset), "flow_noise_mix")
    return x_t, target, (noise if noise is not None else noise_out)


def ddpm_noise_mix(x, noise, sqrt_acp, sqrt_1macp, want_v: bool = True):
    L = _l.load()
    _chk(x, BF16, "x"); _chk(noise, BF16, "noise"); _chk(sqrt_acp, F32, "sqrt_acp"); _chk(sqrt_1macp, F32, "sqrt_1macp")
    x = x.contiguous(); noise = noise.contiguous()
    B = x.shape[0]
    x_t = torch.empty_like(x)
    v = torch.empty_like(x) if want_v else None
    _l.check(L.st355_ddpm_noise_mix(_stream(), _ptr(x), _ptr(noise), _ptr(sqrt_acp), _ptr(sqrt_1macp), _ptr(x_t), _ptr(v),
                                    B, x.numel() // B), "ddpm_noise_mix")
    return x_t, v


def mse_loss(pred, target, weight=None, want_grad: bool = True, grad_scale: float = 1.0):
    """mean_b(mean_chw((pred-target)^2 * w_b)) in fp32 + fused d(loss)/d(pred).  Returns (loss[1], per_sample[B], dpred)."""
    L = _l.load()
    _chk(pred, BF16, "pred"); _chk(target, BF16, "target")
    pred = pred.contiguous(); target = target.contiguous()
    B = pred.shape[0]
    loss = torch.empty(1, dtype=F32, device=pred.device)
    per_sample = torch.empty(B, dtype=F32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    if weight is not None:
        _chk(weight, F32, "weight")
    _l.check(L.st355_mse_loss(_stream(), _ptr(pred), _ptr(target), _ptr(weight), _ptr(loss), _ptr(per_sample), _ptr(dpred),
                              B, pred.numel() // B, grad_scale), "mse_loss")
    return loss, per_sample, dpred


LOSS_TYPES = {"l2": 0, "huber": 1, "smooth_l1": 2}


def cond_loss(pred, target, loss_type: str = "l2", huber_c=0.1, weight=None, want_grad: bool = True, grad_scale: float = 1.0, emask=None):
    """conditional_loss(reduction='none') -> [* emask] -> per-sample mean -> batch mean (common.py:6132-6166, 6402-6429) + fused d(loss)/d(pred).
    huber_c: float or fp32 device tensor [B] (scheduled huber).  emask: fp32 [B, H*W] element mask broadcast over the channels (conditioning-mask
    losses) or None.  Returns (loss[1], per_sample[B], dpred)."""
    L = _l.load()
    _chk(pred, BF16, "pred"); _chk(target, BF16, "target")
    pred = pred.contiguous(); target = target.contiguous()
    B = pred.shape[0]
    loss = torch.empty(1, dtype=F32, device=pred.device)
    per_sample = torch.empty(B, dtype=F32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    if loss_type != "l2":
        if not torch.is_tensor(huber_c):
            huber_c = torch.full((B,), float(huber_c), dtype=F32, device=pred.device)
        _chk(huber_c, F32, "huber_c")
        huber_c = huber_c.contiguous()
    else:
        huber_c = None
    if weight is not None:
        _chk(weight, F32, "weight")
    period = 0
    if emask is not None:
        _chk(emask, F32, "emask")
        emask = emask.reshape(B, -1).contiguous()
        period = emask.shape[1]
    _l.check(L.st355_cond_loss_masked(_stream(), _ptr(pred), _ptr(target), _ptr(weight), _ptr(huber_c), LOSS_TYPES[loss_type], _ptr(emask), period,
                                      _ptr(loss), _ptr(per_sample), _ptr(dpred), B, pred.numel() // B, grad_scale), "cond_loss")
    return loss, per_sample, dpred


def _rf_rows(ts, names):
    """the [B, N] bf16 operands of the ReflexFlow ops: device tensors of one shape, N % 8 == 0, B < 65536; returns (contiguous tensors, B, N)"""
    out = []
    for t, name in zip(ts, names):
        _chk(t, BF16, name)
        if t.shape != ts[0].shape:
            raise _l.St355Error(f"{name}: shape {tuple(t.shape)} differs from {names[0]}'s {tuple(ts[0].shape)}")
        out.append(t.contiguous())
    B = ts[0].shape[0]
    N = ts[0].numel() // B
    if N % 8 != 0 or not 0 < B < 65536:
        raise _l.St355Error(f"{names[0]}: per-sample size {N} must be a multiple of 8 and the batch {B} below 65536")
    return out, B, N


def _rf_scratch(dev, B: int, N: int):
    return _scratch("reflexflow", dev, _l.load().st355_reflexflow_workspace(B, N))


def reflexflow_stats(pred, noisy, latents, clean=None, biased=None):
    """fp32 [B, 4] per sample: sum |clean - biased| (0 without the pair), sum p^2, sum tau^2, sum p tau, tau = noisy - latents; fixed-order two-stage reduction"""
    L = _l.load()
    if (clean is None) != (biased is None):
        raise _l.St355Error("reflexflow_stats: clean and biased come together or not at all")
    pair = [clean, biased] if clean is not None else []
    ts, B, N = _rf_rows([pred, noisy, latents] + pair, ["pred", "noisy", "latents", "clean", "biased"])
    stats = torch.empty(B, 4, dtype=F32, device=pred.device)
    ws = _rf_scratch(pred.device, B, N)
    _l.check(L.st355_reflexflow_stats(_stream(), _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]) if pair else None, _ptr(ts[4]) if pair else None,
                                      _ptr(stats), _ptr(ws), B, N), "reflexflow_stats")
    return stats


def reflexflow_loss(pred, target, noisy, latents, stats, loss_type: str = "l2", huber_c=0.1, clean=None, biased=None, alpha: float = 1.0, beta1: float = 10.0,
                    beta2: float = 1.0, want_grad: bool = True, grad_scale: float = 1.0, emask=None):
    """ops.cond_loss plus the ReflexFlow terms (common.py:6287-6318): the exposure weight 1 + alpha (clean - biased) / max(stats[:, 0], 1e-6) per element, beta2, the
    mask, the per-sample mean, + beta1 * sum (p / |p| - tau / |tau|)^2 (norms clamped at 1e-6, from `stats` = reflexflow_stats(...)), the batch mean, and the fused
    d(loss)/d(pred).  Returns (loss[1], per_sample[B], adr[B] (the term as added), dpred)."""
    L = _l.load()
    if (clean is None) != (biased is None):
        raise _l.St355Error("reflexflow_loss: clean and biased come together or not at all")
    pair = [clean, biased] if clean is not None else []
    ts, B, N = _rf_rows([pred, target, noisy, latents] + pair, ["pred", "target", "noisy", "latents", "clean", "biased"])
    _chk(stats, F32, "stats")
    if tuple(stats.shape) != (B, 4) or not stats.is_contiguous():
        raise _l.St355Error(f"stats: expected a contiguous fp32 [{B}, 4] tensor (reflexflow_stats), got {tuple(stats.shape)}")
    dev = pred.device
    loss = torch.empty(1, dtype=F32, device=dev)
    per_sample = torch.empty(B, dtype=F32, device=dev)
    adr = torch.empty(B, dtype=F32, device=dev)
    dpred = torch.empty_like(ts[0]) if want_grad else None
    if loss_type != "l2":
        if not torch.is_tensor(huber_c):
            huber_c = torch.full((B,), float(huber_c), dtype=F32, device=dev)
        _chk(huber_c, F32, "huber_c")
        huber_c = huber_c.contiguous()
        if huber_c.numel() != B:
            raise _l.St355Error(f"huber_c: expected {B} values, got {huber_c.numel()}")
    else:
        huber_c = None
    period = 0
    if emask is not None:
        _chk(emask, F32, "emask")
        emask = emask.reshape(B, -1).contiguous()
        period = emask.shape[1]
    ws = _rf_scratch(dev, B, N)
    _l.check(L.st355_reflexflow_loss(_stream(), _ptr(ts[0]), _ptr(ts[1]), _ptr(huber_c), LOSS_TYPES[loss_type], _ptr(emask), period, _ptr(ts[2]), _ptr(ts[3]),
                                     _ptr(ts[4]) if pair else None, _ptr(ts[5]) if pair else None, _ptr(stats), float(alpha), float(beta1), float(beta2),
                                     _ptr(loss), _ptr(per_sample), _ptr(adr), _ptr(dpred), _ptr(ws), B, N, grad_scale), "reflexflow_loss")
    return loss, per_sample, adr, dpred


def flow_euler_step(x, v, dt):
    """x[b] += dt[b] * v[b] in place (bf16 [B, ...] contiguous, dt fp32 [B] on the device): fp32 arithmetic, one rounding.  Returns x."""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(v, BF16, "v"); _chk(dt, F32, "dt")
    B = x.shape[0]
    N = x.numel() // B
    if not x.is_contiguous() or x.shape != v.shape or dt.numel() != B or N % 8 != 0:
        raise _l.St355Error(f"flow_euler_step: x must be contiguous (it is updated in place), v of its shape, dt [{B}] and the per-sample size {N} a multiple of 8")
    v = v.contiguous()
    if v.data_ptr() == x.data_ptr():
        raise _l.St355Error("flow_euler_step: x and v must be different buffers")
    _l.check(L.st355_flow_euler_step(_stream(), _ptr(x), _ptr(v), _ptr(dt.contiguous()), B, N), "flow_euler_step")
    return x


def twinflow_rcgm_step(x, acc, fc, t_prev, t_next, first: bool):
    """One step of TwinFlow's RCGM teacher integration, in place: x[b] += (t_next[b] - t_prev[b]) fc[b] (bf16, fp32 arithmetic, one rounding) and
    acc[b] = (0 if first else acc[b]) + (t_prev[b] - t_next[b]) fc[b] (fp32), one pass over fc.  t_prev / t_next: fp32 [B] on the device.  Returns (x, acc)."""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(fc, BF16, "fc"); _chk(acc, F32, "acc"); _chk(t_prev, F32, "t_prev"); _chk(t_next, F32, "t_next")
    B = x.shape[0]
    N = x.numel() // B
    if not x.is_contiguous() or not acc.is_contiguous() or x.shape != fc.shape or acc.shape != x.shape or t_prev.numel() != B or t_next.numel() != B or N % 8 != 0:
        raise _l.St355Error(f"twinflow_rcgm_step: x and acc must be contiguous (they are updated in place), fc and acc of x's shape, t_prev / t_next [{B}] and the "
                            f"per-sample size {N} a multiple of 8")
    fc = fc.contiguous()
    if fc.data_ptr() == x.data_ptr():
        raise _l.St355Error("twinflow_rcgm_step: x and fc must be different buffers")
    _l.check(L.st355_twinflow_rcgm_step(_stream(), _ptr(x), _ptr(acc), _ptr(fc), _ptr(t_prev.contiguous()), _ptr(t_next.contiguous()), 1 if first else 0, B, N),
             "twinflow_rcgm_step")
    return x, acc


def twinflow_loss(pred, target, acc, cond=None, uncond=None, ratio: float = 0.0, clamp: float = 1.0, want_grad: bool = True, grad_scale: float = 1.0):
    """TwinFlow's two terms on the training prediction (common.py `_compute_twinflow_losses`): t' = target + ratio (cond - uncond), r = pred - acc - t';
    losses[0] = mean clamp(r, +-clamp)^2 (the RCGM base term: the target is detached), losses[1] = mean (pred - t')^2 (real velocity), plain means over the whole
    tensor, fixed-order two-stage reduction; dpred = grad_scale (2 / N) (clamp(r) + (pred - t')) from the same pass.  Returns (losses fp32 [2], dpred or None)."""
    L = _l.load()
    if (cond is None) != (uncond is None):
        raise _l.St355Error("twinflow_loss: cond and uncond come together or not at all")
    pair = [cond, uncond] if cond is not None else []
    ts, B, N = _rf_rows([pred, target] + pair, ["pred", "target", "cond", "uncond"])
    _chk(acc, F32, "acc")
    if acc.shape != pred.shape or not acc.is_contiguous():
        raise _l.St355Error(f"acc: expected a contiguous fp32 tensor of pred's shape {tuple(pred.shape)}, got {tuple(acc.shape)}")
    if not float(clamp) >= 0.0:
        raise _l.St355Error(f"twinflow_loss: the clamp ({clamp}) must not be negative")
    dev = pred.device
    losses = torch.empty(2, dtype=F32, device=dev)
    dpred = torch.empty_like(ts[0]) if want_grad else None
    ws = _scratch("twinflow", dev, L.st355_twinflow_workspace(B, N))
    _l.check(L.st355_twinflow_loss(_stream(), _ptr(ts[0]), _ptr(ts[1]), _ptr(acc), _ptr(ts[2]) if pair else None, _ptr(ts[3]) if pair else None, float(ratio),
                                   float(clamp), _ptr(losses), _ptr(dpred), _ptr(ws), B, N, float(grad_scale)), "twinflow_loss")
    return losses, dpred


def twinflow_ucgm_step(x, v, s_cur: float, s_next: float, rho: float = 0.0, noise=None):
    """The UCGM sampler's step (custom_schedule.py `TwinFlowScheduler.step`), in place on bf16 x:
    x <- (1 - s_next) (x - s_cur v) + s_next ((x + (1 - s_cur) v) sqrt(1 - rho) + noise sqrt(rho)); noise may be None when rho == 0.  Returns x."""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(v, BF16, "v")
    n = x.numel()
    if not x.is_contiguous() or x.shape != v.shape or n % 8 != 0 or n == 0:
        raise _l.St355Error(f"twinflow_ucgm_step: x must be contiguous (it is updated in place), v of its shape and the element count {n} a positive multiple of 8")
    if not 0.0 <= float(rho) <= 1.0:
        raise _l.St355Error(f"twinflow_ucgm_step: rho ({rho}) must lie in [0, 1]")
    v = v.contiguous()
    if noise is not None:
        _chk(noise, BF16, "noise")
        if noise.shape != x.shape:
            raise _l.St355Error(f"noise: shape {tuple(noise.shape)} differs from x's {tuple(x.shape)}")
        noise = noise.contiguous()
    elif float(rho) != 0.0:
        raise _l.St355Error("twinflow_ucgm_step: rho > 0 needs noise")
    if v.data_ptr() == x.data_ptr() or (noise is not None and noise.data_ptr() == x.data_ptr()):
        raise _l.St355Error("twinflow_ucgm_step: x, v and noise must be different buffers")
    _l.check(L.st355_twinflow_ucgm_step(_stream(), _ptr(x), _ptr(v), _ptr(noise), float(s_cur), float(s_next), float(rho), n), "twinflow_ucgm_step")
    return x


EVAL_MAX_STACK = 64


def eval_flow_views(latents, noise, sigma, out=None):
    """The evaluation pass's noisy rows for K timesteps of the same samples: out[k, b] = (1 - sigma[k]) latents[b] + sigma[k] noise[b] (bf16 [K, B, ...]; sigma fp32
    [K] on the device, 1 <= K <= 64), latents and noise read once.  Slab k is bit-identical to flow_noise_mix(latents, sigma[k] for every row, noise=noise)[0].
    `out`: a contiguous bf16 tensor of K * latents.numel() elements to write into (overlapping neither input), else allocated.  Returns out."""
    L = _l.load()
    _chk(latents, BF16, "latents"); _chk(noise, BF16, "noise"); _chk(sigma, F32, "sigma")
    B = latents.shape[0]
    N = latents.numel() // max(B, 1)
    K = sigma.numel()
    if noise.shape != latents.shape:
        raise _l.St355Error(f"noise: shape {tuple(noise.shape)} differs from latents' {tuple(latents.shape)}")
    if B <= 0 or N <= 0 or N % 8 != 0:
        raise _l.St355Error(f"eval_flow_views: the per-sample size {N} must be a positive multiple of 8 and the batch {B} positive")
    if not 1 <= K <= EVAL_MAX_STACK or sigma.dim() != 1:
        raise _l.St355Error(f"sigma: expected a 1-D tensor of 1 to {EVAL_MAX_STACK} values, got shape {tuple(sigma.shape)}")
    latents, noise, sigma = latents.contiguous(), noise.contiguous(), sigma.contiguous()
    if out is None:
        out = torch.empty((K,) + tuple(latents.shape), dtype=BF16, device=latents.device)
    else:
        _chk(out, BF16, "out")
        if not out.is_contiguous() or out.numel() != K * latents.numel():
            raise _l.St355Error(f"out: expected a contiguous bf16 tensor of {K * latents.numel()} elements, got shape {tuple(out.shape)} stride {out.stride()}")
        lo, hi = out.data_ptr(), out.data_ptr() + 2 * out.numel()
        for t in (latents, noise):
            if t.data_ptr() < hi and lo < t.data_ptr() + 2 * t.numel():
                raise _l.St355Error("eval_flow_views: out must not overlap latents or noise")
    _l.check(L.st355_eval_flow_views(_stream(), _ptr(latents), _ptr(noise), _ptr(sigma), _ptr(out), B, N, K), "eval_flow_views")
    return out


def eval_loss(pred, target, loss_type: str = "l2", huber_c=0.1, loss_out=None):
    """The evaluation loss of K stacked timesteps: pred bf16 [K, B, ...] against the ONE target bf16 [B, ...] — the l2 / huber / smooth_l1 element loss, the per-sample
    mean, the batch mean, per slab (what cond_loss computes for each slab alone, without gradient, mask or weights).  huber_c: float or fp32 device tensor of K * B
    values.  `loss_out`: a contiguous fp32 [K] view to write the K losses into (a row segment of a device-resident result table), else allocated.  The values do not
    depend on K or on a slab's position.  Returns (loss [K], per_sample [K, B])."""
    L = _l.load()
    _chk(pred, BF16, "pred"); _chk(target, BF16, "target")
    if loss_type not in LOSS_TYPES:
        raise _l.St355Error(f"eval_loss: loss_type {loss_type!r} is not one of {sorted(LOSS_TYPES)}")
    if pred.dim() != target.dim() + 1 or tuple(pred.shape[1:]) != tuple(target.shape):
        raise _l.St355Error(f"pred: expected shape [K, {', '.join(str(s) for s in target.shape)}], got {tuple(pred.shape)}")
    K, B = pred.shape[0], target.shape[0]
    N = target.numel() // max(B, 1)
    if not 1 <= K <= EVAL_MAX_STACK:
        raise _l.St355Error(f"eval_loss: the timestep count {K} must lie in [1, {EVAL_MAX_STACK}]")
    if N <= 0 or N % 8 != 0 or not 0 < B < 65536:
        raise _l.St355Error(f"eval_loss: per-sample size {N} must be a positive multiple of 8 and the batch {B} below 65536")
    pred, target = pred.contiguous(), target.contiguous()
    dev = pred.device
    if loss_type != "l2":
        if not torch.is_tensor(huber_c):
            huber_c = torch.full((K * B,), float(huber_c), dtype=F32, device=dev)
        _chk(huber_c, F32, "huber_c")
        huber_c = huber_c.contiguous()
        if huber_c.numel() != K * B:
            raise _l.St355Error(f"huber_c: expected {K * B} values, got {huber_c.numel()}")
    else:
        huber_c = None
    if loss_out is None:
        loss_out = torch.empty(K, dtype=F32, device=dev)
    else:
        _chk(loss_out, F32, "loss_out")
        if not loss_out.is_contiguous() or loss_out.numel() != K:
            raise _l.St355Error(f"loss_out: expected a contiguous fp32 view of {K} values, got shape {tuple(loss_out.shape)} stride {loss_out.stride()}")
    per_sample = torch.empty(K, B, dtype=F32, device=dev)
    ws = _scratch("eval_loss", dev, L.st355_eval_loss_workspace(B, N, K))
    _l.check(L.st355_eval_loss(_stream(), _ptr(pred), _ptr(target), LOSS_TYPES[loss_type], _ptr(huber_c), _ptr(per_sample), _ptr(loss_out), _ptr(ws), B, N, K),
             "eval_loss")
    return loss_out, per_sample


DIFF2FLOW_MODES = {"epsilon": 0, "v_prediction": 1}


def _d2f_rows(pred, noisy, tau, timesteps, table, weight, emask):
    """the operands of the Diff2Flow loss: pred bf16 [B, ...] whose per-sample block is dense (a leading-channel slice of a wider output is read in place through
    its batch stride), noisy / tau bf16 of its shape, timesteps int64 [B], table fp32 [T, 2], weight fp32 [B] or None, emask fp32 [B, period] or None;
    returns (pred, contiguous noisy, tau, timesteps, table, emask, B, N, pred stride, period)"""
    _chk(pred, BF16, "pred"); _chk(noisy, BF16, "noisy"); _chk(tau, BF16, "tau"); _chk(table, F32, "table")
    _chk(timesteps, torch.int64, "timesteps")
    if noisy.shape != pred.shape or tau.shape != pred.shape:
        raise _l.St355Error(f"diff2flow_loss: noisy {tuple(noisy.shape)} and tau {tuple(tau.shape)} must have pred's shape {tuple(pred.shape)}")
    B = pred.shape[0]
    N = pred.numel() // B if B else 0
    if N <= 0 or not 0 < B < 65536:
        raise _l.St355Error(f"pred: the batch {B} must lie in [1, 65535] and the per-sample size {N} be positive")
    if not pred[0].is_contiguous() or (B > 1 and pred.stride(0) < N):
        pred = pred.contiguous()                                          # (an inner-strided view; the models' predictions never are)
    stride = pred.stride(0) if B > 1 else N
    if timesteps.numel() != B:
        raise _l.St355Error(f"timesteps: expected {B} values, got {timesteps.numel()}")
    if table.dim() != 2 or table.shape[1] != 2 or table.shape[0] < 1 or not table.is_contiguous():
        raise _l.St355Error(f"table: expected a contiguous fp32 [T, 2] tensor, got {tuple(table.shape)}")
    if weight is not None:
        _chk(weight, F32, "weight")
        if weight.numel() != B:
            raise _l.St355Error(f"weight: expected {B} values, got {weight.numel()}")
        weight = weight.contiguous()
    period = 0
    if emask is not None:
        _chk(emask, F32, "emask")
        emask = emask.reshape(B, -1).contiguous()
        period = emask.shape[1]
        if period <= 0 or N % period != 0:
            raise _l.St355Error(f"emask: period {period} must divide the per-sample size {N}")
    return pred, noisy.contiguous(), tau.contiguous(), timesteps.reshape(-1).contiguous(), table, weight, emask, B, N, stride, period


def diff2flow_loss(pred, noisy, tau, timesteps, table, mode: str = "epsilon", weight=None, want_grad: bool = True, grad_scale: float = 1.0, emask=None):
    """The Diff2Flow loss (bridge.py + common.py:6231-6248, 6402-6429) in one pass.  With (c0, c1) = table[clamp(timesteps[b], 0, T - 1)] — (sqrt(1/a), sqrt(1/a - 1))
    for mode "epsilon", (sqrt(a), sqrt(1 - a)) for "v_prediction" — gathered on the device:  z = c0 x - c1 p;  f = p - z  (epsilon)  or  (c0 p + c1 x) - z  (v);
    (f - tau)^2 [* emask] -> per-sample mean [* weight] -> batch mean, and the fused d(loss)/d(pred) (compact bf16, one rounding).  pred may be a leading-channel
    slice of a wider output: it is read in place.  Returns (loss[1], per_sample[B], dpred)."""
    L = _l.load()
    if mode not in DIFF2FLOW_MODES:
        raise _l.St355Error(f"diff2flow_loss: mode must be one of {sorted(DIFF2FLOW_MODES)}, got {mode!r}")
    pred, noisy, tau, timesteps, table, weight, emask, B, N, stride, period = _d2f_rows(pred, noisy, tau, timesteps, table, weight, emask)
    dev = pred.device
    loss = torch.empty(1, dtype=F32, device=dev)
    per_sample = torch.empty(B, dtype=F32, device=dev)
    dpred = torch.empty(pred.shape, dtype=BF16, device=dev) if want_grad else None
    ws = _scratch("diff2flow", dev, L.st355_diff2flow_workspace(B, N))
    _l.check(L.st355_diff2flow_loss(_stream(), _ptr(pred), stride, _ptr(noisy), _ptr(tau), _ptr(timesteps), _ptr(table), table.shape[0], DIFF2FLOW_MODES[mode],
                                    _ptr(weight), _ptr(emask), period, _ptr(loss), _ptr(per_sample), _ptr(dpred), _ptr(ws), B, N, grad_scale), "diff2flow_loss")
    return loss, per_sample, dpred


LCM_MODES = DIFF2FLOW_MODES
LCM_LOSSES = {"l2": 0, "huber": 1}


def _lcm_rows(name, mode, tensors, index_like, tables):
    """the operands of the LCM kernels: `tensors` (name, tensor, dtype, rows per sample-batch) of one [B, ...] shape (the teacher pair has 2B rows), `index_like` int64 [B]
    vectors, `tables` contiguous fp32 [len, 2]; returns (B, N) and the tensors made contiguous, in order"""
    if mode not in LCM_MODES:
        raise _l.St355Error(f"{name}: mode must be one of {sorted(LCM_MODES)}, got {mode!r}")
    lead = tensors[0][1]
    B = lead.shape[0]
    N = lead.numel() // B if B else 0
    if N <= 0 or not 0 < B < 32768:
        raise _l.St355Error(f"{name}: the batch {B} must lie in [1, 32767] and the per-sample size {N} be positive")
    out = []
    for nm, t, dt, mult in tensors:
        _chk(t, dt, nm)
        if t.shape[0] != mult * B or t.numel() != mult * B * N:
            raise _l.St355Error(f"{name}: {nm} {tuple(t.shape)} must hold {mult * B} rows of {N} elements")
        out.append(t.contiguous())
    for nm, t in index_like:
        _chk(t, torch.int64, nm)
        if t.numel() != B:
            raise _l.St355Error(f"{name}: {nm}: expected {B} values, got {t.numel()}")
        out.append(t.reshape(-1).contiguous())
    for nm, t in tables:
        _chk(t, F32, nm)
        if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1 or not t.is_contiguous():
            raise _l.St355Error(f"{name}: {nm}: expected a contiguous fp32 [len, 2] tensor, got {tuple(t.shape)}")
    return (B, N), out


def lcm_solver_step(x_s, teacher_pair, w, index, start, sched, prev, mode: str = "epsilon"):
    """The teacher's DDIM solver step of LCM distillation (lcm/__init__.py:229-252) in one pass.  teacher_pair bf16 [2B, ...]: the conditional predictions, then the
    unconditional ones; p = p_u + w (p_c - p_u); x0 / eps of p at (x_s, sched[start]) by `mode`; x_prev = prev[index].0 x0 + prev[index].1 eps.  Returns (x_prev fp32,
    x_prev bf16), both of x_s's shape."""
    L = _l.load()
    (B, N), (x_s, teacher_pair, index, start) = _lcm_rows("lcm_solver_step", mode, [("x_s", x_s, BF16, 1), ("teacher_pair", teacher_pair, BF16, 2)],
                                                          [("index", index), ("start", start)], [("sched", sched), ("prev", prev)])
    _chk(w, F32, "w")
    if w.numel() != B:
        raise _l.St355Error(f"lcm_solver_step: w: expected {B} values, got {w.numel()}")
    w = w.reshape(-1).contiguous()
    x32 = torch.empty(x_s.shape, dtype=F32, device=x_s.device)
    x16 = torch.empty(x_s.shape, dtype=BF16, device=x_s.device)
    _l.check(L.st355_lcm_solver_step(_stream(), _ptr(x_s), _ptr(teacher_pair), _ptr(w), _ptr(index), _ptr(start), _ptr(sched), sched.shape[0], _ptr(prev), prev.shape[0],
                                     LCM_MODES[mode], _ptr(x32), _ptr(x16), B, N), "lcm_solver_step")
    return x32, x16


def lcm_target(x_prev32, pred_t, timesteps, sched, mode: str = "epsilon", timestep_scaling: float = 10.0):
    """The consistency target (lcm/__init__.py:262-263): c_skip(t) x_prev + c_out(t) x0(pred_t at (x_prev, sched[t])), fp32; rows with t = 0 return x_prev exactly."""
    L = _l.load()
    (B, N), (x_prev32, pred_t, timesteps) = _lcm_rows("lcm_target", mode, [("x_prev32", x_prev32, F32, 1), ("pred_t", pred_t, BF16, 1)], [("timesteps", timesteps)],
                                                      [("sched", sched)])
    target = torch.empty(x_prev32.shape, dtype=F32, device=x_prev32.device)
    _l.check(L.st355_lcm_target(_stream(), _ptr(x_prev32), _ptr(pred_t), _ptr(timesteps), _ptr(sched), sched.shape[0], LCM_MODES[mode], float(timestep_scaling),
                                _ptr(target), B, N), "lcm_target")
    return target


def lcm_loss(pred, x_s, target, start, sched, mode: str = "epsilon", timestep_scaling: float = 10.0, loss_type: str = "l2", huber_c: float = 0.001,
             want_grad: bool = True, grad_scale: float = 1.0):
    """The LCM consistency loss (lcm/__init__.py:282-327) and its gradient in one pass: m = c_skip(start) x_s + c_out(start) x0(pred at (x_s, sched[start]));
    l2: mean (m - target)^2, huber: mean sqrt((m - target)^2 + c^2) - c.  Returns (loss[1], per_sample[B], dpred bf16 or None)."""
    L = _l.load()
    if loss_type not in LCM_LOSSES:
        raise _l.St355Error(f"lcm_loss: loss_type must be one of {sorted(LCM_LOSSES)}, got {loss_type!r}")
    (B, N), (pred, x_s, target, start) = _lcm_rows("lcm_loss", mode, [("pred", pred, BF16, 1), ("x_s", x_s, BF16, 1), ("target", target, F32, 1)], [("start", start)],
                                                   [("sched", sched)])
    dev = pred.device
    loss = torch.empty(1, dtype=F32, device=dev)
    per_sample = torch.empty(B, dtype=F32, device=dev)
    dpred = torch.empty(pred.shape, dtype=BF16, device=dev) if want_grad else None
    ws = _scratch("lcm", dev, L.st355_lcm_workspace(B, N))
    _l.check(L.st355_lcm_loss(_stream(), _ptr(pred), _ptr(x_s), _ptr(target), _ptr(start), _ptr(sched), sched.shape[0], LCM_MODES[mode], float(timestep_scaling),
                              LCM_LOSSES[loss_type], float(huber_c), _ptr(loss), _ptr(per_sample), _ptr(dpred), _ptr(ws), B, N, grad_scale), "lcm_loss")
    return loss, per_sample, dpred


def lcm_sample_step(x, pred, noise, sched, t: int, t_next: int, mode: str = "epsilon", timestep_scaling: float = 10.0):
    """One LCMScheduler step: denoised = c_skip(t) x + c_out(t) x0(pred at (x, sched[t])); returns sched[t_next].0 denoised + sched[t_next].1 noise, or denoised on
    the last step (t_next < 0, noise None).  bf16 in, bf16 out (one rounding)."""
    L = _l.load()
    if mode not in LCM_MODES:
        raise _l.St355Error(f"lcm_sample_step: mode must be one of {sorted(LCM_MODES)}, got {mode!r}")
    _chk(x, BF16, "x"); _chk(pred, BF16, "pred"); _chk(sched, F32, "sched")
    if pred.shape != x.shape or x.numel() == 0:
        raise _l.St355Error(f"lcm_sample_step: pred {tuple(pred.shape)} must have x's shape {tuple(x.shape)}")
    if sched.dim() != 2 or sched.shape[1] != 2 or not sched.is_contiguous():
        raise _l.St355Error(f"lcm_sample_step: sched: expected a contiguous fp32 [T, 2] tensor, got {tuple(sched.shape)}")
    t_next = int(t_next)
    if t_next >= 0:
        if noise is None:
            raise _l.St355Error("lcm_sample_step: every step but the last (t_next < 0) needs its noise")
        _chk(noise, BF16, "noise")
        if noise.shape != x.shape:
            raise _l.St355Error(f"lcm_sample_step: noise {tuple(noise.shape)} must have x's shape {tuple(x.shape)}")
        noise = noise.contiguous()
    else:
        noise = None
    x, pred = x.contiguous(), pred.contiguous()
    out = torch.empty_like(x)
    _l.check(L.st355_lcm_sample_step(_stream(), _ptr(x), _ptr(pred), _ptr(noise), _ptr(sched), sched.shape[0], LCM_MODES[mode], float(timestep_scaling), int(t), t_next,
                                     _ptr(out), x.numel()), "lcm_sample_step")
    return out


FLOW_DPO_NORMS = {"sum": 0, "mean": 1, "masked_mean": 2}
FLOW_DPO_LOGS = ("flow_dpo_loss", "flow_dpo_beta", "flow_dpo_margin", "flow_dpo_win_adv", "flow_dpo_lose_adv", "flow_dpo_policy_win_err",
                 "flow_dpo_policy_lose_err", "flow_dpo_ref_win_err", "flow_dpo_ref_lose_err", "flow_dpo_negative_margin_pct", "flow_dpo_gradient_factor", "total",
                 "flow_dpo_anchor_loss", "flow_dpo_margin_abs", "flow_dpo_margin_ema", "original_loss")          # the entries of flow_dpo_head's log vector, in order


def _fd_rows(policy, ref, target_w, target_l, emask):
    """the operands of the Flow-DPO ops: policy / ref bf16 [2B, ...], the targets bf16 [B, ...] of the same per-sample shape, emask fp32 [B, period] or None;
    returns (contiguous tensors, B, N, emask, period)"""
    _chk(policy, BF16, "policy"); _chk(target_w, BF16, "target_w"); _chk(target_l, BF16, "target_l")
    if ref is not None:
        _chk(ref, BF16, "ref")
        if ref.shape != policy.shape:
            raise _l.St355Error(f"ref: shape {tuple(ref.shape)} differs from policy's {tuple(policy.shape)}")
    if policy.shape[0] % 2 != 0 or target_w.shape != target_l.shape or target_w.shape[0] * 2 != policy.shape[0] or target_w.shape[1:] != policy.shape[1:]:
        raise _l.St355Error(f"flow_dpo: policy [2B, ...] {tuple(policy.shape)} needs targets [B, ...], got {tuple(target_w.shape)} / {tuple(target_l.shape)}")
    B = target_w.shape[0]
    N = target_w.numel() // B
    if N % 8 != 0 or not 0 < B < 32768:
        raise _l.St355Error(f"flow_dpo: per-sample size {N} must be a multiple of 8 and the pair count {B} below 32768")
    period = 0
    if emask is not None:
        _chk(emask, F32, "emask")
        emask = emask.reshape(B, -1).contiguous()
        period = emask.shape[1]
        if period % 8 != 0 or N % period != 0:
            raise _l.St355Error(f"emask: period {period} must be a multiple of 8 dividing the per-sample size {N}")
    return [policy.contiguous(), None if ref is None else ref.contiguous(), target_w.contiguous(), target_l.contiguous()], B, N, emask, period


def flow_dpo_stats(policy, ref, target_w, target_l, emask=None):
    """fp32 [B, 9] per pair (rows [0, B) of policy / ref: preferred, [B, 2B): rejected): the four masked errors (policy preferred, policy rejected, reference
    preferred, reference rejected), the two anchor sums sum (p - r)^2, the mask sum, and the preferred / rejected advantages accumulated element by element;
    fixed-order two-stage reduction"""
    L = _l.load()
    ts, B, N, emask, period = _fd_rows(policy, ref, target_w, target_l, emask)
    if ts[1] is None:
        raise _l.St355Error("flow_dpo_stats: the reference prediction is required")
    stats = torch.empty(B, 9, dtype=F32, device=policy.device)
    ws = _scratch("flow_dpo", policy.device, L.st355_flow_dpo_workspace(B, N))
    _l.check(L.st355_flow_dpo_stats(_stream(), _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]), _ptr(emask), period, _ptr(stats), _ptr(ws), B, N), "flow_dpo_stats")
    return stats


def flow_dpo_head(stats, per_sample: int, norm_type: str = "sum", has_mask: bool = False, beta: float = 1.0, loss_weight: float = 1.0, anchor_alpha: float = 0.0,
                  ema_state=None, auto_num: float = 0.0, decay: float = 0.99, beta_min=None, beta_max=None, eps: float = 1e-6, original_loss=None,
                  sft_weight: float = 0.0, reduce_absmean=None):
    """The one-workgroup head over flow_dpo_stats' [B, 9]: nu, the margins, beta (auto-beta when `ema_state`, fp32 [2] on the device = (ema, initialised), is
    given: it is updated in place; auto_num = -2 logit(target)), the logits, the loss and the per-pair coefficients.  reduce_absmean: a callable that averages
    the device scalar mean_b |margin_b| over the ranks in place (world size > 1), run between the head's two launches.  Returns (loss[1], pair [B, 4] = (margin,
    logit, c, nu), logs fp32 [16] in the order of FLOW_DPO_LOGS)."""
    L = _l.load()
    _chk(stats, F32, "stats")
    if stats.dim() != 2 or stats.shape[1] != 9 or not stats.is_contiguous():
        raise _l.St355Error(f"stats: expected a contiguous fp32 [B, 9] tensor (flow_dpo_stats), got {tuple(stats.shape)}")
    B, dev = stats.shape[0], stats.device
    auto = ema_state is not None
    if auto:
        _chk(ema_state, F32, "ema_state")
        if ema_state.numel() != 2 or not ema_state.is_contiguous():
            raise _l.St355Error("ema_state: expected a contiguous fp32 [2] tensor (ema, initialised)")
    if original_loss is not None:
        _chk(original_loss, F32, "original_loss")
    loss = torch.empty(1, dtype=F32, device=dev)
    pair = torch.empty(B, 4, dtype=F32, device=dev)
    logs = torch.empty(16, dtype=F32, device=dev)
    absmean = torch.empty(1, dtype=F32, device=dev)
    inf = float("inf")

    def launch(mode):
        _l.check(L.st355_flow_dpo_head(_stream(), _ptr(stats), FLOW_DPO_NORMS[norm_type], int(bool(has_mask)), mode, _ptr(absmean), _ptr(ema_state), int(auto),
                                       float(beta), float(auto_num), float(decay), -inf if beta_min is None else float(beta_min),
                                       inf if beta_max is None else float(beta_max), float(eps), float(loss_weight), float(anchor_alpha), _ptr(original_loss),
                                       float(sft_weight), _ptr(pair), _ptr(loss), _ptr(logs), B, int(per_sample)), "flow_dpo_head")

    if auto and reduce_absmean is not None:
        launch(1)
        reduce_absmean(absmean)
        launch(2)
    else:
        launch(0)
    return loss, pair, logs


def flow_dpo_grad(policy, ref, target_w, target_l, pair, emask=None, anchor_alpha: float = 0.0, grad_scale: float = 1.0, upstream=None):
    """d loss / d policy, bf16 [2B, ...] in one write: +-2 c_b nu_b m (p - t) + anchor_alpha (p - r) / (B n), times grad_scale (and the device scalar `upstream`)"""
    L = _l.load()
    ts, B, N, emask, period = _fd_rows(policy, ref, target_w, target_l, emask)
    _chk(pair, F32, "pair")
    if tuple(pair.shape) != (B, 4) or not pair.is_contiguous():
        raise _l.St355Error(f"pair: expected a contiguous fp32 [{B}, 4] tensor (flow_dpo_head), got {tuple(pair.shape)}")
    if float(anchor_alpha) != 0.0 and ts[1] is None:
        raise _l.St355Error("flow_dpo_grad: the anchor term (anchor_alpha != 0) needs the reference prediction")
    if upstream is not None:
        _chk(upstream, F32, "upstream")
        upstream = upstream.reshape(-1).contiguous()
        if upstream.numel() != 1:
            raise _l.St355Error("upstream: expected one fp32 device scalar")
    dpred = torch.empty_like(ts[0])
    _l.check(L.st355_flow_dpo_grad(_stream(), _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]), _ptr(emask), period, _ptr(pair), _ptr(dpred), B, N,
                                   float(anchor_alpha), float(grad_scale), _ptr(upstream)), "flow_dpo_grad")
    return dpred


def flux_pack(latents):
    L = _l.load()
    _chk(latents, BF16, "latents")
    latents = latents.contiguous()
    B, Cc, H, W = latents.shape
    out = torch.empty(B, (H // 2) * (W // 2), Cc * 4, dtype=BF16, device=latents.device)
    _l.check(L.st355_flux_pack(_stream(), _ptr(latents), _ptr(out), B, Cc, H, W), "flux_pack")
    return out


def flux_unpack(packed, Cc: int, H: int, W: int):
    L = _l.load()
    _chk(packed, BF16, "packed")
    packed = packed.contiguous()
    B = packed.shape[0]
    out = torch.empty(B, Cc, H, W, dtype=BF16, device=packed.device)
    _l.check(L.st355_flux_unpack(_stream(), _ptr(packed), _ptr(out), B, Cc, H, W), "flux_unpack")
    return out


def patchify(latents, order: int = 0):
    """[B,C,H,W] -> [B,(H/2)(W/2),4C]; order 0 = (c,dh,dw) features (Flux pack / PatchEmbed im2col), 1 = (dh,dw,c) (SD3/PixArt)"""
    L = _l.load()
    _chk(latents, BF16, "latents")
    latents = latents.contiguous()
    B, Cc, H, W = latents.shape
    out = torch.empty(B, (H // 2) * (W // 2), Cc * 4, dtype=BF16, device=latents.device)
    _l.check(L.st355_patchify(_stream(), _ptr(latents), _ptr(out), B, Cc, H, W, order), "patchify")
    return out


def unpatchify(packed, Cc: int, H: int, W: int, order: int = 0):
    L = _l.load()
    _chk(packed, BF16, "packed")
    packed = packed.contiguous()
    B = packed.shape[0]
    out = torch.empty(B, Cc, H, W, dtype=BF16, device=packed.device)
    _l.check(L.st355_unpatchify(_stream(), _ptr(packed), _ptr(out), B, Cc, H, W, order), "unpatchify")
    return out


def timestep_proj(t, dim: int, scale: float = 1.0):
    L = _l.load()
    _chk(t, F32, "t")
    out = torch.empty(t.shape[0], dim, dtype=BF16, device=t.device)
    _l.check(L.st355_timestep_proj(_stream(), _ptr(t.contiguous()), _ptr(out), t.shape[0], dim, scale), "timestep_proj")
    return out


def silu(x):
    L = _l.load()
    _chk(x, BF16, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    _l.check(L.st355_silu(_stream(), _ptr(x), _ptr(y), x.numel()), "silu")
    return y


def gelu_tanh(x):
    L = _l.load()
    _chk(x, BF16, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    _l.check(L.st355_gelu_tanh(_stream(), _ptr(x), _ptr(y), x.numel()), "gelu_tanh")
    return y


def silu_bwd(x, dy):
    """dx = dy * silu'(x)"""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(dy, BF16, "dy")
    x = x.contiguous(); dy = dy.contiguous()
    dx = torch.empty_like(x)
    _l.check(L.st355_silu_bwd(_stream(), _ptr(x), _ptr(dy), _ptr(dx), x.numel()), "silu_bwd")
    return dx


def add(a, b):
    L = _l.load()
    _chk(a, BF16, "a"); _chk(b, BF16, "b")
    a = a.contiguous(); b = b.contiguous()
    y = torch.empty_like(a)
    _l.check(L.st355_add(_stream(), _ptr(a), _ptr(b), _ptr(y), a.numel()), "add")
    return y


def gather_rows(x, idx, out=None):
    """out[b, j, :] = x[b, idx[b, j], :]; x [B, S, D] bf16 (last dim contiguous), idx [B, K] int32 -> [B, K, D]  (TREADRouter.start_route)"""
    L = _l.load()
    _dev(x, "x"); _dev(idx, "idx")
    if x.dtype != BF16 or x.dim() != 3 or x.stride(2) != 1 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise _l.St355Error("gather_rows: x [B, S, D] bf16 with contiguous rows, idx [B, K] contiguous int32")
    B, S, D = x.shape
    K = idx.shape[1]
    if out is None:
        out = torch.empty(B, K, D, dtype=BF16, device=x.device)
    _l.check(L.st355_gather_rows(_stream(), _ptr(x), x.stride(1), x.stride(0), _ptr(idx), _ptr(out), out.stride(1), out.stride(0), B, K, D), "gather_rows")
    return out


def scatter_rows(src, idx, dst):
    """dst[b, idx[b, j], :] = src[b, j, :] in place; src [B, K, D], dst [B, S, D] bf16, idx [B, K] int32  (TREADRouter.end_route)"""
    L = _l.load()
    _dev(src, "src"); _dev(dst, "dst"); _dev(idx, "idx")
    if src.dtype != BF16 or dst.dtype != BF16 or src.dim() != 3 or dst.dim() != 3 or src.stride(2) != 1 or dst.stride(2) != 1 or idx.dtype != torch.int32:
        raise _l.St355Error("scatter_rows: src [B, K, D] / dst [B, S, D] bf16 with contiguous rows, idx [B, K] int32")
    B, K, D = src.shape
    _l.check(L.st355_scatter_rows(_stream(), _ptr(src), src.stride(1), src.stride(0), _ptr(idx.contiguous()), _ptr(dst), dst.stride(1), dst.stride(0), B, K, D),
             "scatter_rows")
    return dst


def scale_cols(x, gate, rows_per_batch: int, out=None):
    """out[m,n] = x[m,n] * gate[m // rows_per_batch, n]"""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(gate, BF16, "gate")
    ldx = _rows(x, "x"); gs = _rows(gate, "gate")
    M, N = x.shape
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=x.device)
    _l.check(L.st355_scale_cols(_stream(), _ptr(x), ldx, _ptr(gate), gs, rows_per_batch, _ptr(out), _rows(out, "out"), M, N),
             "scale_cols")
    return out


# ------------------------------------------------------------------------------------------------
# GEMM family
# ------------------------------------------------------------------------------------------------
_GEMM_WS_BYTES = 512 << 20           # ONE size for every caller (r5 advice: a smaller first request made a later one re-allocate under captured graphs): the largest
                                     # user is the weight-gradient split-K (7 slices of a 6144 x 1536 gradient: 264 MB); the stream-K tail keeps up to 128 x 3 tile slabs (96 MiB)
_gemm_flags = {}


def _gemm_tile_flags(dev):
    """st355_gemm_args.tile_flags: 1024 arrival counters of the stream-K tail, zero once — every launch leaves them zero"""
    f = _gemm_flags.get(dev.index)
    if f is None:
        if torch.cuda.is_current_stream_capturing():
            raise _l.St355Error("the GEMM tile counters would be allocated inside a hipGraph capture: run one eager step first")
        f = torch.zeros(1024, dtype=torch.int32, device=dev)
        _gemm_flags[dev.index] = f
    return f


def _gemm_workspace(dev):
    """the shared scratch of the split-K paths (thin GEMMs, weight gradients) and the stream-K tail; its byte count is .numel()"""
    return _scratch("gemm", dev, _GEMM_WS_BYTES)


def qk_rope(Q, K, rrms, wq, wk, cos, sin, H: int, S: int, pos0: int, eps: float = 1e-6, Vt=None):
    """operands of the fused QKV projection epilogue (EPI_QK_NORM_ROPE; st355_qk_rope in st355.h): pass as gemm(..., rope=qk_rope(...)).
    Q, K: [B,H,S,128] bf16 outputs; rrms: [B*S, 2H] fp32 output; wq / wk: RMSNorm weights [128] or None; cos / sin: [S,64] fp32, one angle per
    interleaved channel pair (= full_table[:, 0::2])."""
    if cos.shape != (S, 64) or sin.shape != (S, 64) or not cos.is_contiguous() or not sin.is_contiguous():
        raise _l.St355Error(f"qk_rope: cos / sin must be contiguous [S={S}, 64] per-pair tables, got {tuple(cos.shape)}")
    _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(rrms, F32, "rrms"); _chk(cos, F32, "cos"); _chk(sin, F32, "sin")
    r = QkRope()
    r.Q, r.K, r.rrms, r.wq, r.wk, r.cos, r.sin = _ptr(Q), _ptr(K), _ptr(rrms), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin)
    r.H, r.S, r.pos0, r.eps = H, S, pos0, eps
    if Vt is not None:                  # also emit the head-major V^T [B,H,128,Sp] for attn_fwd (else: row-major V only, for attn_fwd_vrows)
        _chk(Vt, BF16, "Vt")
        r.Vt, r.Sp = _ptr(Vt), Vt.shape[-1]
    r._keep = (Q, K, rrms, wq, wk, cos, sin, Vt)
    return r


def heads(Q, K, Vt, H: int, S: int, pos0: int, n_q: int, n_k: int):
    """destinations of the head-splitting projection epilogue (EPI_HEADS; st355_heads in st355.h): pass as gemm(..., epilogue=EPI_HEADS, heads=heads(...),
    rows_per_batch=rows of this stream per sample).  Q / K: [B, H, S, 64] bf16 (None when the projection has no such part); Vt: [B, H, 64, Sp] or None."""
    h = Heads()
    for t, nm in ((Q, "Q"), (K, "K"), (Vt, "Vt")):
        if t is not None:
            _chk(t, BF16, nm)
            if not t.is_contiguous():
                raise _l.St355Error(f"heads: {nm} must be contiguous")
    h.Q, h.K, h.Vt = _ptr(Q), _ptr(K), _ptr(Vt)
    h.H, h.S, h.pos0, h.Sp, h.n_q, h.n_k = H, S, pos0, (Vt.shape[-1] if Vt is not None else 0), n_q, n_k
    h._keep = (Q, K, Vt)
    return h


def _gemm_args(g, a, w, bias=None, out=None, epilogue: int = EPI_NONE, a2=None, b2=None, aux_out=None, aux_in=None,
               gate=None, rows_per_batch: int = 0, k2_real: int = 0, rope=None, heads=None):
    """a, a2, out, aux_in, aux_out may be 3-D [segments, rows, cols] strided views (see _seg): one problem over the row blocks of a joint buffer.
    epilogue=EPI_QK_NORM_ROPE (rope=qk_rope(...), rows_per_batch=rows of this stream per sample): `out` is the V destination [M, N/3] (q / k go
    head-major to rope.Q / rope.K)."""
    _chk(a, BF16, "a"); _chk(w, BF16, "w")
    M, K, g.lda, seg, g.seg_a = _seg(a, "a")
    N, Kw = w.shape
    if K != Kw:
        raise _l.St355Error(f"gemm: K mismatch {K} vs {Kw}")
    if epilogue == EPI_QK_NORM_ROPE:
        if rope is None or out is None:
            raise _l.St355Error("gemm: EPI_QK_NORM_ROPE needs rope=qk_rope(...) and out= (the V destination)")
        g.rope = C.pointer(rope)
        g._rope_keep = rope
        g.rows_per_batch = rows_per_batch
    # output width: N, except the fused-QKV form (the V third), EPI_HEADS (the v heads), EPI_GEGLU (value * gelu(gate): N / 2) and EPI_GEGLU_GRAD (d value | d gate: 2 N)
    n_out = N // 3 if epilogue == EPI_QK_NORM_ROPE else N // 2 if epilogue == EPI_GEGLU else 2 * N if epilogue == EPI_GEGLU_GRAD else N
    if epilogue == EPI_HEADS:
        if heads is None:
            raise _l.St355Error("gemm: EPI_HEADS needs heads=heads(...)")
        n_out = N - heads.n_q - heads.n_k
        g.heads = C.pointer(heads)
        g._heads_keep = heads
        g.rows_per_batch = rows_per_batch
        if n_out == 0:                     # no v part (a q-only / k-only projection): C is never written — an [M, 8] scratch satisfies the argument checks
            if out is not None:
                raise _l.St355Error("gemm: EPI_HEADS without v heads takes no out=")
            n_out = 8
    if epilogue != EPI_QK_NORM_ROPE and out is None:
        out = torch.empty(M, n_out, dtype=BF16, device=a.device)
    Mo, No, g.ldc, sr, g.seg_c = _seg(out, "out")
    if (Mo, No) != (M, n_out):
        raise _l.St355Error(f"gemm: out is {Mo}x{No}, expected {M}x{n_out}")
    seg = _seg_join(seg, sr, "gemm")
    g.A, g.B, g.ldb, g.C = _ptr(a), _ptr(w), _rows(w, "w"), _ptr(out)
    g.M, g.N, g.K, g.K2 = M, N, K, 0
    if a2 is not None:
        _chk(a2, BF16, "a2"); _chk(b2, BF16, "b2")
        M2, K2, g.lda2, sr, g.seg_a2 = _seg(a2, "a2")
        seg = _seg_join(seg, sr, "gemm")
        if M2 != M or b2.shape[0] != N or K2 != b2.shape[1]:
            raise _l.St355Error("gemm: low-rank extension shape mismatch")
        g.A2 = _ptr(a2)
        g.B2, g.ldb2 = _ptr(b2), _rows(b2, "b2")
        g.K2 = K2
        g.K2_real = int(k2_real)          # adapter columns inside the 64-column granule (profiler accounting only)
    if bias is not None:
        _chk(bias, BF16, "bias")
        if not bias.is_contiguous():
            raise _l.St355Error("gemm: bias must be contiguous")
        g.bias = _ptr(bias)
    g.epilogue = epilogue
    if (N <= 128 and M >= 1024) or (M * N >= 128 * 65536 and epilogue <= EPI_ADD):       # thin problems (split-K slabs); 128+ tiles of 256x256 (stream-K tail)
        ws = _gemm_workspace(a.device)
        g.workspace, g.workspace_bytes = _ptr(ws), ws.numel()
        g.tile_flags = _ptr(_gemm_tile_flags(a.device))
    if aux_out is not None:
        _chk(aux_out, BF16, "aux_out")
        _, _, g.ld_aux_out, sr, g.seg_out = _seg(aux_out, "aux_out")
        seg = _seg_join(seg, sr, "gemm")
        g.aux_out = _ptr(aux_out)
    if aux_in is not None:
        _chk(aux_in, BF16, "aux_in")
        _, _, g.ld_aux_in, sr, g.seg_in = _seg(aux_in, "aux_in")
        seg = _seg_join(seg, sr, "gemm")
        g.aux_in = _ptr(aux_in)
    if gate is not None:
        _chk(gate, BF16, "gate")
        g.gate, g.gate_stride = _ptr(gate), _rows(gate, "gate")
        g.rows_per_batch = rows_per_batch
    g.seg_rows = seg
    return out


def gemm(a, w, **kw):
    """out[M,N] = a[M,K] @ w[N,K]^T (+ a2[M,K2] @ b2[N,K2]^T) with a fused epilogue (see st355.h).
    kwargs: bias, out, epilogue, a2, b2, aux_out, aux_in, gate, rows_per_batch."""
    L = _l.load()
    g = GemmArgs()
    out = _gemm_args(g, a, w, **kw)
    _l.check(L.st355_gemm_bf16(_stream(), C.byref(g)), "gemm_bf16")
    return out


def sum_chunks_bf16(chunks, world: int, out):
    """out[i] = bf16(sum_w float(chunks[w * n + i])), n = out.numel(): the fp32-accumulating local half of the all-to-all reduce-scatter (grad_sync)"""
    L = _l.load()
    _chk(chunks, BF16, "chunks"); _chk(out, BF16, "out")
    n = out.numel()
    if chunks.numel() != world * n:
        raise _l.St355Error(f"sum_chunks_bf16: chunks holds {chunks.numel()} elements, expected world * n = {world * n}")
    _l.check(L.st355_sum_chunks_bf16(_stream(), _ptr(chunks), int(world), int(n), _ptr(out)), "sum_chunks_bf16")
    return out


def geglu_interleave(w, bias=None):
    """the feed-forward projection's rows (nn.Linear.weight [2F, K] = [value rows | gate rows]) in the order the EPI_GEGLU / EPI_GEGLU_GRAD epilogues contract
    them: every 64 rows = 32 value features followed by the 32 gate features of the SAME indices (st355.h).  Returns (w_il, bias_il); built once for frozen weights."""
    N2, K = w.shape
    F_ = N2 // 2
    if N2 % 64 or F_ % 32:
        raise _l.St355Error(f"geglu_interleave: 2F = {N2} must be a multiple of 64")
    wi = torch.stack([w[:F_].view(F_ // 32, 32, K), w[F_:].view(F_ // 32, 32, K)], dim=1).reshape(N2, K).contiguous()
    bi = None if bias is None else torch.stack([bias[:F_].view(F_ // 32, 32), bias[F_:].view(F_ // 32, 32)], dim=1).reshape(N2).contiguous()
    return wi, bi


def gemm_set_tail_split(mode: int) -> int:
    """st355_gemm_set_tail_split: 1 = stream-K tail where it applies (default), 0 = the uncut schedules, -1 = environment; returns the previous mode"""
    return int(_l.load().st355_gemm_set_tail_split(int(mode)))


def gemm_tail_placement() -> int:
    """st355_gemm_tail_placement: 0 = the XCD placement probe has not run on this device, 1 = round-robin confirmed (stream-K tail in use), 2 = not confirmed"""
    return int(_l.load().st355_gemm_tail_placement())


def gemm_set_persistent(mode: int) -> int:
    """st355_gemm_set_persistent: 1 = persistent tile walk (k_gemm_pz) where it applies, 0 = one tile per workgroup, -1 = default; returns the previous mode"""
    return int(_l.load().st355_gemm_set_persistent(int(mode)))


def attn_set_impl(fwd: int = -1, dq: int = -1, dkv: int = -1):
    """st355_attn_set_impl: fwd / dq 64 = the hand-scheduled 64-rows-per-wave kernels where they apply (default), 32 = the 32-row kernels everywhere;
    dkv 4 = the hand-scheduled dK/dV body (default), 3 = k_attn_bwd_dkv3; -1 = unchanged.  Returns the previous (fwd, dq, dkv)."""
    prev = int(_l.load().st355_attn_set_impl(int(fwd), int(dq), int(dkv)))
    return prev // 65536, (prev // 256) % 256, prev % 256


def attn_set_ds(mode: int = -1) -> int:
    """st355_attn_set_ds: the dS-spill attention backward (head_dim 128): 0 = never (the recompute kernels: A/B switch), 1 = wherever it is built, whatever the size
    (tests), -1 = the library's size gate (default).  Returns the previous mode."""
    return int(_l.load().st355_attn_set_ds(int(mode)))


ATTN_ROUTE_KINDS = {10: "fwd64", 20: "fwd4", 30: "fwd4_bias", 40: "fwd4_res", 50: "fwd4_res_bias", 60: "fwd4_vrows", 70: "fwd4_vrows_bias",
                    100: "prep", 110: "prep_res", 120: "prep_dot", 130: "prep_res_dot",
                    200: "dkv4", 210: "dkv4_rope", 220: "dkv3", 230: "dkv3_rope", 240: "dkv2",
                    300: "dq64", 310: "dq64_rope", 320: "dq_tr", 330: "dq_tr_bias", 340: "dq", 350: "dq_bias", 360: "dq_tr_rope",
                    370: "dq_tr_bias_rope", 250: "dkv4_ds", 260: "dkv4_rope_ds", 380: "dq_ds", 390: "dq_ds_rope"}      # ST355_ATTN_ROUTE_* (st355.h) + 0 / 1 / 2 for head_dim 64 / 96 / 128
ATTN_PLAN_FLAGS = {"key_bias": 1, "vrows": 2, "O_res": 4, "Qt": 8, "Kt": 16, "rope": 32, "ds": 64}


def attn_route_name(route: int) -> str:
    kind, hd = route // 10 * 10, route % 10
    return f"{ATTN_ROUTE_KINDS[kind]}<{(64, 96, 128)[hd]}>"


def attn_plan(B, H, Sq, Sk, d, key_bias=False, vrows=False, O_res=False, Qt=False, Kt=False, rope=False, ds=False):
    """st355_attn_plan: the kernels a forward + backward of this shape would run on now, without launching anything.  The keyword arguments say what the calls
    are given (truthy: present; ds: a large-enough dS^T spill buffer).  Returns {"fwd", "prep", "dkv", "dq": route names such as "dq64<128>", "dq_tail": bool}."""
    flags = 0
    for k, v in (("key_bias", key_bias), ("vrows", vrows), ("O_res", O_res), ("Qt", Qt), ("Kt", Kt), ("rope", rope), ("ds", ds)):
        if v is not None and v is not False:
            flags |= ATTN_PLAN_FLAGS[k]
    routes = (C.c_int32 * 5)()
    _l.check(_l.load().st355_attn_plan(int(B), int(H), int(Sq), int(Sk), int(d), flags, routes), "attn_plan")
    return {"fwd": attn_route_name(routes[0]), "prep": attn_route_name(routes[1]), "dkv": attn_route_name(routes[2]), "dq": attn_route_name(routes[3]),
            "dq_tail": bool(routes[4])}


def gemm_grouped(problems):
    """run several independent GEMMs that share one epilogue kind in as few launches as possible.
    problems: list of dicts with keys a, w and the kwargs of gemm().  Returns the list of outputs."""
    L = _l.load()
    arr = (GemmArgs * len(problems))()
    outs = []
    for g, pr in zip(arr, problems):
        pr = dict(pr)
        outs.append(_gemm_args(g, pr.pop("a"), pr.pop("w"), **pr))
    _l.check(L.st355_gemm_bf16_grouped(_stream(), arr, len(problems)), "gemm_bf16_grouped")
    return outs


GEMM_ROUTES = {1: "ROWS", 2: "THIN", 3: "SPLITK", 4: "S2", 5: "P3", 6: "PQ", 7: "PZ", 8: "PQ_TAIL", 9: "PQ_QK_ROPE", 10: "PQ_HEADS", 11: "PQ_GEGLU",
               12: "PZ_GEGLU_GRAD", 13: "PAIR_PQ", 14: "PAIR_P3", 15: "PAIR_HEADS", 16: "PAIR_QK_ROPE"}      # ST355_ROUTE_* (st355.h)


def gemm_plan(problems):
    """st355_gemm_plan: the schedule (a GEMM_ROUTES name) each problem would run on as gemm_grouped(problems) — for one problem, as gemm(**problems[0]) — without
    launching anything.  Same dicts as gemm_grouped; outputs not given are allocated as there (and not written)."""
    L = _l.load()
    arr = (GemmArgs * len(problems))()
    keep = []
    for g, pr in zip(arr, problems):
        pr = dict(pr)
        keep.append(_gemm_args(g, pr.pop("a"), pr.pop("w"), **pr))
    routes = (C.c_int32 * len(problems))()
    _l.check(L.st355_gemm_plan(arr, len(problems), routes), "gemm_plan")
    return [GEMM_ROUTES[r] for r in routes]


def fp8_quantize_weight(w):
    """quantize_weight_to_fp8 (fp8_native.py:25-30): returns (q uint8 [N,K] holding e4m3fn bytes, scale fp32 [N])"""
    L = _l.load()
    _chk(w, BF16, "w")
    N, K = w.shape
    q = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=F32, device=w.device)
    _l.check(L.st355_fp8_quantize_weight(_stream(), _ptr(w), _rows(w, "w"), _ptr(q), _ptr(scale), N, K), "fp8_quantize_weight")
    return q, scale


def fp8_quantize_act(x):
    """per-call e5m2 quantisation of the activations (fp8_native.py:58-60): returns (q uint8 [M,K], scale_a fp32 [1] = 1/input_scale)"""
    L = _l.load()
    _chk(x, BF16, "x")
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    scale_a = torch.empty(1, dtype=F32, device=x.device)
    ws = torch.empty(1, dtype=torch.int32, device=x.device)
    _l.check(L.st355_fp8_quantize_act(_stream(), _ptr(x), _rows(x, "x"), _ptr(q), _ptr(scale_a), M, K, _ptr(ws)), "fp8_quantize_act")
    return q, scale_a


def linear_fp8(xq, scale_a, wq, w_scale, bias=None, out=None):
    """out = (xq wq^T) * scale_a * w_scale[n] + bias  -> bf16   (torch._scaled_mm with row-wise scales, fp8_native.py:64-75)"""
    L = _l.load()
    for t, nm in ((xq, "xq"), (wq, "wq")):
        _dev(t, nm)
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise _l.St355Error(f"linear_fp8: {nm} must be a contiguous uint8 (fp8 bytes) tensor")
    _chk(scale_a, F32, "scale_a"); _chk(w_scale, F32, "w_scale")
    M, K = xq.shape
    N = wq.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=xq.device)
    if bias is not None:
        _chk(bias, BF16, "bias")
    _l.check(L.st355_linear_fp8(_stream(), _ptr(xq), K, _ptr(scale_a), _ptr(wq), K, _ptr(w_scale), _ptr(bias), _ptr(out), _rows(out, "out"),
                                M, N, K), "linear_fp8")
    return out


def _tn_operand(t, name: str):
    """a TN operand: 2-D [M, C] (row stride free) or a 3-D [B, rows, C] view of a joint buffer (row stride ld, segment stride a multiple of it):
    -> (pointer tensor, ld, logical rows M, C, seg_rows or 0, physical segment stride in rows or 0)"""
    _chk(t, BF16, name)
    if t.dim() == 2:
        return t, _rows(t, name), t.shape[0], t.shape[1], 0, 0
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) <= 0 or t.stride(0) % t.stride(1) != 0:
        raise _l.St355Error(f"gemm_tn: {name} must be [M, C] or a [B, rows, C] view whose batch stride is a whole number of rows")
    B, rows, Cn = t.shape
    return t, t.stride(1), B * rows, Cn, rows, t.stride(0) // t.stride(1)


def gemm_tn(Lm, R, out=None, accumulate: bool = False):
    """out[P,Q] (+)= Lm[M,P]^T @ R[M,Q]  — the weight-gradient form (dW = dY^T X).  M must be a multiple of 64 (zero-padded rows).  Either operand may be a
    3-D [B, rows, C] strided view (a stream's rows of a joint buffer, rows a multiple of 64): contracted in place (st355_gemm_tn_seg_bf16)."""
    L = _l.load()
    Lm, ldl, M, P, seg_a, str_a = _tn_operand(Lm, "L")
    R, ldr, M2, Q, seg_b, str_b = _tn_operand(R, "R")
    if M2 != M:
        raise _l.St355Error("gemm_tn: operands must share the contraction length")
    if out is None:
        if accumulate:
            raise _l.St355Error("gemm_tn: accumulate needs an output tensor")
        out = torch.empty(P, Q, dtype=BF16, device=Lm.device)
    _chk(out, BF16, "out")
    ws = _gemm_workspace(Lm.device)                     # fp32 split-K slabs: up to 7 slices of a 6144 x 1536 gradient (264 MB)
    if seg_a or seg_b:
        seg = seg_a or seg_b
        if seg_a and seg_b and seg_a != seg_b:
            raise _l.St355Error("gemm_tn: two segmented operands must share the segment length")
        _l.check(L.st355_gemm_tn_seg_bf16(_stream(), _ptr(Lm), ldl, str_a if seg_a else 0, _ptr(R), ldr, str_b if seg_b else 0, _ptr(out), _rows(out, "out"),
                                          M, seg, P, Q, 1 if accumulate else 0, _ptr(ws), ws.numel()), "gemm_tn_seg_bf16")
        return out
    _l.check(L.st355_gemm_tn_bf16(_stream(), _ptr(Lm), ldl, _ptr(R), ldr, _ptr(out), _rows(out, "out"), M, P, Q,
                                  1 if accumulate else 0, _ptr(ws), ws.numel()), "gemm_tn_bf16")
    return out


def colsum_prod(a, out, b=None, rows_per_batch: Optional[int] = None, mode: int = 0, prev=None, shift=None, scale=None, accumulate: bool = False):
    """out[bi, :] (+)= sum over the rows of batch bi of a (* b).  out: fp32 2-D view [nb, N] (row stride free).  mode 1: see st355.h."""
    L = _l.load()
    _chk(a, BF16, "a"); _chk(out, F32, "out")
    rows, N = a.shape
    rpb = rows if rows_per_batch is None else rows_per_batch
    if b is not None:
        _chk(b, BF16, "b")
    ws = _scratch("colsum", a.device, L.st355_colsum_workspace(rows, N, rpb))
    ms = 0
    if mode == 1:
        _chk(shift, BF16, "shift"); _chk(scale, BF16, "scale"); _chk(prev, F32, "prev")
        ms = _rows(shift, "shift")
        if _rows(scale, "scale") != ms:
            raise _l.St355Error("colsum_prod: shift and scale must share a row stride")
    _l.check(L.st355_colsum_prod(_stream(), _ptr(a), _rows(a, "a"), _ptr(b), _rows(b, "b") if b is not None else 0, rows, N, rpb, _ptr(out),
                                 _rows(out, "out"), mode, _ptr(prev), _rows(prev, "prev") if prev is not None else 0, _ptr(shift), _ptr(scale),
                                 ms, 1 if accumulate else 0, _ptr(ws)), "colsum_prod")
    return out


def stat_out(out, reduce_batches: bool = False, accumulate: bool = False):
    """st355_stat_out of a destination tensor: fp32 2-D view [nb, N] (per-batch rows, row stride free) or — reduce_batches — one fp32 / bf16 row [N]"""
    o = _l.StatOut()
    if out is None:
        return o
    if out.dtype not in (F32, BF16) or (out.dtype == BF16 and not reduce_batches):
        raise _l.St355Error("stat_out: per-batch sums are fp32; a bf16 destination is one row summed over the batches")
    _dev(out, "stat_out")
    o.out, o.stride = out.data_ptr(), (0 if reduce_batches else _rows(out, "stat_out"))
    o.reduce_batches, o.out_bf16, o.accumulate = int(reduce_batches), int(out.dtype == BF16), int(accumulate)
    o._keep = out
    return o


def ln_modulate_bwd_stats(dy, x, scale, rows_per_batch: int, d_shift, d_scale, dres=None, gate=None, y_branch=None, d_gate=None, d_bias=None, eps: float = 1e-6,
                          want_gated: bool = False, out=None):
    """ln_modulate_bwd + the sums autograd accumulates around the AdaLN instance (st355_ln_modulate_bwd_stats): d_shift / d_scale fp32 [nb, D] views,
    d_gate = sum dx * y_branch (fp32 [nb, D]), d_bias = sum gate * dx over all rows (one fp32 / bf16 row).  Returns (dx, dxg)."""
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x"); _chk(scale, BF16, "scale")
    rows, D = x.shape
    dx = torch.empty(rows, D, dtype=BF16, device=x.device) if out is None else out
    dxg = torch.empty(rows, D, dtype=BF16, device=x.device) if want_gated else None
    ws = _scratch("stats", x.device, L.st355_stats_workspace(rows, D, rows_per_batch, 4))
    outs = [stat_out(d_shift), stat_out(d_scale), stat_out(d_gate), stat_out(d_bias, reduce_batches=True)]
    _l.check(L.st355_ln_modulate_bwd_stats(_stream(), _ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(scale), _rows(scale, "scale"), rows_per_batch,
                                           _ptr(dres), _rows(dres, "dres") if dres is not None else 0, _ptr(gate) if want_gated else None,
                                           _rows(gate, "gate") if want_gated else 0, _ptr(dx), _rows(dx, "dx"), _ptr(dxg), D, rows, D, eps,
                                           _ptr(y_branch), _rows(y_branch, "y_branch") if y_branch is not None else 0,
                                           C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]), _ptr(ws)), "ln_modulate_bwd_stats")
    return dx, dxg


def scale_cols_stats(x, gate, rows_per_batch: int, y_branch=None, d_gate=None, d_bias=None, out=None):
    """scale_cols + d_gate = sum_t x * y_branch (fp32 [nb, N]) + d_bias = sum over all rows of the output (one fp32 / bf16 row)"""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(gate, BF16, "gate")
    M, N = x.shape
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=x.device)
    ws = _scratch("stats", x.device, L.st355_stats_workspace(M, N, rows_per_batch, 2))
    og, ob = stat_out(d_gate), stat_out(d_bias, reduce_batches=True)
    _l.check(L.st355_scale_cols_stats(_stream(), _ptr(x), _rows(x, "x"), _ptr(gate), _rows(gate, "gate"), rows_per_batch, _ptr(out), _rows(out, "out"), M, N,
                                      _ptr(y_branch), _rows(y_branch, "y_branch") if y_branch is not None else 0, C.byref(og), C.byref(ob), _ptr(ws)),
             "scale_cols_stats")
    return out


def colsum_rows(a, rows_per_batch: int, batch_stride_rows: int, nb: int, out, per_batch: bool = False, accumulate: bool = False):
    """column sums of nb row blocks of `a` (block b = rows [b * batch_stride_rows, + rows_per_batch) of the 2-D tensor a, in place): one row over all blocks
    (fp32 / bf16 [N]) or per-block fp32 rows [nb, N]"""
    L = _l.load()
    _chk(a, BF16, "a")
    N = a.shape[1]
    ws = _scratch("stats", a.device, L.st355_stats_workspace(nb * rows_per_batch, N, rows_per_batch, 1))
    o = stat_out(out, reduce_batches=not per_batch, accumulate=accumulate)
    _l.check(L.st355_colsum_rows(_stream(), _ptr(a), _rows(a, "a"), rows_per_batch, batch_stride_rows, nb, N, C.byref(o), _ptr(ws)), "colsum_rows")
    return out


def transpose(src, out=None):
    """out[c, r] = src[r, c] (bf16)"""
    L = _l.load()
    _chk(src, BF16, "src")
    R, Cn = src.shape
    if out is None:
        out = torch.empty(Cn, R, dtype=BF16, device=src.device)
    _chk(out, BF16, "out")
    _l.check(L.st355_transpose_bf16(_stream(), _ptr(src), _rows(src, "src"), _ptr(out), _rows(out, "out"), R, Cn), "transpose_bf16")
    return out


def _skinny_scratch(dev, M: int, P: int, R: int):
    """the split-M partials of skinny_tn / skinny_tn_multi and of the Flux backward blocks: one scratch per device (see _scratch)"""
    return _scratch("skinny", dev, _l.load().st355_skinny_tn_workspace(M, P, R))


def skinny_plan(M: int, P: int, seg_rows: int = 0):
    """st355_skinny_plan: the split-M plan skinny_tn / skinny_tn_multi would launch for this shape ({"mc": rows per workgroup, "nchunks": partials the
    reduce sums}), from the launchers' own chunk choice, without launching anything"""
    out = (C.c_int32 * 2)()
    _l.check(_l.load().st355_skinny_plan(int(M), int(P), int(seg_rows), out), "skinny_plan")
    return {"mc": int(out[0]), "nchunks": int(out[1])}


def skinny_tn(Lm, R, out, so_p: int, so_r: int, r_used: int, alpha: float = 1.0, accumulate: bool = False):
    """out[p*so_p + r*so_r] (+)= alpha * sum_m Lm[m,p] * R[m,r]   (fp32 out; rank-space LoRA gradients).  Lm / R may be 3-D segmented views (_seg)."""
    L = _l.load()
    _chk(Lm, BF16, "L"); _chk(R, BF16, "R"); _chk(out, F32, "out")
    M, P, ldl, seg, seg_l = _seg(Lm, "L")
    Mr, Rn, ldr, sr, seg_r = _seg(R, "R")
    if Mr != M:
        raise _l.St355Error(f"skinny_tn: L has {M} rows, R has {Mr}")
    seg = _seg_join(seg, sr, "skinny_tn")
    ws = _skinny_scratch(Lm.device, M, P, Rn)
    _l.check(L.st355_skinny_tn_seg(_stream(), _ptr(Lm), ldl, _ptr(R), ldr, _ptr(out), so_p, so_r, M, P, Rn,
                                   r_used, alpha, 1 if accumulate else 0, _ptr(ws), seg, seg_l, seg_r), "skinny_tn")
    return out


def skinny_tn_multi(Lm, R, outs, so_p: int, so_r: int, r_used: int, alpha: float = 1.0, accumulate: bool = False):
    """outs[g][p*so_p + r*so_r] (+)= alpha * sum_m Lm[m,p] * R[m, 32 g + r] for the len(outs) <= 4 adapters that share Lm: ONE pass over Lm (R: [M, >= 128])."""
    L = _l.load()
    _chk(Lm, BF16, "L"); _chk(R, BF16, "R")
    M, P, ldl, seg, seg_l = _seg(Lm, "L")
    Mr, Rn, ldr, sr, seg_r = _seg(R, "R")
    if Mr != M or Rn < 128 or not (1 <= len(outs) <= 4):
        raise _l.St355Error(f"skinny_tn_multi: L has {M} rows, R {Mr} x {Rn} (needs 128 columns), {len(outs)} outputs (1..4)")
    seg = _seg_join(seg, sr, "skinny_tn_multi")
    for o in outs:
        _chk(o, F32, "out")
    ws = _skinny_scratch(Lm.device, M, P, 128)
    arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    _l.check(L.st355_skinny_tn_multi(_stream(), _ptr(Lm), ldl, _ptr(R), ldr, arr, len(outs), so_p, so_r, M, P, r_used, alpha, 1 if accumulate else 0,
                                     _ptr(ws), seg, seg_l, seg_r), "skinny_tn_multi")
    return outs


# ------------------------------------------------------------------------------------------------
# LoRA dropout (csrc/lora_dropout.hip; st355_lora_drop in include/st355.h): the mask is regenerated from (key, call, stream, row, col), never stored
# ------------------------------------------------------------------------------------------------
def lora_dropout_threshold(p: float) -> int:
    """T = round(p * 65536): an element is dropped iff its 16-bit lane < T, so the realised probability is p' = T / 65536 (0 < p < 1 is built)"""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"lora_dropout must lie in [0, 1), got {p}")
    T = int(round(p * 65536.0))
    if not 1 <= T <= 65535:
        raise ValueError(f"lora_dropout={p} rounds to the threshold {T} / 65536: outside the 16-bit lanes of the mask generator")
    return T


def _drop_struct(drop, streams, name: str):
    """`drop`: the component's dropout state — .thr (lora_dropout_threshold), .key0 / .key1 (32-bit words of the Philox key), .call (ONE int32 on the device, read
    as uint32).  streams: the stream ids of the 1 .. 4 targets."""
    if not 1 <= len(streams) <= 4:
        raise _l.St355Error(f"{name}: 1 .. 4 targets share one input (got {len(streams)})")
    call = drop.call
    _chk(call, torch.int32, "call")
    if call.numel() != 1:
        raise _l.St355Error(f"{name}: the call counter is ONE int32 on the device")
    st = _l.LoraDrop()
    st.key0, st.key1, st.threshold = int(drop.key0) & 0xFFFFFFFF, int(drop.key1) & 0xFFFFFFFF, int(drop.thr)
    st.scale = 1.0 / (1.0 - int(drop.thr) / 65536.0)
    st.call = call.data_ptr()
    for i in range(4):
        st.streams[i] = int(streams[min(i, len(streams) - 1)]) & 0xFFFFFFFF
    return st


def _drop_rows(t, name: str):
    """(M, cols, ld, seg_rows, seg_stride_rows) of a masked operand: 2-D row-major or a [B, rows, C] view (_seg); K % 8 and 16-byte rows are what one Philox
    group per 16-byte chunk needs"""
    M, K, ld, seg, seg_s = _seg(t, name)
    if K % 8 or ld % 8 or t.data_ptr() % 16:
        raise _l.St355Error(f"{name}: LoRA dropout needs K % 8 == 0 and 16-byte aligned rows (the mask is drawn per group of 8 input columns; got K = {K}, "
                            f"row stride {ld})")
    return M, K, ld, seg, seg_s


def lora_dropout_advance(call):
    """*call += 1: a one-thread launch that belongs to the step (a captured step advances the counter on the device)"""
    _chk(call, torch.int32, "call")
    _l.check(_l.load().st355_lora_dropout_advance(_stream(), _ptr(call)), "lora_dropout_advance")
    return call


def lora_dropout_mask(M: int, K: int, drop, stream: int):
    """the keep bits of (key, call, stream) over an [M, K] input as uint8 (tests and tools; never on the step)"""
    if K % 8 or M <= 0:
        raise _l.St355Error(f"lora_dropout_mask: K must be a multiple of 8 (got {K})")
    out = torch.empty(M, K, dtype=torch.uint8, device=drop.call.device)
    st = _drop_struct(drop, [stream], "lora_dropout_mask")
    _l.check(_l.load().st355_lora_dropout_mask(_stream(), _ptr(out), M, K, C.byref(st)), "lora_dropout_mask")
    return out


def lora_down_drop(x, A_cat, r_pad: int, streams, drop, out=None):
    """T[m, g r_pad + r] = scale sum_k keep_g(m,k) x[m,k] A_cat[g r_pad + r, k] for the len(streams) targets of a group in ONE pass over x (bf16 T [M, K2], one
    rounding; the K-extension consumes it as it does the unmasked product)"""
    _chk(x, BF16, "x"); _chk(A_cat, BF16, "A_cat")
    M, K, ldx, seg, seg_s = _drop_rows(x, "lora_down_drop: x")
    K2 = A_cat.shape[0]
    if A_cat.dim() != 2 or A_cat.shape[1] != K or not A_cat.is_contiguous():
        raise _l.St355Error(f"lora_down_drop: expected contiguous A_cat [K2, {K}], got {tuple(A_cat.shape)}")
    if r_pad not in (32, 64, 128) or len(streams) * r_pad > K2:
        raise _l.St355Error(f"lora_down_drop: r_pad must be 32, 64 or 128 and the targets' columns fit K2 (got r_pad {r_pad}, {len(streams)} targets, K2 {K2})")
    if out is None:
        out = torch.empty(M, K2, dtype=BF16, device=x.device)
    _chk(out, BF16, "out")
    if tuple(out.shape) != (M, K2):
        raise _l.St355Error(f"lora_down_drop: expected out [{M}, {K2}], got {tuple(out.shape)}")
    st = _drop_struct(drop, streams, "lora_down_drop")
    _l.check(_l.load().st355_lora_down_drop(_stream(), _ptr(x), ldx, seg, seg_s, _ptr(A_cat), _ptr(out), _rows(out, "out"), M, K, len(streams), r_pad, K2,
                                            C.byref(st)), "lora_down_drop")
    return out


def lora_dx_drop(dx, U, A_cat_T, r_pad: int, streams, drop):
    """dx[m, k] += scale sum_g keep_g(m,k) sum_r U[m, g r_pad + r] A_cat_T[k, g r_pad + r], in place into a bf16 tensor or [B, rows, C] view (one rounding): the
    adapter term of a projection's input gradient, which the mask keeps off the K-extension of the dx GEMM"""
    _chk(dx, BF16, "dx"); _chk(U, BF16, "U"); _chk(A_cat_T, BF16, "A_cat_T")
    M, K, ldd, seg, seg_s = _drop_rows(dx, "lora_dx_drop: dx")
    K2 = A_cat_T.shape[1]
    if A_cat_T.dim() != 2 or A_cat_T.shape[0] != K or not A_cat_T.is_contiguous():
        raise _l.St355Error(f"lora_dx_drop: expected contiguous A_cat_T [{K}, K2], got {tuple(A_cat_T.shape)}")
    if U.dim() != 2 or tuple(U.shape) != (M, K2) or U.data_ptr() % 16:
        raise _l.St355Error(f"lora_dx_drop: expected U [{M}, {K2}], got {tuple(U.shape)}")
    if r_pad not in (32, 64, 128) or len(streams) * r_pad > K2:
        raise _l.St355Error(f"lora_dx_drop: r_pad must be 32, 64 or 128 and the targets' columns fit K2 (got r_pad {r_pad}, {len(streams)} targets, K2 {K2})")
    st = _drop_struct(drop, streams, "lora_dx_drop")
    _l.check(_l.load().st355_lora_dx_drop(_stream(), _ptr(dx), ldd, seg, seg_s, _ptr(U), _rows(U, "U"), _ptr(A_cat_T), M, K, len(streams), r_pad, K2, C.byref(st)),
             "lora_dx_drop")
    return dx


_TS_KINDS = {F32: 0, BF16: 1, torch.int64: 2}          # ST355_TS_*


def tlora_mask(t, r_pad: int, rank: int, G: int, rows_per_sample: int, ranks_table, timesteps):
    """T-LoRA (csrc/tlora.hip): zeroes, in place, column g r_pad + j of row m of the rank-space operand t (bf16 [M, >= G r_pad] or a [B, rows, C] view) iff
    j >= ranks_table[clamp(trunc(timesteps[m // rows_per_sample]), 0, T)], for g < G and j < rank.  timesteps: [B] on the device, fp32 / bf16 / int64;
    ranks_table: int32 [T + 1] on the device.  Nothing is read on the host."""
    _chk(t, BF16, "tlora_mask: t"); _chk(ranks_table, torch.int32, "tlora_mask: ranks_table"); _dev(timesteps, "tlora_mask: timesteps")
    M, cols, ld, seg, seg_s = _seg(t, "tlora_mask: t")
    if timesteps.dtype not in _TS_KINDS or timesteps.dim() != 1 or not timesteps.is_contiguous():
        raise _l.St355Error(f"tlora_mask: timesteps must be a contiguous [B] tensor of fp32 / bf16 / int64, got {timesteps.dtype} {tuple(timesteps.shape)}")
    if ranks_table.dim() != 1 or not ranks_table.is_contiguous() or ranks_table.numel() < 2:
        raise _l.St355Error(f"tlora_mask: ranks_table must be a contiguous int32 [T + 1], got {tuple(ranks_table.shape)}")
    if cols < G * r_pad:
        raise _l.St355Error(f"tlora_mask: {G} targets of {r_pad} columns do not fit the operand's {cols} columns")
    _l.check(_l.load().st355_tlora_mask(_stream(), _ptr(t), ld, seg, seg_s, M, int(rows_per_sample), int(G), int(r_pad), int(rank), _ptr(timesteps),
                                        _TS_KINDS[timesteps.dtype], timesteps.numel(), _ptr(ranks_table), ranks_table.numel() - 1), "tlora_mask")
    return t


def skinny_tn_drop(Lm, R, out, so_p: int, so_r: int, r_used: int, stream: int, drop, alpha: float = 1.0, accumulate: bool = False):
    """skinny_tn with the LoRA-dropout mask of `stream` on Lm (the Linear's input): out[p*so_p + r*so_r] (+)= alpha scale sum_m keep(m,p) Lm[m,p] R[m,r]"""
    L = _l.load()
    _chk(Lm, BF16, "L"); _chk(R, BF16, "R"); _chk(out, F32, "out")
    M, P, ldl, seg, seg_l = _drop_rows(Lm, "skinny_tn_drop: L")
    Mr, Rn, ldr, sr, seg_r = _seg(R, "R")
    if Mr != M:
        raise _l.St355Error(f"skinny_tn_drop: L has {M} rows, R has {Mr}")
    seg = _seg_join(seg, sr, "skinny_tn_drop")
    ws = _skinny_scratch(Lm.device, M, P, Rn)
    st = _drop_struct(drop, [stream], "skinny_tn_drop")
    _l.check(L.st355_skinny_tn_drop(_stream(), _ptr(Lm), ldl, _ptr(R), ldr, _ptr(out), so_p, so_r, M, P, Rn, r_used, alpha, 1 if accumulate else 0, _ptr(ws),
                                    seg, seg_l, seg_r, C.byref(st)), "skinny_tn_drop")
    return out


def skinny_tn_drop_multi(Lm, R, outs, so_p: int, so_r: int, r_used: int, streams, drop, alpha: float = 1.0, accumulate: bool = False):
    """skinny_tn_multi with target g's mask (streams[g]) on Lm for column block g of R: the q / k / v adapters' dA in ONE pass over Lm"""
    L = _l.load()
    _chk(Lm, BF16, "L"); _chk(R, BF16, "R")
    M, P, ldl, seg, seg_l = _drop_rows(Lm, "skinny_tn_drop_multi: L")
    Mr, Rn, ldr, sr, seg_r = _seg(R, "R")
    if Mr != M or Rn < 128 or not (1 <= len(outs) <= 4) or len(streams) != len(outs):
        raise _l.St355Error(f"skinny_tn_drop_multi: L has {M} rows, R {Mr} x {Rn} (needs 128 columns), {len(outs)} outputs (1..4), {len(streams)} streams")
    seg = _seg_join(seg, sr, "skinny_tn_drop_multi")
    for o in outs:
        _chk(o, F32, "out")
    ws = _skinny_scratch(Lm.device, M, P, 128)
    arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    st = _drop_struct(drop, streams, "skinny_tn_drop_multi")
    _l.check(L.st355_skinny_tn_drop_multi(_stream(), _ptr(Lm), ldl, _ptr(R), ldr, arr, len(outs), so_p, so_r, M, P, r_used, alpha, 1 if accumulate else 0,
                                          _ptr(ws), seg, seg_l, seg_r, C.byref(st)), "skinny_tn_drop_multi")
    return outs


# ------------------------------------------------------------------------------------------------
# DoRA (csrc/dora.hip): the row scale g = m / ||W + s B A|| folded into the GEMM operands once per forward, dm and the row-scaled dB of the backward
# ------------------------------------------------------------------------------------------------
def dora_fold(W, A_cat_T, B_blk, m, targets, r_pad: int, inv_norm, g, Wf, WfT, Bf, BfT, init: bool = False):
    """One adapter group (st355_dora_fold): from the frozen W [N, K] and the packed bf16 operands the forward multiplies with (A_cat_T [K, K2], B_blk [N, K2], which
    carries s) write inv_norm / g [N] fp32 (g = m / ||W + s B A||_row; init: m = the norm is written first, g = 1 exactly), Wf = bf16(g . W), WfT its transpose,
    Bf = bf16(g . B_blk), BfT its transpose.  targets: [(n_off, N)] of the 1 .. 4 targets, rising; target i owns slab i of the K-extension."""
    for t, nm in ((W, "W"), (A_cat_T, "A_cat_T"), (B_blk, "B_blk"), (Wf, "Wf"), (WfT, "WfT"), (Bf, "Bf"), (BfT, "BfT")):
        _chk(t, BF16, nm)
    for t, nm in ((m, "m"), (inv_norm, "inv_norm"), (g, "g")):
        _chk(t, F32, nm)
    if W.dim() != 2:
        raise _l.St355Error(f"dora_fold: expected W [N, K], got {tuple(W.shape)}")
    N, K = W.shape
    K2 = B_blk.shape[1] if B_blk.dim() == 2 else -1
    if tuple(A_cat_T.shape) != (K, K2) or tuple(B_blk.shape) != (N, K2) or tuple(Wf.shape) != (N, K) or tuple(WfT.shape) != (K, N) or tuple(Bf.shape) != (N, K2) \
            or tuple(BfT.shape) != (K2, N) or any(t.numel() != N for t in (m, inv_norm, g)) \
            or not all(t.is_contiguous() for t in (W, A_cat_T, B_blk, m, inv_norm, g, Wf, WfT, Bf, BfT)):
        raise _l.St355Error(f"dora_fold: expected contiguous W [N, K], A_cat_T [K, K2], B_blk [N, K2], m / inv_norm / g [N], Wf [N, K], WfT [K, N], Bf [N, K2], BfT [K2, N] "
                            f"(N = {N}, K = {K}, K2 = {K2})")
    G = len(targets)
    if not 1 <= G <= 4:
        raise _l.St355Error(f"dora_fold: 1 .. 4 targets per group (got {G})")
    n_off = (C.c_int32 * G)(*[int(o) for o, _ in targets])
    n_cnt = (C.c_int32 * G)(*[int(n) for _, n in targets])
    _l.check(_l.load().st355_dora_fold(_stream(), _ptr(W), _ptr(A_cat_T), _ptr(B_blk), _ptr(m), 1 if init else 0, _ptr(inv_norm), _ptr(g), _ptr(Wf), _ptr(WfT), _ptr(Bf),
                                       _ptr(BfT), N, K, K2, G, n_off, n_cnt, int(r_pad)), "dora_fold")
    return g


def dora_y0_scratch(dev, M: int, N: int):
    """[M, N] bf16 over the DoRA backward's scratch (the recomputed y0 = x W^T + s (x A^T) B^T of one adapted Linear; consumed by dora_dmag right away)"""
    return _scratch("dora_y0", dev, 2 * M * N)[:2 * M * N].view(BF16).view(M, N)


def dora_db_scratch(dev, N: int, rank: int):
    """[N, rank] fp32 over the DoRA backward's second scratch (the unscaled s dy^T T of one target, consumed by dora_db_finish right away)"""
    return _scratch("dora_db", dev, 4 * N * rank)[:4 * N * rank].view(F32).view(N, rank)


def dora_dmag(dy, y0, inv_norm, dm, accumulate: bool = False):
    """dm[n] (+)= inv_norm[n] sum_rows dy[row, n] y0[row, n] (st355_dora_dmag).  dy: compact [M, N] bf16 or a [B, rows, N] view of a joint buffer; y0 [M, N] bf16;
    two-stage fixed-order reduction over 256-row chunks of the LOGICAL rows: a view and its compact copy give the same bits."""
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(y0, BF16, "y0"); _chk(inv_norm, F32, "inv_norm"); _chk(dm, F32, "dm")
    M, N, ldd, seg, seg_s = _seg(dy, "dora_dmag: dy")
    if y0.dim() != 2 or tuple(y0.shape) != (M, N) or inv_norm.numel() != N or dm.numel() != N or not (inv_norm.is_contiguous() and dm.is_contiguous()):
        raise _l.St355Error(f"dora_dmag: expected y0 [{M}, {N}], contiguous inv_norm / dm [{N}]")
    ldy = _rows(y0, "dora_dmag: y0")
    if N % 8 or ldd % 8 or ldy % 8 or dy.data_ptr() % 16 or y0.data_ptr() % 16:
        raise _l.St355Error(f"dora_dmag: N and the row strides must be multiples of 8, the operands 16-byte aligned (N = {N}, strides {ldd} / {ldy})")
    ws = _scratch("dora_dmag", dy.device, L.st355_dora_dmag_workspace(M, N))
    _l.check(L.st355_dora_dmag(_stream(), _ptr(dy), ldd, seg, seg_s, _ptr(y0), ldy, _ptr(inv_norm), _ptr(dm), M, N, 1 if accumulate else 0, _ptr(ws)), "dora_dmag")
    return dm


def dora_db_finish(P, g, gB, accumulate: bool = False):
    """gB[n, :] (+)= g[n] P[n, :] (st355_dora_db_finish): P [N, rank] fp32 = s dy^T T from skinny_tn (accumulate=False), g [N] fp32, gB [N, rank] fp32"""
    _chk(P, F32, "P"); _chk(g, F32, "g"); _chk(gB, F32, "gB")
    if P.dim() != 2 or P.shape != gB.shape or g.numel() != P.shape[0] or not (P.is_contiguous() and gB.is_contiguous() and g.is_contiguous()):
        raise _l.St355Error(f"dora_db_finish: expected contiguous P / gB [N, rank] and g [N], got {tuple(P.shape)}, {tuple(gB.shape)}, {tuple(g.shape)}")
    _l.check(_l.load().st355_dora_db_finish(_stream(), _ptr(P), _ptr(g), _ptr(gB), P.shape[0], P.shape[1], 1 if accumulate else 0), "dora_db_finish")
    return gB


# ------------------------------------------------------------------------------------------------
# LyCORIS LoKr (csrc/lokr.hip): dW = s kron(w1, w2) folded into the GEMM operands once per forward; the structured gradients of w1 / w2 in the backward
# ------------------------------------------------------------------------------------------------
def lokr_fold(W, targets, s: float, Wf, WfT):
    """One fused projection (st355_lokr_fold): Wf = bf16(W + s kron(w1, w2)) on every target's row slab, WfT its transpose, and the bf16 copy of every w2.
    targets: 1 .. 4 of (n_off, N, w1 [ol, im] fp32, w2 [ok, in] fp32, w2b [ok, in] bf16) in rising row order; rows outside every target are copied."""
    for t, nm in ((W, "W"), (Wf, "Wf"), (WfT, "WfT")):
        _chk(t, BF16, nm)
    if W.dim() != 2:
        raise _l.St355Error(f"lokr_fold: expected W [N, K], got {tuple(W.shape)}")
    N, K = W.shape
    if not (W.is_contiguous() and Wf.is_contiguous() and WfT.is_contiguous()) or tuple(Wf.shape) != (N, K) or tuple(WfT.shape) != (K, N):
        raise _l.St355Error(f"lokr_fold: expected contiguous W / Wf [N, K] and WfT [K, N], got {tuple(W.shape)}, {tuple(Wf.shape)}, {tuple(WfT.shape)}")
    G = len(targets)
    if not 1 <= G <= 4:
        raise _l.St355Error(f"lokr_fold: 1 .. 4 targets per projection (got {G})")
    i32a, vpa = C.c_int32 * G, C.c_void_p * G
    n_off, n_cnt, ol, im, p1, p2, pb = i32a(), i32a(), i32a(), i32a(), vpa(), vpa(), vpa()
    for g, (off, n, w1, w2, w2b) in enumerate(targets):
        _chk(w1, F32, "w1"); _chk(w2, F32, "w2"); _chk(w2b, BF16, "w2b")
        if w1.dim() != 2 or w2.dim() != 2 or not (w1.is_contiguous() and w2.is_contiguous() and w2b.is_contiguous()) or w2b.shape != w2.shape \
                or w1.shape[0] * w2.shape[0] != n or w1.shape[1] * w2.shape[1] != K:
            raise _l.St355Error(f"lokr_fold: target {g}: expected contiguous w1 [ol, im], w2 / w2b [ok, in] with ol * ok = {n} and im * in = {K}, got "
                                f"{tuple(w1.shape)}, {tuple(w2.shape)}, {tuple(w2b.shape)}")
        n_off[g], n_cnt[g], ol[g], im[g], p1[g], p2[g], pb[g] = int(off), int(n), w1.shape[0], w1.shape[1], w1.data_ptr(), w2.data_ptr(), w2b.data_ptr()
    _l.check(_l.load().st355_lokr_fold(_stream(), _ptr(W), _ptr(Wf), _ptr(WfT), N, K, G, n_off, n_cnt, ol, im, p1, p2, pb, float(s)), "lokr_fold")
    return Wf


def lokr_scratch(which: str, dev, M: int, cols: int):
    """[M, cols] bf16 over one of the LoKr backward's scratch buffers ("dp": the mixed gradient, "p": x.view(M im, in) w2^T; each consumed right away)"""
    return _scratch("lokr_" + which, dev, 2 * M * cols)[:2 * M * cols].view(BF16).view(M, cols)


def lokr_mix(dy, n_off: int, w1, ok: int, out):
    """out[m, j ok + k] = bf16(sum_i w1[i, j] dy[m, n_off + i ok + k]) (st355_lokr_mix).  dy: compact [M, C] bf16 or a [B, rows, C] view of a joint buffer;
    w1 [ol, im] fp32; out [M, im ok] bf16 contiguous."""
    _chk(dy, BF16, "lokr_mix: dy"); _chk(w1, F32, "lokr_mix: w1"); _chk(out, BF16, "lokr_mix: out")
    M, Cn, ldd, seg, seg_s = _seg(dy, "lokr_mix: dy")
    if w1.dim() != 2 or not w1.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != (M, w1.shape[1] * ok) or n_off + w1.shape[0] * ok > Cn:
        raise _l.St355Error(f"lokr_mix: expected contiguous w1 [ol, im] and out [{M}, im * {ok}], the slab inside dy's {Cn} columns; got {tuple(w1.shape)}, "
                            f"{tuple(out.shape)}, n_off {n_off}")
    _l.check(_l.load().st355_lokr_mix(_stream(), _ptr(dy), ldd, seg, seg_s, int(n_off), _ptr(w1), w1.shape[0], w1.shape[1], int(ok), _ptr(out), M), "lokr_mix")
    return out


def lokr_dw2(dP, x, im: int, out, alpha: float = 1.0, accumulate: bool = False):
    """out[ok, in] (+)= alpha dP.view(M im, ok)^T x.view(M im, in) (st355_lokr_dw2).  dP [M, im ok] bf16 contiguous; x: compact [M, im in] bf16 or a
    [B, rows, im in] view of a joint buffer; out fp32 contiguous."""
    L = _l.load()
    _chk(dP, BF16, "lokr_dw2: dP"); _chk(x, BF16, "lokr_dw2: x"); _chk(out, F32, "lokr_dw2: out")
    M, K, ldx, seg, seg_s = _seg(x, "lokr_dw2: x")
    if out.dim() != 2 or not out.is_contiguous() or not dP.is_contiguous() or dP.dim() != 2:
        raise _l.St355Error("lokr_dw2: expected contiguous dP [M, im * ok] and out [ok, in]")
    ok, in_ = out.shape
    if tuple(dP.shape) != (M, im * ok) or K != im * in_:
        raise _l.St355Error(f"lokr_dw2: expected dP [{M}, {im * ok}] and x with {im * in_} columns, got {tuple(dP.shape)} and {K}")
    ws = _scratch("lokr_dw2", x.device, L.st355_lokr_dw2_workspace(M * im, ok, in_))
    _l.check(L.st355_lokr_dw2(_stream(), _ptr(dP), _ptr(x), ldx, seg, seg_s, int(im), _ptr(out), M, ok, in_, float(alpha), 1 if accumulate else 0, _ptr(ws)), "lokr_dw2")
    return out


def lokr_dw1(dy, n_off: int, P, out, ok: int, alpha: float = 1.0, accumulate: bool = False):
    """out[i, j] (+)= alpha sum_{m, k} dy[m, n_off + i ok + k] P[m, j ok + k] (st355_lokr_dw1).  dy as for lokr_mix; P [M, im ok] bf16 contiguous; out [ol, im] fp32."""
    L = _l.load()
    _chk(dy, BF16, "lokr_dw1: dy"); _chk(P, BF16, "lokr_dw1: P"); _chk(out, F32, "lokr_dw1: out")
    M, Cn, ldd, seg, seg_s = _seg(dy, "lokr_dw1: dy")
    if out.dim() != 2 or not out.is_contiguous() or not P.is_contiguous() or tuple(P.shape) != (M, out.shape[1] * ok) or n_off + out.shape[0] * ok > Cn:
        raise _l.St355Error(f"lokr_dw1: expected contiguous out [ol, im] and P [{M}, im * {ok}], the slab inside dy's {Cn} columns; got {tuple(out.shape)}, "
                            f"{tuple(P.shape)}, n_off {n_off}")
    ws = _scratch("lokr_dw1", dy.device, L.st355_lokr_dw1_workspace(M))
    _l.check(L.st355_lokr_dw1(_stream(), _ptr(dy), ldd, seg, seg_s, int(n_off), _ptr(P), _ptr(out), M, out.shape[0], out.shape[1], int(ok), float(alpha),
                              1 if accumulate else 0, _ptr(ws)), "lokr_dw1")
    return out


# ------------------------------------------------------------------------------------------------
# AdaLN / RMSNorm + RoPE
# ------------------------------------------------------------------------------------------------
def ln_modulate_fwd(x, scale, shift, rows_per_batch: int, eps: float = 1e-6, out=None):
    """y = LN(x) * (1 + scale[b]) + shift[b]; scale/shift are [B, D] views sharing one row stride."""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(scale, BF16, "scale"); _chk(shift, BF16, "shift")
    rows, D = x.shape
    ms = _rows(scale, "scale")
    if _rows(shift, "shift") != ms:
        raise _l.St355Error("ln_modulate_fwd: scale and shift must share a row stride")
    if out is None:
        out = torch.empty(rows, D, dtype=BF16, device=x.device)
    _l.check(L.st355_ln_modulate_fwd(_stream(), _ptr(x), _rows(x, "x"), _ptr(scale), _ptr(shift), ms, rows_per_batch,
                                     _ptr(out), _rows(out, "out"), rows, D, eps), "ln_modulate_fwd")
    return out


_zero_rows = {}


def layer_norm_xhat(x, eps: float = 1e-6, out=None):
    """xhat = LN(x) with no modulation (ln_modulate_fwd with scale = shift = 0): the factor of the modulation-SCALE gradient, d scale_b = sum_t dY * xhat.
    The engines compute that sum from xhat itself; recovering xhat from the saved modulated output as (n - shift) / (1 + scale) (colsum_prod mode 1) is
    singular where a scale entry is exactly -1 in bf16 — which random-init modulation tables hit in a few entries per step."""
    _chk(x, BF16, "x")
    key = (str(x.device), x.shape[1])
    z = _zero_rows.get(key)
    if z is None:
        z = _zero_rows[key] = torch.zeros(1, x.shape[1], dtype=BF16, device=x.device)
    return ln_modulate_fwd(x, z, z, x.shape[0], eps=eps, out=out)


def ln_modulate_bwd(dy, x, scale, rows_per_batch: int, dres=None, gate=None, eps: float = 1e-6, want_gated: bool = False, out=None):
    """dx = dres + LNbwd(dy*(1+scale));  dxg = gate[b]*dx (if want_gated).  Returns (dx, dxg).  out: optional destination view for dx (row stride free)."""
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x"); _chk(scale, BF16, "scale")
    rows, D = x.shape
    dx = torch.empty(rows, D, dtype=BF16, device=x.device) if out is None else out
    if out is not None:
        _chk(out, BF16, "out")
        if tuple(out.shape) != (rows, D):
            raise _l.St355Error("ln_modulate_bwd: out shape mismatch")
    dxg = torch.empty(rows, D, dtype=BF16, device=x.device) if want_gated else None
    if dres is not None:
        _chk(dres, BF16, "dres")
    if want_gated:
        _chk(gate, BF16, "gate")
    _l.check(L.st355_ln_modulate_bwd(_stream(), _ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(scale), _rows(scale, "scale"),
                                     rows_per_batch, _ptr(dres), _rows(dres, "dres") if dres is not None else 0,
                                     _ptr(gate) if want_gated else None, _rows(gate, "gate") if want_gated else 0,
                                     _ptr(dx), _rows(dx, "dx"), _ptr(dxg), D, rows, D, eps), "ln_modulate_bwd")
    return dx, dxg


def qk_norm_rope_fwd(qkv, wq, wk, cos, sin, Q, K, Qt, Kt, Vt, B, H, d, S_part, pos0, S, Sp, eps: float = 1e-6):
    L = _l.load()
    _chk(qkv, BF16, "qkv"); _chk(cos, F32, "cos"); _chk(sin, F32, "sin")
    _l.check(L.st355_qk_norm_rope_fwd(_stream(), _ptr(qkv), _rows(qkv, "qkv"), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin),
                                      _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(Vt), B, H, d, S_part, pos0, S, Sp, eps),
             "qk_norm_rope_fwd")


def qk_norm_rope_bwd(dQ, dK, qkv, wq, wk, cos, sin, dqkv, B, H, d, S_part, pos0, S, eps: float = 1e-6):
    L = _l.load()
    _chk(dQ, BF16, "dQ"); _chk(dK, BF16, "dK"); _chk(qkv, BF16, "qkv"); _chk(dqkv, BF16, "dqkv")
    _l.check(L.st355_qk_norm_rope_bwd(_stream(), _ptr(dQ), _ptr(dK), _ptr(qkv), _rows(qkv, "qkv"), _ptr(wq), _ptr(wk),
                                      _ptr(cos), _ptr(sin), _ptr(dqkv), _rows(dqkv, "dqkv"), B, H, d, S_part, pos0, S, eps),
             "qk_norm_rope_bwd")


def qk_norm_rope_bwd_wgrad(dQ, dK, qkv, wq, wk, cos, sin, dqkv, B, H, d, S_part, pos0, S, gwq, gwk, accumulate: bool = False, eps: float = 1e-6):
    """qk_norm_rope_bwd + d loss / d (norm_q.weight, norm_k.weight) into the bf16 [d] views gwq / gwk (None: absent / frozen)"""
    L = _l.load()
    _chk(dQ, BF16, "dQ"); _chk(dK, BF16, "dK"); _chk(qkv, BF16, "qkv"); _chk(dqkv, BF16, "dqkv")
    for g in (gwq, gwk):
        if g is not None:
            _chk(g, BF16, "gw")
    ws = _scratch("qk_norm_wgrad", dQ.device, L.st355_qk_norm_wgrad_workspace(B, H, d, S_part))
    _l.check(L.st355_qk_norm_rope_bwd_wgrad(_stream(), _ptr(dQ), _ptr(dK), _ptr(qkv), _rows(qkv, "qkv"), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin),
                                            _ptr(dqkv), _rows(dqkv, "dqkv"), B, H, d, S_part, pos0, S, eps, _ptr(gwq), _ptr(gwk),
                                            1 if accumulate else 0, _ptr(ws)), "qk_norm_rope_bwd_wgrad")


def qk_rope_norm_bwd(dQ, dK, Q, K, rrms, wq, wk, cos, sin, dqkv, B, H, d, S_part, pos0, S):
    """backward of the fused projection epilogue: from the roped head-major Q / K and the saved 1/rms (no pre-norm projection kept)"""
    L = _l.load()
    _chk(dQ, BF16, "dQ"); _chk(dK, BF16, "dK"); _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(rrms, F32, "rrms"); _chk(dqkv, BF16, "dqkv")
    _l.check(L.st355_qk_rope_norm_bwd(_stream(), _ptr(dQ), _ptr(dK), _ptr(Q), _ptr(K), _ptr(rrms), _ptr(wq), _ptr(wk), _ptr(cos), _ptr(sin),
                                      _ptr(dqkv), _rows(dqkv, "dqkv"), B, H, d, S_part, pos0, S), "qk_rope_norm_bwd")


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _res_ok(O, O_res):
    _chk(O_res, BF16, "O_res")
    if O_res.shape != O.shape or _rows(O_res, "O_res") != _rows(O, "O"):
        raise _l.St355Error("attention: O_res must have O's shape and row stride")


def attn_fwd(Q, K, Vt, O, lse2, B, H, S, Sp, d, scale: float, key_bias=None, O_res=None):
    """O: 2-D token-major view [B*S, >=H*d]; lse2 [B,H,S] fp32.  O_res (same layout): also write the rounding residual bf16(O_fp32 - O) for attn_bwd(O_res=...)."""
    L = _l.load()
    _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(Vt, BF16, "Vt"); _chk(O, BF16, "O"); _chk(lse2, F32, "lse2")
    if O_res is not None:
        _res_ok(O, O_res)
        _l.check(L.st355_attn_fwd_res(_stream(), _ptr(Q), _ptr(K), _ptr(Vt), _ptr(key_bias), _ptr(O), _rows(O, "O"), _ptr(O_res), _ptr(lse2),
                                      B, H, S, S, Sp, d, scale), "attn_fwd_res")
        return
    _l.check(L.st355_attn_fwd(_stream(), _ptr(Q), _ptr(K), _ptr(Vt), _ptr(key_bias), _ptr(O), _rows(O, "O"), _ptr(lse2),
                              B, H, S, Sp, d, scale), "attn_fwd")


def attn_fwd_vrows(Q, K, v_rows, O, lse2, B, H, S, d, scale: float, key_bias=None):
    """attn_fwd with V row-major: v_rows is a 2-D token-major view [B*S, >= H*d] (head h at columns h*d); no V^T copy.  d = 128."""
    L = _l.load()
    _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(v_rows, BF16, "v_rows"); _chk(O, BF16, "O"); _chk(lse2, F32, "lse2")
    _l.check(L.st355_attn_fwd_vrows(_stream(), _ptr(Q), _ptr(K), _ptr(v_rows), _rows(v_rows, "v_rows"), _ptr(key_bias), _ptr(O), _rows(O, "O"),
                                    _ptr(lse2), B, H, S, d, scale), "attn_fwd_vrows")


def _attn_bwd_scratch(dev, B, H, S, Sp, d):
    """the partials of the attention backward: one scratch per device, shared by attn_bwd, attn_bwd_rope, attn_cross_bwd and the block backward entry points"""
    return _scratch("attn_bwd", dev, _l.load().st355_attn_bwd_workspace(B, H, S, Sp, d))


def attn_ds_scratch(dev, B, H, S, Sp, d, key_bias=None, rope=False):
    """the dS^T spill buffer of the attention backward — allocated only where the library would take the spill route with one (st355_attn_plan decides; elsewhere
    None: today's kernels run); one scratch per device under the retire-and-refuse rule of _scratch"""
    if d != 128 or key_bias is not None or Sp != S:
        return None
    if not attn_plan(B, H, S, S, d, rope=rope, ds=True)["dq"].startswith("dq_ds"):
        return None
    return _scratch("attn_bwd_ds", dev, _l.load().st355_attn_bwd_ds_bytes(B, H, S, Sp, S, d))


def attn_ds_bytes(ds) -> int:
    return 0 if ds is None else ds.numel() * ds.element_size()


# ST355_ATTN_TR=0: the engines build head-major Q^T / K^T copies and the backward reads them (dkv2 / dq); default: no copies, transposing LDS reads
ATTN_TR = os.environ.get("ST355_ATTN_TR", "1") != "0"


def attn_bwd(Q, K, Qt, Kt, v_rows, O, dO, lse2, dQ, dK, dv_rows, B, H, S, Sp, d, scale: float, key_bias=None, O_res=None, ds=None, ds_bytes=None):
    """ds (a uint8 device tensor; ds_bytes: what the call is told it holds, default all of it): the caller's dS^T spill buffer -> st355_attn_bwd_ds"""
    L = _l.load()
    ws = _attn_bwd_scratch(Q.device, B, H, S, Sp, d)
    if ds is not None:
        _l.check(L.st355_attn_bwd_ds(_stream(), _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(v_rows), _rows(v_rows, "v_rows"),
                                     _ptr(O), _rows(O, "O"), _ptr(dO), _rows(dO, "dO"), _ptr(lse2), _ptr(key_bias),
                                     _ptr(dQ), _ptr(dK), _ptr(dv_rows), _rows(dv_rows, "dv_rows"), B, H, S, Sp, d, scale, _ptr(ws), _ptr(ds),
                                     attn_ds_bytes(ds) if ds_bytes is None else int(ds_bytes)), "attn_bwd_ds")
        return
    if O_res is not None:          # delta = rowsum(dO * (O + O_res))
        _res_ok(O, O_res)
        _l.check(L.st355_attn_bwd_res(_stream(), _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(v_rows), _rows(v_rows, "v_rows"),
                                      _ptr(O), _rows(O, "O"), _ptr(O_res), _ptr(dO), _rows(dO, "dO"), _ptr(lse2), _ptr(key_bias),
                                      _ptr(dQ), _ptr(dK), _ptr(dv_rows), _rows(dv_rows, "dv_rows"), B, H, S, Sp, S, Sp, d, scale, _ptr(ws)), "attn_bwd_res")
        return
    _l.check(L.st355_attn_bwd(_stream(), _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(v_rows), _rows(v_rows, "v_rows"),
                              _ptr(O), _rows(O, "O"), _ptr(dO), _rows(dO, "dO"), _ptr(lse2), _ptr(key_bias),
                              _ptr(dQ), _ptr(dK), _ptr(dv_rows), _rows(dv_rows, "dv_rows"), B, H, S, Sp, d, scale, _ptr(ws)),
             "attn_bwd")


def attn_bwd_rope(Q, K, v_rows, O, dO, lse2, rrms, wq_lo, wk_lo, wq_hi, wk_hi, split: int, cos_p, sin_p, dqkv, B, H, S, Sp, d, scale: float, key_bias=None,
                  ds=None, ds_bytes=None):
    """attention backward with the RoPE + RMSNorm backward fused into the dQ / dK epilogues (head_dim 128, after a fused QKV projection): dq, dk, dv are
    written straight into the rows of the projection gradient dqkv [B*S, >= 3*H*d]; joint positions < split use the *_lo norm weights.
    ds / ds_bytes: a dS^T spill buffer of the caller's (as attn_bwd); None: the shared scratch where the library would take the spill route."""
    L = _l.load()
    _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(rrms, F32, "rrms"); _chk(dqkv, BF16, "dqkv"); _chk(cos_p, F32, "cos_p"); _chk(sin_p, F32, "sin_p")
    ws = _attn_bwd_scratch(Q.device, B, H, S, Sp, d)
    if ds is None:
        ds = attn_ds_scratch(Q.device, B, H, S, Sp, d, key_bias, rope=True)
    if ds is not None:
        _l.check(L.st355_attn_bwd_rope_ds(_stream(), _ptr(Q), _ptr(K), _ptr(v_rows), _rows(v_rows, "v_rows"), _ptr(O), _rows(O, "O"), _ptr(dO), _rows(dO, "dO"),
                                          _ptr(lse2), _ptr(key_bias), _ptr(rrms), _ptr(wq_lo), _ptr(wk_lo), _ptr(wq_hi), _ptr(wk_hi), split, _ptr(cos_p), _ptr(sin_p),
                                          _ptr(dqkv), _rows(dqkv, "dqkv"), B, H, S, Sp, d, scale, _ptr(ws), _ptr(ds),
                                          attn_ds_bytes(ds) if ds_bytes is None else int(ds_bytes)), "attn_bwd_rope_ds")
        return
    _l.check(L.st355_attn_bwd_rope(_stream(), _ptr(Q), _ptr(K), _ptr(v_rows), _rows(v_rows, "v_rows"), _ptr(O), _rows(O, "O"), _ptr(dO), _rows(dO, "dO"),
                                   _ptr(lse2), _ptr(key_bias), _ptr(rrms), _ptr(wq_lo), _ptr(wk_lo), _ptr(wq_hi), _ptr(wk_hi), split, _ptr(cos_p), _ptr(sin_p),
                                   _ptr(dqkv), _rows(dqkv, "dqkv"), B, H, S, Sp, d, scale, _ptr(ws)), "attn_bwd_rope")


# ------------------------------------------------------------------------------------------------
# optimiser / EMA
# ------------------------------------------------------------------------------------------------
def adamw_ema_step(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2,
                   grad_scale: float = 1.0, ema=None, ema_decay: float = 0.0, p_bf16=None):
    L = _l.load()
    if p.dtype == F32:
        for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
            _chk(t, F32, n)
        _l.check(L.st355_adamw_ema_step(_stream(), _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), _ptr(p_bf16), p.numel(),
                                        lr, beta1, beta2, eps, weight_decay, step, grad_scale, ema_decay), "adamw_ema_step")
    else:
        _chk(p, BF16, "p"); _chk(g, BF16, "g"); _chk(m, F32, "m"); _chk(v, F32, "v")
        _l.check(L.st355_adamw_ema_step_bf16(_stream(), _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(),
                                             lr, beta1, beta2, eps, weight_decay, step, grad_scale, ema_decay),
                 "adamw_ema_step_bf16")


def lion_step(p, g, m, lr: float, beta1=0.9, beta2=0.99, weight_decay=0.0, grad_scale: float = 1.0, comp=None, ema=None,
              ema_decay: float = 0.0, p_bf16=None):
    """Lion over a flat arena (st355_lion_step*): fp32 p / g / m (optional fp32 ema, bf16 copy p_bf16), or bf16 p / g / m with an optional bf16 Kahan
    compensation buffer `comp` (and bf16 ema)"""
    L = _l.load()
    if p.dtype == F32:
        for t, n in ((p, "p"), (g, "g"), (m, "m")):
            _chk(t, F32, n)
        if comp is not None:
            raise _l.St355Error("lion_step: an fp32 arena takes no compensation buffer")
        if ema is not None:
            _chk(ema, F32, "ema")
        if p_bf16 is not None:
            _chk(p_bf16, BF16, "p_bf16")
        if any(t is not None and (t.numel() != p.numel() or not t.is_contiguous()) for t in (p, g, m, ema, p_bf16)):
            raise _l.St355Error("lion_step: every arena must be contiguous and have p's length")
        _l.check(L.st355_lion_step(_stream(), _ptr(p), _ptr(g), _ptr(m), _ptr(ema), _ptr(p_bf16), p.numel(),
                                   lr, beta1, beta2, weight_decay, grad_scale, ema_decay), "lion_step")
    else:
        for t, n in ((p, "p"), (g, "g"), (m, "m")):
            _chk(t, BF16, n)
        if p_bf16 is not None:
            raise _l.St355Error("lion_step: p_bf16 belongs to the fp32 arena")
        for t, n in ((comp, "comp"), (ema, "ema")):
            if t is not None:
                _chk(t, BF16, n)
        if any(t is not None and (t.numel() != p.numel() or not t.is_contiguous()) for t in (p, g, m, comp, ema)):
            raise _l.St355Error("lion_step: every arena must be contiguous and have p's length")
        _l.check(L.st355_lion_step_bf16(_stream(), _ptr(p), _ptr(g), _ptr(m), _ptr(comp), _ptr(ema), p.numel(),
                                        lr, beta1, beta2, weight_decay, grad_scale, ema_decay), "lion_step_bf16")


def ema_update(shadow, param, decay: float):
    L = _l.load()
    if shadow.dtype != param.dtype:
        raise _l.St355Error("ema_update: dtype mismatch")
    _l.check(L.st355_ema_update(_stream(), _ptr(shadow), _ptr(param), shadow.numel(), decay, shadow.element_size()), "ema_update")


def grad_norm(g):
    """returns fp32 [2] device tensor: (sum of squares, max |g|).  The per-block partials live in a scratch of this (device, stream): norms on different streams
    (a side-stream EMA / ControlNet norm, a hipGraph capture next to eager calls) never share one"""
    L = _l.load()
    out = torch.empty(2, dtype=F32, device=g.device)
    st = _stream()
    ws = _scratch("grad_norm", g.device, 2 * 1024 * 4, key=(st,))          # 2 x 1024 fp32 partials
    _l.check(L.st355_grad_norm_ws(st, _ptr(g), g.numel(), g.element_size(), _ptr(out), _ptr(ws)), "grad_norm")
    return out


def grad_clamp_(g, c: float):
    """in place: g <- clamp(g, -c, c) (clip_grad_value_)"""
    L = _l.load()
    _dev(g, "g")
    if g.dtype not in (F32, BF16) or not g.is_contiguous():
        raise _l.St355Error("grad_clamp: expected a contiguous fp32 / bf16 tensor")
    _l.check(L.st355_grad_clamp(_stream(), _ptr(g), g.numel(), g.element_size(), float(c)), "grad_clamp")
    return g


def grad_clip_norm_(g, stats, max_norm: float, pre_scale: float = 1.0):
    """in place: g *= min(1, max_norm / (sqrt(stats[0]) * pre_scale + 1e-6)); stats = grad_norm(g) (device, never read on the host)"""
    L = _l.load()
    _dev(g, "g"); _chk(stats, F32, "stats")
    if g.dtype not in (F32, BF16) or not g.is_contiguous():
        raise _l.St355Error("grad_clip_norm: expected a contiguous fp32 / bf16 tensor")
    _l.check(L.st355_grad_clip_norm(_stream(), _ptr(g), g.numel(), g.element_size(), _ptr(stats), float(max_norm), float(pre_scale)), "grad_clip_norm")
    return g


class MuonPlan:
    """st355_muon_plan for a fixed list of matrices of one fp32 arena (element offsets, shapes): the host plan, its device copy and the
    workspace, all made once here — the step itself then allocates nothing and never syncs"""

    HEADER, RECORD = 8, 16

    def __init__(self, offsets, shapes, device):
        n = len(shapes)
        if n == 0 or len(offsets) != n:
            raise _l.St355Error("muon_plan: expected one offset per matrix shape")
        L = _l.load()
        off = (C.c_int64 * n)(*[int(o) for o in offsets])
        rows = (C.c_int32 * n)(*[int(s[0]) for s in shapes])
        cols = (C.c_int32 * n)(*[int(s[1]) for s in shapes])
        self.host = torch.zeros(self.HEADER + self.RECORD * n, dtype=torch.int64)
        ws = C.c_int64(0)
        _l.check(L.st355_muon_plan(off, rows, cols, n, _ptr(self.host), C.byref(ws)), "muon_plan")
        self.n = n
        self.ws_floats = int(ws.value)
        self.dev = self.host.to(device)
        self.ws = torch.empty(self.ws_floats, dtype=F32, device=device)

    def launches(self, ns_steps: int) -> int:
        """kernel launches of one call: prep + norm + (gram, poly, update) per iteration and per short-side class present"""
        rp = self.host[self.HEADER:].view(self.n, self.RECORD)[:, 5]
        return 2 + 3 * ns_steps * len(set(rp.tolist()))


def _coeffs(coeffs):
    flat = [float(v) for abc in coeffs for v in abc]
    if not flat or len(flat) % 3:
        raise _l.St355Error("muon: coefficients must be a list of (a, b, c) triples, one per iteration")
    return (C.c_float * len(flat))(*flat), len(flat) // 3


def muon_step(plan: MuonPlan, p, g, m, coeffs, lr: float, momentum: float = 0.95, weight_decay: float = 0.1, eps: float = 1e-7,
              rms_scale_factor: float = 0.2, grad_scale: float = 1.0):
    """one Muon step over the arena (p, g, m: fp32 flat, plan offsets into them): momentum, Newton-Schulz with one (a, b, c) per iteration,
    scale, decoupled decay, apply — in place on p and m"""
    L = _l.load()
    for t, nm in ((p, "p"), (g, "g"), (m, "m")):
        _chk(t, F32, nm)
        if not t.is_contiguous() or t.numel() != p.numel():
            raise _l.St355Error(f"muon_step: {nm} must be a contiguous fp32 arena of {p.numel()} elements")
    cf, ns = _coeffs(coeffs)
    _l.check(L.st355_muon_step(_stream(), _ptr(plan.host), _ptr(plan.dev), _ptr(p), _ptr(g), _ptr(m), _ptr(plan.ws), plan.ws_floats,
                               float(grad_scale), float(momentum), float(lr), float(weight_decay), float(eps), float(rms_scale_factor), ns, cf),
             "muon_step")


def muon_orthogonalize(plan: MuonPlan, x, coeffs, normalize: bool = True, eps: float = 1e-7, out=None):
    """the bare orthogonalisation of every matrix of the arena x (fp32 flat): out = NS(x) (x / max(||x||_F, eps) first if normalize)"""
    L = _l.load()
    _chk(x, F32, "x")
    if not x.is_contiguous():
        raise _l.St355Error("muon_orthogonalize: x must be contiguous")
    out = torch.zeros_like(x) if out is None else out
    _chk(out, F32, "out")
    cf, ns = _coeffs(coeffs)
    _l.check(L.st355_muon_orthogonalize(_stream(), _ptr(plan.host), _ptr(plan.dev), _ptr(x), _ptr(out), _ptr(plan.ws), plan.ws_floats,
                                        int(bool(normalize)), float(eps), ns, cf), "muon_orthogonalize")
    return out


class SoapPlan:
    """st355_soap_plan for a fixed list of matrices of one fp32 arena (element offsets, shapes): the host plan, its device copy and the workspace,
    made once.  `qq` is the length of the GG / Q arenas (sum of r^2, r = a matrix's short side), `rr` the sum of r; `q_offsets[i]`, `short[i]`
    place matrix i's r x r block in them"""

    HEADER, RECORD = 8, 12

    def __init__(self, offsets, shapes, device):
        n = len(shapes)
        if n == 0 or len(offsets) != n:
            raise _l.St355Error("soap_plan: expected one offset per matrix shape")
        L = _l.load()
        off = (C.c_int64 * n)(*[int(o) for o in offsets])
        rows = (C.c_int32 * n)(*[int(s[0]) for s in shapes])
        cols = (C.c_int32 * n)(*[int(s[1]) for s in shapes])
        self.host = torch.zeros(self.HEADER + self.RECORD * n, dtype=torch.int64)
        ws = C.c_int64(0)
        _l.check(L.st355_soap_plan(off, rows, cols, n, _ptr(self.host), C.byref(ws)), "soap_plan")
        self.n = n
        self.ws_floats = int(ws.value)
        self.qq, self.rr = int(self.host[3]), int(self.host[4])
        rec = self.host[self.HEADER:].view(n, self.RECORD)
        self.short = rec[:, 1].tolist()
        self.q_offsets = rec[:, 8].tolist()
        self.r_offsets = rec[:, 10].tolist()
        self.idx_offsets = rec[:, 9].tolist()
        self.dev = self.host.to(device)
        self.ws = torch.zeros(self.ws_floats, dtype=F32, device=device)

    def launches(self, first: bool = False, refresh: bool = False) -> int:
        """kernel launches of one call: the step (or the Gram pass) per short-side class present, the fold, then the eigensolver on the first call or
        the refresh and one permutation per class"""
        ncls = len(set(self.host[self.HEADER:].view(self.n, self.RECORD)[:, 3].tolist()))
        return ncls + 1 + (1 if first else (1 + ncls if refresh else 0))

    def sort_index(self, i: int):
        """the index the last refresh sorted matrix i's eigenbasis by (int32 [r], a view of the workspace)"""
        o = self.idx_offsets[i]
        return self.ws[o:o + self.short[i]].view(torch.int32)


def soap_step(plan: SoapPlan, p, g, m, v, gg, q, step_size: float, beta1: float, beta2: float, eps: float, lr_weight_decay: float,
              gg_weight: float, first: bool, refresh: bool, grad_scale: float = 1.0):
    """one SOAP call over the arena (p, g, m, v: fp32 flat, plan offsets into them; gg, q: the plan's r x r blocks), in place.  first: only
    GG and the eigenbasis; refresh: the basis is re-sorted and re-orthogonalised after the update.  step_size carries the bias correction"""
    L = _l.load()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, F32, nm)
        if not t.is_contiguous() or t.numel() != p.numel():
            raise _l.St355Error(f"soap_step: {nm} must be a contiguous fp32 arena of {p.numel()} elements")
    for t, nm in ((gg, "gg"), (q, "q")):
        _chk(t, F32, nm)
        if not t.is_contiguous() or t.numel() != plan.qq:
            raise _l.St355Error(f"soap_step: {nm} must be a contiguous fp32 arena of {plan.qq} elements")
    _l.check(L.st355_soap_step(_stream(), _ptr(plan.host), _ptr(plan.dev), _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(gg), _ptr(q), _ptr(plan.ws),
                               plan.ws_floats, float(grad_scale), float(beta1), float(beta2), float(eps), float(step_size), float(lr_weight_decay),
                               float(gg_weight), int(bool(first)), int(bool(refresh))), "soap_step")


def soap_eigh(plan: SoapPlan, gg, q=None, evals=None):
    """eigenvectors (columns of each r x r block of q) and eigenvalues (descending, plan.rr floats) of every symmetric block of gg"""
    L = _l.load()
    _chk(gg, F32, "gg")
    if not gg.is_contiguous() or gg.numel() != plan.qq:
        raise _l.St355Error(f"soap_eigh: gg must be a contiguous fp32 arena of {plan.qq} elements")
    q = torch.zeros_like(gg) if q is None else q
    evals = torch.zeros(plan.rr, dtype=F32, device=gg.device) if evals is None else evals
    _chk(q, F32, "q"); _chk(evals, F32, "evals")
    if q.numel() != plan.qq or evals.numel() != plan.rr or not q.is_contiguous() or not evals.is_contiguous():
        raise _l.St355Error("soap_eigh: q / evals do not match the plan")
    _l.check(L.st355_soap_eigh(_stream(), _ptr(plan.host), _ptr(plan.dev), _ptr(gg), _ptr(q), _ptr(evals)), "soap_eigh")
    return q, evals


def adafactor_factor_shape(shape):
    """(batch, R, C) of a parameter shape as torch.optim.Adafactor factors it: the last two dims, the leading dims a batch; a 1-D tensor of k
    elements is (1, 0, k)"""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or any(s < 1 for s in shape):
        raise _l.St355Error(f"adafactor_plan: cannot take a tensor of shape {shape}")
    if len(shape) == 1:
        return 1, 0, shape[0]
    batch = 1
    for s in shape[:-2]:
        batch *= s
    return batch, shape[-2], shape[-1]


class AdafactorPlan:
    """st355_adafactor_plan for a fixed list of tensors of one arena (element offsets, shapes of any rank): the host plan and its device copy, made
    once.  `rv_len`, `cv_len`, `var_len` are the lengths of the three fp32 state buffers; `rv_offsets[i]`, `cv_offsets[i]`, `var_offsets[i]` and
    `factors[i]` = (batch, R, C) place tensor i's slices in them.  The workspace (`ws_floats`) comes from the scratch helper at every step."""

    HEADER, RECORD = 8, 16

    def __init__(self, offsets, shapes, device):
        n = len(shapes)
        if n == 0 or len(offsets) != n:
            raise _l.St355Error("adafactor_plan: expected one offset per tensor shape")
        L = _l.load()
        self.factors = [adafactor_factor_shape(s) for s in shapes]
        if any(max(f) >= 2 ** 31 for f in self.factors):
            raise _l.St355Error("adafactor_plan: a dimension of 2^31 or more")
        off = (C.c_int64 * n)(*[int(o) for o in offsets])
        batch = (C.c_int64 * n)(*[f[0] for f in self.factors])
        rows = (C.c_int32 * n)(*[f[1] for f in self.factors])
        cols = (C.c_int32 * n)(*[f[2] for f in self.factors])
        self.host = torch.zeros(self.HEADER + self.RECORD * n, dtype=torch.int64)
        ws = C.c_int64(0)
        _l.check(L.st355_adafactor_plan(off, batch, rows, cols, n, _ptr(self.host), C.byref(ws)), "adafactor_plan")
        self.n = n
        self.ws_floats = int(ws.value)
        self.rv_len, self.cv_len, self.var_len = (int(self.host[i]) for i in (3, 4, 5))
        rec = self.host[self.HEADER:].view(n, self.RECORD)
        self.rv_offsets, self.cv_offsets, self.var_offsets = rec[:, 6].tolist(), rec[:, 7].tolist(), rec[:, 8].tolist()
        self.end = int(rec[-1, 0] + rec[-1, 5])
        self.dev = self.host.to(device)


def adafactor_step(plan: AdafactorPlan, pflat, gflat, row_var, col_var, variance, step: int, lr: float, beta2_decay: float = -0.8, eps1: Optional[float] = None,
                   eps2: float = 1e-3, d: float = 1.0, weight_decay: float = 0.0, grad_scale: float = 1.0):
    """one torch.optim.Adafactor step over the arena (pflat, gflat: bf16 or fp32 flat, plan offsets into them; row_var, col_var, variance: the plan's
    fp32 state buffers), in place.  `step` is the count AFTER this step (1 for the first).  eps1=None is torch's: the epsilon of the arena's dtype"""
    L = _l.load()
    if pflat.dtype not in (F32, BF16):
        raise _l.St355Error(f"adafactor_step: the arena must be fp32 or bf16, got {pflat.dtype}")
    _chk(pflat, pflat.dtype, "pflat"); _chk(gflat, pflat.dtype, "gflat")
    if not pflat.is_contiguous() or not gflat.is_contiguous() or gflat.numel() != pflat.numel() or pflat.numel() < plan.end:
        raise _l.St355Error(f"adafactor_step: pflat and gflat must be contiguous arenas of one length >= {plan.end}")
    for t, nm, k in ((row_var, "row_var", plan.rv_len), (col_var, "col_var", plan.cv_len), (variance, "variance", plan.var_len)):
        _chk(t, F32, nm)
        if not t.is_contiguous() or t.numel() < k:
            raise _l.St355Error(f"adafactor_step: {nm} must be a contiguous fp32 buffer of at least {k} elements")
    if step < 1:
        raise _l.St355Error("adafactor_step: step counts from 1")
    if eps1 is None:
        eps1 = torch.finfo(pflat.dtype).eps
    ws = _scratch("adafactor", pflat.device, 4 * max(plan.ws_floats, 1))
    _l.check(L.st355_adafactor_step(_stream(), _ptr(plan.host), _ptr(plan.dev), _ptr(pflat), _ptr(gflat), pflat.element_size(), pflat.numel(),
                                    _ptr(row_var), _ptr(col_var), _ptr(variance), _ptr(ws), ws.numel() // 4, float(grad_scale),
                                    float(step) ** beta2_decay, min(float(lr), 1.0 / float(step) ** 0.5), float(eps1), float(eps2), float(d),
                                    float(lr) * float(weight_decay)), "adafactor_step")


def _token_view(t, name: str):
    """a [B, rows, D] bf16 view with unit inner stride (e.g. the image rows of a joint [B * S, D] buffer): (B, rows, D, row stride, batch stride)"""
    _chk(t, BF16, name)
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) < 0:
        raise _l.St355Error(f"{name}: expected a [B, rows, D] view with unit inner stride, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)


def layersync_fwd(student, teacher, G, cos_rows, sim):
    """LayerSync (st355_layersync_fwd): student / teacher [B, rows, D] bf16 views of one row stride; cos_rows[B * rows] fp32 = the per-token cosine, sim (one fp32)
    = its mean, G [B * rows, D] bf16 contiguous = d sim / d student.  G may be the student's own (compact) buffer.  Writes into the tensors given, allocates nothing."""
    L = _l.load()
    B, rows, D, ld, sb = _token_view(student, "student")
    Bt, rt, Dt, ldt, tb = _token_view(teacher, "teacher")
    _chk(G, BF16, "G"); _chk(cos_rows, F32, "cos_rows"); _chk(sim, F32, "sim")
    if (Bt, rt, Dt, ldt) != (B, rows, D, ld):
        raise _l.St355Error(f"layersync_fwd: student {tuple(student.shape)} (row stride {ld}) and teacher {tuple(teacher.shape)} (row stride {ldt}) must agree")
    if not G.is_contiguous() or G.numel() != B * rows * D or not cos_rows.is_contiguous() or cos_rows.numel() != B * rows or sim.numel() != 1:
        raise _l.St355Error("layersync_fwd: G must be contiguous with B * rows * D elements, cos_rows contiguous with B * rows, sim one element")
    if G.data_ptr() == student.data_ptr() and not student.is_contiguous():
        raise _l.St355Error("layersync_fwd: G may alias the student only when the student is compact")
    _l.check(L.st355_layersync_fwd(_stream(), _ptr(student), _ptr(teacher), _ptr(G), _ptr(cos_rows), _ptr(sim), B, rows, D, ld, sb, tb, None), "layersync_fwd")
    return G, cos_rows, sim


def layersync_inject(dx, G, scale):
    """dx[b, r, :] = bf16(float(dx) + scale * float(G)) in place (st355_layersync_inject): dx a [B, rows, D] bf16 view, G [B * rows, D] contiguous, scale ONE fp32 on the device"""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(dx, "dx")
    _chk(G, BF16, "G"); _chk(scale, F32, "scale")
    if not G.is_contiguous() or G.numel() != B * rows * D or scale.numel() != 1:
        raise _l.St355Error("layersync_inject: G must be contiguous with B * rows * D elements, scale one fp32 element")
    _l.check(L.st355_layersync_inject(_stream(), _ptr(dx), _ptr(G), _ptr(scale), B, rows, D, ld, bs), "layersync_inject")
    return dx


IG_N = 64          # output features of the Internal Guidance head (16 latent channels x a 2 x 2 patch)


def _ig_params(name: str, gamma, beta, W, b):
    """the head's four parameters (or their gradients): all fp32 (adapter arena) or all bf16 (full fine-tune arena), contiguous, W [64, D].  Returns (D, bf16?)"""
    dt = W.dtype
    if dt not in (F32, BF16) or any(t.dtype != dt for t in (gamma, beta, b)):
        raise _l.St355Error(f"{name}: gamma, beta, W and b must share one dtype, fp32 or bf16")
    for t in (gamma, beta, W, b):
        _dev(t, name)
    if W.dim() != 2 or W.shape[0] != IG_N:
        raise _l.St355Error(f"{name}: the head has N = {IG_N} output features, got W {tuple(W.shape)}")
    D = W.shape[1]
    if gamma.numel() != D or beta.numel() != D or b.numel() != IG_N or not all(t.is_contiguous() for t in (gamma, beta, W, b)):
        raise _l.St355Error(f"{name}: expected contiguous gamma [D], beta [D], W [{IG_N}, D], b [{IG_N}]")
    return D, int(dt == BF16)


def ig_fold(gamma, beta, W, b, Wf, WfT, c):
    """Internal Guidance head (st355_ig_fold): Wf [64, D] = bf16(gamma * W), WfT [D, 64] its transpose, c [64] = bf16(W beta + b) — the operands of
    ig_head_fwd / ig_head_bwd, from the current parameters (fp32 or bf16).  Writes into the tensors given."""
    L = _l.load()
    D, p16 = _ig_params("ig_fold", gamma, beta, W, b)
    _chk(Wf, BF16, "Wf"); _chk(WfT, BF16, "WfT"); _chk(c, BF16, "c")
    if tuple(Wf.shape) != (IG_N, D) or tuple(WfT.shape) != (D, IG_N) or c.numel() != IG_N or not (Wf.is_contiguous() and WfT.is_contiguous() and c.is_contiguous()):
        raise _l.St355Error(f"ig_fold: expected contiguous Wf [{IG_N}, {D}], WfT [{D}, {IG_N}], c [{IG_N}]")
    _l.check(L.st355_ig_fold(_stream(), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b), p16, _ptr(Wf), _ptr(WfT), _ptr(c), IG_N, D), "ig_fold")
    return Wf, WfT, c


def ig_head_fwd(h, Wf, c, xhat, rstd, y):
    """Internal Guidance head forward: h a [B, rows, D] bf16 view (read once, no compact copy) -> xhat [B * rows, D] compact bf16 = LN(h) without affine (centred
    variance), rstd [B * rows] fp32 (st355_ig_head_fwd), then the tokens y [B * rows, 64] bf16 = xhat Wf^T + c on the thin GEMM route (D % 64 == 0).  Writes into the
    tensors given."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(h, "h")
    _chk(xhat, BF16, "xhat"); _chk(rstd, F32, "rstd"); _chk(y, BF16, "y"); _chk(Wf, BF16, "Wf"); _chk(c, BF16, "c")
    M = B * rows
    if tuple(Wf.shape) != (IG_N, D):
        raise _l.St355Error(f"ig_head_fwd: the head has N = {IG_N} output features over D = {D}, got Wf {tuple(Wf.shape)}")
    if D % 64:
        raise _l.St355Error(f"ig_head_fwd: D must be a multiple of 64, the contraction granule of the projection's GEMM (got {D}; the row kernel itself takes D % 8 == 0)")
    if tuple(xhat.shape) != (M, D) or not xhat.is_contiguous() or rstd.numel() != M or not rstd.is_contiguous() or tuple(y.shape) != (M, IG_N) or not y.is_contiguous():
        raise _l.St355Error(f"ig_head_fwd: expected contiguous xhat [{M}, {D}], rstd [{M}], y [{M}, {IG_N}]")
    _l.check(L.st355_ig_head_fwd(_stream(), _ptr(h), _ptr(xhat), _ptr(rstd), B, rows, D, ld, bs), "ig_head_fwd")
    gemm(xhat, Wf, bias=c, out=y)
    return xhat, rstd, y


def ig_head_bwd(xhat, rstd, dy, WfT, dx):
    """Internal Guidance head backward into the dX chain (st355_ig_head_bwd): dx, a [B, rows, D] bf16 view, += rstd * (g - mean(g) - xhat * mean(g * xhat)) with
    g = dy Wf never stored (dy [B * rows, 64] bf16 compact, WfT [D, 64]); fp32 sum, one bf16 rounding, rows outside the view untouched."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(dx, "dx")
    _chk(xhat, BF16, "xhat"); _chk(rstd, F32, "rstd"); _chk(dy, BF16, "dy"); _chk(WfT, BF16, "WfT")
    M = B * rows
    if dy.dim() != 2 or dy.shape[1] != IG_N or tuple(WfT.shape) != (D, IG_N):
        raise _l.St355Error(f"ig_head_bwd: the head has N = {IG_N} output features over D = {D}, got dy {tuple(dy.shape)}, WfT {tuple(WfT.shape)}")
    if tuple(xhat.shape) != (M, D) or dy.shape[0] != M or rstd.numel() != M or not (xhat.is_contiguous() and dy.is_contiguous() and rstd.is_contiguous() and WfT.is_contiguous()):
        raise _l.St355Error(f"ig_head_bwd: expected contiguous xhat [{M}, {D}], rstd [{M}], dy [{M}, {IG_N}], WfT [{D}, {IG_N}]")
    _l.check(L.st355_ig_head_bwd(_stream(), _ptr(xhat), _ptr(rstd), _ptr(dy), _ptr(WfT), _ptr(dx), B, rows, D, IG_N, ld, bs), "ig_head_bwd")
    return dx


def ig_wgrad(xhat, dy, gamma, beta, W, g_gamma, g_beta, g_W, g_b, accumulate: bool = False):
    """the head's four parameter gradients (st355_ig_wgrad) from P = dy^T xhat (skinny_tn: fp32 [64, D]) and db = colsum(dy): g_W = P * gamma + db beta^T, g_b = db,
    g_gamma = sum_n W * P, g_beta = sum_n W * db.  Parameters and gradients share one dtype (fp32 or bf16); accumulate adds to what the gradients hold."""
    L = _l.load()
    D, p16 = _ig_params("ig_wgrad", gamma, beta, W, g_b)
    D2, g16 = _ig_params("ig_wgrad", g_gamma, g_beta, g_W, g_b)
    _chk(xhat, BF16, "xhat"); _chk(dy, BF16, "dy")
    if D2 != D or g16 != p16 or xhat.dim() != 2 or dy.dim() != 2 or xhat.shape[1] != D or dy.shape[1] != IG_N or dy.shape[0] != xhat.shape[0] \
            or not (xhat.is_contiguous() and dy.is_contiguous()):
        raise _l.St355Error(f"ig_wgrad: expected contiguous xhat [M, {D}], dy [M, {IG_N}] and gradients in the parameters' dtype and shapes")
    ws = _scratch("ig_wgrad", xhat.device, (IG_N * D + IG_N) * 4).view(F32)
    P, db = ws[:IG_N * D].view(IG_N, D), ws[IG_N * D:IG_N * D + IG_N].view(1, IG_N)
    skinny_tn(xhat, dy, P, 1, D, IG_N)
    colsum_prod(dy, db)
    _l.check(L.st355_ig_wgrad(_stream(), _ptr(P), _ptr(db), _ptr(gamma), _ptr(beta), _ptr(W), p16, _ptr(g_gamma), _ptr(g_beta), _ptr(g_W), _ptr(g_b), IG_N, D,
                              1 if accumulate else 0), "ig_wgrad")
    return g_gamma, g_beta, g_W, g_b


NEXTLAT_MODES = {"smooth_l1": 0, "mse": 1}          # nextlat.py:147-150 `nextlat_state_loss`


def _al16(name: str, *ts):
    for t in ts:
        if t.data_ptr() % 16:
            raise _l.St355Error(f"{name}: operands must be 16-byte aligned (a view that starts off a 16-byte boundary)")


def _nextlat_params(name: str, gamma, beta, W_up, b_up, W_down, b_down):
    """the predictor's six parameters (or their gradients): all fp32 (adapter arena) or all bf16 (full fine-tune arena), contiguous, 16-byte aligned, W_up [2D, D],
    W_down [D, 2D].  Returns (D, bf16?)"""
    ts = (gamma, beta, W_up, b_up, W_down, b_down)
    dt = W_up.dtype
    if dt not in (F32, BF16) or any(t.dtype != dt for t in ts):
        raise _l.St355Error(f"{name}: the six predictor tensors must share one dtype, fp32 or bf16")
    for t in ts:
        _dev(t, name)
    if W_up.dim() != 2 or W_up.shape[0] != 2 * W_up.shape[1]:
        raise _l.St355Error(f"{name}: expected W_up [2D, D], got {tuple(W_up.shape)}")
    D = W_up.shape[1]
    if D % 8 or D > 4096:
        raise _l.St355Error(f"{name}: D must be a multiple of 8, at most 4096 (got {D})")
    if tuple(W_down.shape) != (D, 2 * D) or gamma.numel() != D or beta.numel() != D or b_up.numel() != 2 * D or b_down.numel() != D \
            or not all(t.is_contiguous() for t in ts):
        raise _l.St355Error(f"{name}: expected contiguous gamma [D], beta [D], W_up [2D, D], b_up [2D], W_down [D, 2D], b_down [D] with D = {D}")
    _al16(name, *ts)
    return D, int(dt == BF16)


def _nextlat_scale(name: str, s):
    if not torch.is_tensor(s):
        raise _l.St355Error(f"{name}: the scale is ONE fp32 on the device, not a host number")
    _chk(s, F32, "scale")
    if s.numel() != 1:
        raise _l.St355Error(f"{name}: the scale is ONE fp32 on the device")


def nextlat_fold(gamma, beta, W_up, b_up, W_down, b_down, W1f, W1fT, c1, Wd, WdT, bd):
    """NextLat predictor (st355_nextlat_fold): W1f [2D, D] = bf16(gamma * W_up), W1fT [D, 2D] its transpose, c1 [2D] = bf16(W_up beta + b_up), Wd [D, 2D] =
    bf16(W_down), WdT [2D, D], bd [D] = bf16(b_down) — the operands of the predictor's four GEMMs, from the current parameters (fp32 or bf16).  Writes into the
    tensors given."""
    L = _l.load()
    D, p16 = _nextlat_params("nextlat_fold", gamma, beta, W_up, b_up, W_down, b_down)
    outs = (W1f, W1fT, c1, Wd, WdT, bd)
    for t, nm in zip(outs, ("W1f", "W1fT", "c1", "Wd", "WdT", "bd")):
        _chk(t, BF16, nm)
    if tuple(W1f.shape) != (2 * D, D) or tuple(W1fT.shape) != (D, 2 * D) or c1.numel() != 2 * D or tuple(Wd.shape) != (D, 2 * D) or tuple(WdT.shape) != (2 * D, D) \
            or bd.numel() != D or not all(t.is_contiguous() for t in outs):
        raise _l.St355Error(f"nextlat_fold: expected contiguous W1f [2D, D], W1fT [D, 2D], c1 [2D], Wd [D, 2D], WdT [2D, D], bd [D] with D = {D}")
    _al16("nextlat_fold", *outs)
    _l.check(L.st355_nextlat_fold(_stream(), _ptr(gamma), _ptr(beta), _ptr(W_up), _ptr(b_up), _ptr(W_down), _ptr(b_down), p16, _ptr(W1f), _ptr(W1fT), _ptr(c1),
                                  _ptr(Wd), _ptr(WdT), _ptr(bd), D), "nextlat_fold")
    return outs


def nextlat_rows(h, xhat, rstd):
    """the predictor's row pass (st355_ig_head_fwd as it is): h a [B, rows, D] bf16 view (read once, no compact copy) -> xhat [B * rows, D] compact bf16 = LN(h) without
    affine (centred variance, eps 1e-6), rstd [B * rows] fp32.  D % 64 == 0: xhat feeds the up projection's GEMM."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(h, "h")
    _chk(xhat, BF16, "xhat"); _chk(rstd, F32, "rstd")
    M = B * rows
    if D % 64:
        raise _l.St355Error(f"nextlat_rows: D must be a multiple of 64, the contraction granule of the up projection's GEMM (got {D}; the row kernel itself takes D % 8 == 0)")
    if D > 4096 or ld % 8 or bs % 8:
        raise _l.St355Error(f"nextlat_rows: the view's strides must be multiples of 8 elements, D at most 4096 (got D = {D}, strides {h.stride()})")
    if tuple(xhat.shape) != (M, D) or not xhat.is_contiguous() or rstd.numel() != M or not rstd.is_contiguous():
        raise _l.St355Error(f"nextlat_rows: expected contiguous xhat [{M}, {D}], rstd [{M}]")
    _al16("nextlat_rows", h, xhat)
    _l.check(L.st355_ig_head_fwd(_stream(), _ptr(h), _ptr(xhat), _ptr(rstd), B, rows, D, ld, bs), "nextlat_rows")
    return xhat, rstd


def _gelu_operands(name: str, *ts):
    for t in ts:
        _chk(t, BF16, name)
    n = ts[0].numel()
    if n == 0 or n % 8 or any(t.shape != ts[0].shape or not t.is_contiguous() for t in ts):
        raise _l.St355Error(f"{name}: expected contiguous bf16 tensors of one shape, a multiple of 8 elements")
    _al16(name, *ts)
    return n


def gelu_erf(U, A):
    """A = gelu_erf(U) (st355_gelu_erf_fwd; the exact erf form of F.gelu), contiguous bf16, 8 elements per lane.  Writes into A."""
    L = _l.load()
    n = _gelu_operands("gelu_erf", U, A)
    _l.check(L.st355_gelu_erf_fwd(_stream(), _ptr(U), _ptr(A), n), "gelu_erf_fwd")
    return A


def gelu_erf_bwd(U, dA, dU):
    """dU = dA * gelu_erf'(U) (st355_gelu_erf_bwd); dU may be dA."""
    L = _l.load()
    n = _gelu_operands("gelu_erf_bwd", U, dA, dU)
    _l.check(L.st355_gelu_erf_bwd(_stream(), _ptr(U), _ptr(dA), _ptr(dU), n), "gelu_erf_bwd")
    return dU


def nextlat_loss(pred, target, mode: str, loss):
    """NextLat state loss (st355_nextlat_loss): pred [B * rows, D] compact bf16, target a [B, rows, D] bf16 view (the block output's rows 1 .. S-1).  mode
    "smooth_l1" (beta 1) or "mse".  pred is OVERWRITTEN with psi = d(per-element loss) / d pred (clamp(pred - t, -1, 1) / 2 (pred - t)); loss (one fp32) = the mean
    over B * rows * D, a two-stage fixed-order reduction."""
    L = _l.load()
    if mode not in NEXTLAT_MODES:
        raise _l.St355Error("nextlat_loss: mode must be 'smooth_l1' or 'mse'")
    B, rows, D, ld, bs = _token_view(target, "target")
    _chk(pred, BF16, "pred"); _chk(loss, F32, "loss")
    M = B * rows
    if D % 8 or D > 4096 or ld % 8 or bs % 8:
        raise _l.St355Error(f"nextlat_loss: D and the view's strides must be multiples of 8 elements, D at most 4096 (got D = {D}, strides {target.stride()})")
    if tuple(pred.shape) != (M, D) or not pred.is_contiguous() or loss.numel() != 1:
        raise _l.St355Error(f"nextlat_loss: expected contiguous pred [{M}, {D}] and one fp32 for the loss")
    _al16("nextlat_loss", pred, target)
    ws = _scratch("nextlat_loss", pred.device, L.st355_nextlat_loss_workspace(M))
    _l.check(L.st355_nextlat_loss(_stream(), _ptr(pred), _ptr(target), B, rows, D, ld, bs, NEXTLAT_MODES[mode], _ptr(loss), _ptr(ws)), "nextlat_loss")
    return loss


def nextlat_ln_bwd_add(g, xhat, rstd, scale, dx):
    """the predictor's LayerNorm backward into the dX chain (st355_nextlat_ln_bwd_add): dx, a [B, rows, D] bf16 view, = bf16(float(dx) + s * rstd * (g - mean(g) -
    xhat * mean(g * xhat))); g / xhat [B * rows, D] compact bf16, s ONE fp32 on the device.  Rows outside the view are not touched."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(dx, "dx")
    _chk(g, BF16, "g"); _chk(xhat, BF16, "xhat"); _chk(rstd, F32, "rstd")
    _nextlat_scale("nextlat_ln_bwd_add", scale)
    M = B * rows
    if D % 8 or D > 4096 or ld % 8 or bs % 8:
        raise _l.St355Error(f"nextlat_ln_bwd_add: D and the view's strides must be multiples of 8 elements, D at most 4096 (got D = {D}, strides {dx.stride()})")
    if tuple(g.shape) != (M, D) or tuple(xhat.shape) != (M, D) or rstd.numel() != M or not (g.is_contiguous() and xhat.is_contiguous() and rstd.is_contiguous()):
        raise _l.St355Error(f"nextlat_ln_bwd_add: expected contiguous g [{M}, {D}], xhat [{M}, {D}], rstd [{M}]")
    _al16("nextlat_ln_bwd_add", g, xhat, dx)
    _l.check(L.st355_nextlat_ln_bwd_add(_stream(), _ptr(g), _ptr(xhat), _ptr(rstd), _ptr(scale), _ptr(dx), B, rows, D, ld, bs), "nextlat_ln_bwd_add")
    return dx


def nextlat_wgrad_up(P1, db1, gamma, beta, W_up, scale, g_gamma, g_beta, g_W, g_b, accumulate: bool = False):
    """gradients of the predictor's LayerNorm affine and up projection (st355_nextlat_wgrad_up) from P1 [2D, D] bf16 = dU^T xhat (gemm_tn) and db1 [2D] fp32 =
    colsum(dU): g_W = s (P1 * gamma + db1 beta^T), g_b = s db1, g_gamma = s sum_n W_up * P1, g_beta = s sum_n W_up * db1.  Parameters and gradients share one
    dtype (fp32 or bf16); accumulate adds to what the gradients hold."""
    L = _l.load()
    dt = W_up.dtype
    ts = (gamma, beta, W_up, g_gamma, g_beta, g_W, g_b)
    if dt not in (F32, BF16) or any(t.dtype != dt for t in ts):
        raise _l.St355Error("nextlat_wgrad_up: parameters and gradients must share one dtype, fp32 or bf16")
    _chk(P1, BF16, "P1"); _chk(db1, F32, "db1")
    _nextlat_scale("nextlat_wgrad_up", scale)
    for t in ts:
        _dev(t, "nextlat_wgrad_up")
    if W_up.dim() != 2 or W_up.shape[0] != 2 * W_up.shape[1]:
        raise _l.St355Error(f"nextlat_wgrad_up: expected W_up [2D, D], got {tuple(W_up.shape)}")
    D = W_up.shape[1]
    if D % 8 or D > 4096:
        raise _l.St355Error(f"nextlat_wgrad_up: D must be a multiple of 8, at most 4096 (got {D})")
    if tuple(P1.shape) != (2 * D, D) or db1.numel() != 2 * D or tuple(g_W.shape) != (2 * D, D) or g_b.numel() != 2 * D or any(t.numel() != D for t in (gamma, beta, g_gamma, g_beta)) \
            or not all(t.is_contiguous() for t in ts + (P1, db1)):
        raise _l.St355Error(f"nextlat_wgrad_up: expected contiguous P1 [2D, D], db1 [2D] and parameters / gradients in the predictor's shapes with D = {D}")
    _al16("nextlat_wgrad_up", P1, gamma, beta, W_up, g_W)
    ws = _scratch("nextlat_wgrad", P1.device, L.st355_nextlat_wgrad_workspace(D))
    _l.check(L.st355_nextlat_wgrad_up(_stream(), _ptr(P1), _ptr(db1), _ptr(gamma), _ptr(beta), _ptr(W_up), int(dt == BF16), _ptr(scale), _ptr(g_gamma), _ptr(g_beta),
                                      _ptr(g_W), _ptr(g_b), D, 1 if accumulate else 0, _ptr(ws)), "nextlat_wgrad_up")
    return g_gamma, g_beta, g_W, g_b


def nextlat_wgrad_down(P2, db2, scale, g_W, g_b, accumulate: bool = False):
    """gradients of the predictor's down projection (st355_nextlat_wgrad_down): g_W [D, 2D] = s P2 (P2 bf16 = psi^T A, gemm_tn), g_b [D] = s db2 (db2 fp32 =
    colsum(psi)); the gradients fp32 or bf16; accumulate adds to what they hold."""
    L = _l.load()
    dt = g_W.dtype
    if dt not in (F32, BF16) or g_b.dtype != dt:
        raise _l.St355Error("nextlat_wgrad_down: the gradients must share one dtype, fp32 or bf16")
    _chk(P2, BF16, "P2"); _chk(db2, F32, "db2"); _dev(g_W, "g_W"); _dev(g_b, "g_b")
    _nextlat_scale("nextlat_wgrad_down", scale)
    if g_W.dim() != 2 or g_W.shape[1] != 2 * g_W.shape[0]:
        raise _l.St355Error(f"nextlat_wgrad_down: expected g_W [D, 2D], got {tuple(g_W.shape)}")
    D = g_W.shape[0]
    if D % 8 or D > 4096:
        raise _l.St355Error(f"nextlat_wgrad_down: D must be a multiple of 8, at most 4096 (got {D})")
    if tuple(P2.shape) != (D, 2 * D) or db2.numel() != D or g_b.numel() != D or not all(t.is_contiguous() for t in (P2, db2, g_W, g_b)):
        raise _l.St355Error(f"nextlat_wgrad_down: expected contiguous P2 [D, 2D], db2 [D], g_W [D, 2D], g_b [D] with D = {D}")
    _al16("nextlat_wgrad_down", P2, db2, g_W, g_b)
    _l.check(L.st355_nextlat_wgrad_down(_stream(), _ptr(P2), _ptr(db2), int(dt == BF16), _ptr(scale), _ptr(g_W), _ptr(g_b), D, 1 if accumulate else 0),
             "nextlat_wgrad_down")
    return g_W, g_b


def _sf_vec(t, name: str):
    """a [B] fp32 device vector of Self-Flow's views pass"""
    _chk(t, F32, name)
    if t.dim() != 1 or not t.is_contiguous():
        raise _l.St355Error(f"self_flow_views: {name} must be a contiguous [B] fp32 tensor, got {tuple(t.shape)}")


def self_flow_views(latents, noise, sigma, sigma_alt, timesteps, timesteps_alt, uniforms, ratio: float, patch: int = 2, want_sigma_grid: bool = False, out=None):
    """Self-Flow's two views in ONE streaming pass (st355_self_flow_views; common.py `_prepare_image_crepa_self_flow_batch`): latents / noise [B, C, H, W], both bf16 or
    both fp32 (each sample contiguous; the batch stride may be larger), sigma / sigma_alt / timesteps / timesteps_alt [B] fp32 and uniforms [B, H/p, W/p] fp32 on the
    device.  A token is masked iff its uniform < ratio.  Returns (noisy_student, noisy_teacher, token_timesteps [B, (H/p)(W/p)] fp32, sigma_teacher [B] fp32,
    timestep_teacher [B] fp32, sigma_grid [B, 1, H, W] fp32 or None).  fp32 arithmetic, one rounding per output element, nothing read on the host.  out: the first
    five outputs preallocated (contiguous, 16-byte aligned views), else they are allocated here."""
    L = _l.load()
    if latents.dtype not in (BF16, F32) or noise.dtype != latents.dtype:
        raise _l.St355Error(f"self_flow_views: latents and noise must share one dtype, bf16 or fp32 (got {latents.dtype}, {noise.dtype})")
    _dev(latents, "latents"); _dev(noise, "noise")
    if latents.dim() != 4 or noise.shape != latents.shape:
        raise _l.St355Error(f"self_flow_views: expected latents and noise [B, C, H, W] of one shape, got {tuple(latents.shape)} and {tuple(noise.shape)}")
    B, Cc, H, W = latents.shape
    patch = int(patch)
    if patch < 1 or H % patch or W % patch:
        raise _l.St355Error(f"self_flow_views: H % patch_size != 0 or W % patch_size != 0 (H = {H}, W = {W}, patch_size = {patch}): the reference's repeat_interleave "
                            "and slice are not a defined computation there")
    if not 0.0 <= float(ratio) <= 0.5:
        raise _l.St355Error(f"self_flow_views: the mask ratio must lie in [0, 0.5] (got {ratio})")
    for t, nm in ((latents, "latents"), (noise, "noise")):
        if not t[0].is_contiguous() or (B > 1 and t.stride(0) < Cc * H * W):
            raise _l.St355Error(f"self_flow_views: every sample of {nm} must be contiguous, samples at least C * H * W elements apart (strides {t.stride()})")
    for t, nm in ((sigma, "sigma"), (sigma_alt, "sigma_alt"), (timesteps, "timesteps"), (timesteps_alt, "timesteps_alt")):
        _sf_vec(t, nm)
        if t.numel() != B:
            raise _l.St355Error(f"self_flow_views: {nm} has {t.numel()} entries for a batch of {B}")
    _chk(uniforms, F32, "uniforms")
    if tuple(uniforms.shape) != (B, H // patch, W // patch) or not uniforms.is_contiguous():
        raise _l.St355Error(f"self_flow_views: expected contiguous uniforms [{B}, {H // patch}, {W // patch}], got {tuple(uniforms.shape)}")
    vec = 8 if latents.dtype == BF16 else 4
    lbs, nbs = (latents.stride(0), noise.stride(0)) if B > 1 else (Cc * H * W, Cc * H * W)
    if (Cc * H * W) % vec or lbs % vec or nbs % vec:
        raise _l.St355Error(f"self_flow_views: C * H * W and the batch strides must be multiples of {vec} elements (16 bytes per lane), got {Cc * H * W}, {lbs}, {nbs}")
    _al16("self_flow_views", latents, noise)
    dev = latents.device
    ntok = (H // patch) * (W // patch)
    if out is None:
        noisy_s, noisy_t = torch.empty(B, Cc, H, W, dtype=latents.dtype, device=dev), torch.empty(B, Cc, H, W, dtype=latents.dtype, device=dev)
        tok = torch.empty(B, ntok, dtype=F32, device=dev)
        sig_T, t_T = torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev)
    else:
        noisy_s, noisy_t, tok, sig_T, t_T = out
        for t, shp, dt in ((noisy_s, (B, Cc, H, W), latents.dtype), (noisy_t, (B, Cc, H, W), latents.dtype), (tok, (B, ntok), F32), (sig_T, (B,), F32), (t_T, (B,), F32)):
            _chk(t, dt, "out")
            if tuple(t.shape) != shp or not t.is_contiguous():
                raise _l.St355Error(f"self_flow_views: expected a contiguous output of shape {shp}, got {tuple(t.shape)} (strides {t.stride()})")
        _al16("self_flow_views", noisy_s, noisy_t)
    grid = torch.empty(B, 1, H, W, dtype=F32, device=dev) if want_sigma_grid else None
    _l.check(L.st355_self_flow_views(_stream(), _ptr(latents), _ptr(noise), int(latents.dtype == BF16), lbs, nbs, _ptr(sigma), _ptr(sigma_alt), _ptr(timesteps),
                                     _ptr(timesteps_alt), _ptr(uniforms), float(ratio), patch, _ptr(noisy_s), _ptr(noisy_t), _ptr(tok), _ptr(sig_T), _ptr(t_T), _ptr(grid),
                                     B, Cc, H, W), "self_flow_views")
    return noisy_s, noisy_t, tok, sig_T, t_T, grid


def _sf_params(name: str, gamma, beta, W, b):
    """the projector's four fp32 parameters (or their gradients): contiguous, 16-byte aligned, W [D, D].  Returns D"""
    ts = (gamma, beta, W, b)
    for t in ts:
        _chk(t, F32, name)
    if W.dim() != 2 or W.shape[0] != W.shape[1]:
        raise _l.St355Error(f"{name}: expected W [D, D], got {tuple(W.shape)}")
    D = W.shape[1]
    if D % 8 or D > 4096:
        raise _l.St355Error(f"{name}: D must be a multiple of 8, at most 4096 (got {D})")
    if any(t.numel() != D for t in (gamma, beta, b)) or not all(t.is_contiguous() for t in ts):
        raise _l.St355Error(f"{name}: expected contiguous gamma [D], beta [D], W [D, D], b [D] with D = {D}")
    _al16(name, gamma, beta, W)
    return D


def self_flow_fold(gamma, beta, W, b, Wf, WfT, c):
    """Self-Flow projector (st355_self_flow_fold): Wf [D, D] = bf16(gamma * W), WfT its transpose, c [D] = bf16(W beta + b) — the operands of the projection
    proj = xhat Wf^T + c and of the backward's g = G Wf, from the current fp32 parameters.  Writes into the tensors given."""
    L = _l.load()
    D = _sf_params("self_flow_fold", gamma, beta, W, b)
    for t, nm in ((Wf, "Wf"), (WfT, "WfT"), (c, "c")):
        _chk(t, BF16, nm)
    if tuple(Wf.shape) != (D, D) or tuple(WfT.shape) != (D, D) or c.numel() != D or not (Wf.is_contiguous() and WfT.is_contiguous() and c.is_contiguous()):
        raise _l.St355Error(f"self_flow_fold: expected contiguous Wf [D, D], WfT [D, D], c [D] with D = {D}")
    _al16("self_flow_fold", Wf, WfT)
    _l.check(L.st355_self_flow_fold(_stream(), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b), _ptr(Wf), _ptr(WfT), _ptr(c), D), "self_flow_fold")
    return Wf, WfT, c


def self_flow_rows(h, xhat, rstd):
    """the projector's row pass (st355_self_flow_rows): h a [B, rows, D] bf16 view (read once, no compact copy) -> xhat [B * rows, D] compact bf16 = LN(h) without
    affine (centred variance, nn.LayerNorm's default eps 1e-5), rstd [B * rows] fp32.  D % 64 == 0: xhat feeds the projection's GEMM."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(h, "h")
    _chk(xhat, BF16, "xhat"); _chk(rstd, F32, "rstd")
    M = B * rows
    if D % 64:
        raise _l.St355Error(f"self_flow_rows: D must be a multiple of 64, the contraction granule of the projection's GEMM (got {D}; the row kernel itself takes D % 8 == 0)")
    if D > 4096 or ld % 8 or bs % 8:
        raise _l.St355Error(f"self_flow_rows: the view's strides must be multiples of 8 elements, D at most 4096 (got D = {D}, strides {h.stride()})")
    if tuple(xhat.shape) != (M, D) or not xhat.is_contiguous() or rstd.numel() != M or not rstd.is_contiguous():
        raise _l.St355Error(f"self_flow_rows: expected contiguous xhat [{M}, {D}], rstd [{M}]")
    _al16("self_flow_rows", h, xhat)
    _l.check(L.st355_self_flow_rows(_stream(), _ptr(h), _ptr(xhat), _ptr(rstd), B, rows, D, ld, bs), "self_flow_rows")
    return xhat, rstd


def self_flow_wgrad(P, db, gamma, beta, W, scale, g_gamma, g_beta, g_W, g_b, accumulate: bool = False):
    """gradients of the projector (st355_self_flow_wgrad) from P [D, D] bf16 = G^T xhat (gemm_tn) and db [D] fp32 = colsum(G): g_W = s (P * gamma + db beta^T),
    g_b = s db, g_gamma = s sum_n W * P, g_beta = s sum_n W * db; s ONE fp32 on the device.  accumulate adds to what the gradients hold."""
    L = _l.load()
    D = _sf_params("self_flow_wgrad", gamma, beta, W, g_b)
    _sf_params("self_flow_wgrad", g_gamma, g_beta, g_W, g_b)
    _chk(P, BF16, "P"); _chk(db, F32, "db")
    _nextlat_scale("self_flow_wgrad", scale)
    if tuple(P.shape) != (D, D) or db.numel() != D or tuple(g_W.shape) != (D, D) or not (P.is_contiguous() and db.is_contiguous()):
        raise _l.St355Error(f"self_flow_wgrad: expected contiguous P [D, D] bf16, db [D] fp32 and gradients in the projector's shapes with D = {D}")
    _al16("self_flow_wgrad", P)
    ws = _scratch("self_flow_wgrad", P.device, L.st355_self_flow_wgrad_workspace(D))
    _l.check(L.st355_self_flow_wgrad(_stream(), _ptr(P), _ptr(db), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(scale), _ptr(g_gamma), _ptr(g_beta), _ptr(g_W), _ptr(g_b), D,
                                     1 if accumulate else 0, _ptr(ws)), "self_flow_wgrad")
    return g_gamma, g_beta, g_W, g_b


# ------------------------------------------------------------------------------------------------
# Self-Transcendence (csrc/self_transcendence.hip): the projector Linear(D -> Hp) -> SiLU -> Linear(Hp -> Hp) -> SiLU -> Linear(Hp -> D) and its masked per-sample MSE
# ------------------------------------------------------------------------------------------------
def _st_params(name: str, W1, b1, W2, b2, W3, b3):
    """the projector's six fp32 parameters (or their gradients): contiguous, W1 [Hp, D], W2 [Hp, Hp], W3 [D, Hp].  Returns (D, Hp)"""
    ts = (W1, b1, W2, b2, W3, b3)
    for t in ts:
        _chk(t, F32, name)
    if W1.dim() != 2 or W2.dim() != 2 or W3.dim() != 2:
        raise _l.St355Error(f"{name}: expected W1 [Hp, D], W2 [Hp, Hp], W3 [D, Hp]")
    Hp, D = W1.shape
    if D % 8 or Hp % 8 or D > 16384 or Hp > 16384:
        raise _l.St355Error(f"{name}: D and Hp must be multiples of 8, at most 16384 (got D = {D}, Hp = {Hp})")
    if tuple(W2.shape) != (Hp, Hp) or tuple(W3.shape) != (D, Hp) or b1.numel() != Hp or b2.numel() != Hp or b3.numel() != D or not all(t.is_contiguous() for t in ts):
        raise _l.St355Error(f"{name}: expected contiguous W1 [Hp, D], b1 [Hp], W2 [Hp, Hp], b2 [Hp], W3 [D, Hp], b3 [D] with D = {D}, Hp = {Hp}")
    _al16(name, *ts)
    return D, Hp


def st_fold(W1, b1, W2, b2, W3, b3, W1h, W1T, b1h, W2h, W2T, b2h, W3h, W3T, b3h):
    """Self-Transcendence projector (st355_st_fold): ONE launch turns the six fp32 masters into the bf16 GEMM operands: W1h [Hp, D] and W1T [D, Hp], W2h / W2T
    [Hp, Hp], b1h / b2h [Hp], and — P3 = W3T.shape[1] <= D, the columns of the projection that are read — the first P3 rows of W3h [D, Hp], the compact
    W3T [Hp, P3] and the first P3 of b3h [D].  Nothing behind row P3 of W3h / element P3 of b3h is written.  Writes into the tensors given."""
    L = _l.load()
    D, Hp = _st_params("st_fold", W1, b1, W2, b2, W3, b3)
    outs = (W1h, W1T, b1h, W2h, W2T, b2h, W3h, W3T, b3h)
    for t in outs:
        _chk(t, BF16, "st_fold")
    P3 = W3T.shape[1] if W3T.dim() == 2 else 0
    if P3 <= 0 or P3 % 8 or P3 > D:
        raise _l.St355Error(f"st_fold: W3T [Hp, P3] must have 0 < P3 <= D columns, a multiple of 8 (got {tuple(W3T.shape)})")
    if not all(t.is_contiguous() for t in outs) or tuple(W1h.shape) != (Hp, D) or tuple(W1T.shape) != (D, Hp) or tuple(W2h.shape) != (Hp, Hp) \
            or tuple(W2T.shape) != (Hp, Hp) or tuple(W3h.shape) != (D, Hp) or tuple(W3T.shape) != (Hp, P3) or b1h.numel() != Hp or b2h.numel() != Hp or b3h.numel() != D:
        raise _l.St355Error(f"st_fold: expected contiguous W1h [Hp, D], W1T [D, Hp], b1h [Hp], W2h [Hp, Hp], W2T [Hp, Hp], b2h [Hp], W3h [D, Hp], W3T [Hp, P3], b3h [D] "
                            f"with D = {D}, Hp = {Hp}")
    _al16("st_fold", *outs)
    _l.check(L.st355_st_fold(_stream(), *(_ptr(t) for t in (W1, b1, W2, b2, W3, b3)), *(_ptr(t) for t in outs), D, Hp, P3), "st_fold")
    return outs


def _st_loss_operands(name: str, pred, sigmas, tmin, tmax, B: int, S: int, Pc: int, per_sample, stats):
    _chk(pred, BF16, "pred"); _chk(sigmas, F32, "sigmas"); _chk(per_sample, F32, "per_sample"); _chk(stats, F32, "stats")
    if not float(tmin) <= float(tmax):
        raise _l.St355Error(f"{name}: the timestep range must satisfy min <= max (got {tmin}, {tmax})")
    if tuple(pred.shape) != (B * S, Pc) or not pred.is_contiguous() or Pc % 8:
        raise _l.St355Error(f"{name}: expected contiguous pred [{B * S}, {Pc}] bf16 with a multiple of 8 columns, got {tuple(pred.shape)}")
    if sigmas.numel() != B or per_sample.numel() != B or stats.numel() != 3 or not (sigmas.is_contiguous() and per_sample.is_contiguous() and stats.is_contiguous()):
        raise _l.St355Error(f"{name}: expected contiguous sigmas [{B}], per_sample [{B}] and stats [3] fp32")
    if B > 4096:
        raise _l.St355Error(f"{name}: at most 4096 samples (got {B})")
    _al16(name, pred)


def st_vae_loss(pred, target, grid, sigmas, tmin: float, tmax: float, per_sample, stats):
    """Self-Transcendence stage `vae` (st355_st_vae_loss): pred [B * S, P] compact bf16 against the diffusion target [B, C, H, W] (bf16 or fp32) read in place on the
    gh x gw token grid (grid = (gh, gw), gh * gw == S; P = C (H / gh) (W / gw), columns in (c, a, e) order).  per_sample [B] = the per-sample means of (pred - t)^2;
    sample b is active iff tmin <= sigmas[b] <= tmax (on the device); stats [3] = (the mean of the active samples' means or 0, their count, 1 / (count S P) or 0);
    pred <- G = 2 (pred - t) of an active sample, exactly 0 otherwise.  Nothing is read on the host."""
    L = _l.load()
    _dev(target, "target")
    if target.dtype not in (BF16, F32) or target.dim() != 4:
        raise _l.St355Error(f"st_vae_loss: expected the target [B, C, H, W] in bf16 or fp32, got {tuple(target.shape)} {target.dtype}")
    B, Cc, H, W = target.shape
    gh, gw = (int(v) for v in grid)
    if gh <= 0 or gw <= 0 or H % gh or W % gw:
        raise _l.St355Error(f"st_vae_loss: the token grid {(gh, gw)} does not divide the latent shape {(H, W)}")
    S, P = gh * gw, Cc * (H // gh) * (W // gw)
    if not target[0].is_contiguous() or (B > 1 and target.stride(0) < Cc * H * W):
        raise _l.St355Error(f"st_vae_loss: every sample of the target must be contiguous, samples at least C * H * W elements apart (strides {target.stride()})")
    _st_loss_operands("st_vae_loss", pred, sigmas, tmin, tmax, B, S, P, per_sample, stats)
    ws = _scratch("st_loss", pred.device, L.st355_st_loss_workspace(B, S * P))
    _l.check(L.st355_st_vae_loss(_stream(), _ptr(pred), _ptr(target), int(target.dtype == BF16), target.stride(0) if B > 1 else Cc * H * W, _ptr(sigmas), float(tmin),
                                 float(tmax), B, S, Cc, H, W, gh, gw, _ptr(per_sample), _ptr(stats), _ptr(ws)), "st_vae_loss")
    return stats


def st_cfg_loss(pred, capture, cfg_scale: float, sigmas, tmin: float, tmax: float, per_sample, stats):
    """Self-Transcendence stage `self` (st355_st_cfg_loss): pred [B * S, D] compact bf16 against u + cfg_scale (c - u) formed in fp32, c = capture[:B], u = capture[B:]
    of the teacher's [2B, S, D] bf16 capture (a view: unit inner stride, strides multiples of 8).  Outputs as st_vae_loss."""
    L = _l.load()
    B2, S, D, ld, bs = _token_view(capture, "capture")
    if B2 % 2 or B2 == 0:
        raise _l.St355Error(f"st_cfg_loss: the capture holds the conditional rows, then the unconditional rows: an even batch (got {B2})")
    B = B2 // 2
    if D % 8 or ld % 8 or bs % 8 or (B2 > 1 and bs < S * ld):
        raise _l.St355Error(f"st_cfg_loss: D and the capture's strides must be multiples of 8 elements (got D = {D}, strides {capture.stride()})")
    _st_loss_operands("st_cfg_loss", pred, sigmas, tmin, tmax, B, S, D, per_sample, stats)
    cond, unc = capture[:B], capture[B:]
    _al16("st_cfg_loss", cond, unc)
    ws = _scratch("st_loss", pred.device, L.st355_st_loss_workspace(B, S * D))
    _l.check(L.st355_st_cfg_loss(_stream(), _ptr(pred), _ptr(cond), _ptr(unc), ld, bs, float(cfg_scale), _ptr(sigmas), float(tmin), float(tmax), B, S, D,
                                 _ptr(per_sample), _ptr(stats), _ptr(ws)), "st_cfg_loss")
    return stats


def st_wgrad(P, db, scale, g_W, g_b, accumulate: bool = False):
    """gradients of one of the projector's Linears (st355_st_wgrad): g_W [R, Cc] fp32 = s P (P bf16 = dY^T A, gemm_tn), g_b [R] fp32 = s db (db fp32 = colsum(dY),
    colsum_prod); s ONE fp32 on the device (the upstream gradient times the loss kernel's normaliser).  accumulate adds to what the gradients hold."""
    L = _l.load()
    _chk(P, BF16, "P"); _chk(db, F32, "db"); _chk(g_W, F32, "g_W"); _chk(g_b, F32, "g_b")
    _nextlat_scale("st_wgrad", scale)
    if P.dim() != 2 or P.shape[1] % 8:
        raise _l.St355Error(f"st_wgrad: expected P [R, Cc] with Cc a multiple of 8, got {tuple(P.shape)}")
    R, Cc = P.shape
    if tuple(g_W.shape) != (R, Cc) or db.numel() != R or g_b.numel() != R or not all(t.is_contiguous() for t in (P, db, g_W, g_b)):
        raise _l.St355Error(f"st_wgrad: expected contiguous P [{R}, {Cc}] bf16, db [{R}] fp32, g_W [{R}, {Cc}], g_b [{R}] fp32")
    _al16("st_wgrad", P, g_W)
    _l.check(L.st355_st_wgrad(_stream(), _ptr(P), _ptr(db), _ptr(scale), _ptr(g_W), _ptr(g_b), R, Cc, 1 if accumulate else 0), "st_wgrad")
    return g_W, g_b


def st_dx_add(g, scale, dx):
    """the projector's input gradient into the dX chain (st355_st_dx_add): dx, a [B, rows, D] bf16 view, = bf16(float(dx) + s g), g [B * rows, D] compact bf16,
    s ONE fp32 on the device.  In place."""
    L = _l.load()
    B, rows, D, ld, bs = _token_view(dx, "dx")
    _chk(g, BF16, "g")
    _nextlat_scale("st_dx_add", scale)
    if D % 8 or ld % 8 or bs % 8 or (B > 1 and bs < rows * ld):
        raise _l.St355Error(f"st_dx_add: D and the view's strides must be multiples of 8 elements (got D = {D}, strides {dx.stride()})")
    if tuple(g.shape) != (B * rows, D) or not g.is_contiguous():
        raise _l.St355Error(f"st_dx_add: expected contiguous g [{B * rows}, {D}]")
    _al16("st_dx_add", g, dx)
    _l.check(L.st355_st_dx_add(_stream(), _ptr(g), _ptr(scale), _ptr(dx), B, rows, D, ld, bs), "st_dx_add")
    return dx


def lora_pack(A, Bm, scale: float, A_cat, A_cat_T, B_blk, B_blk_T, k2_off: int = 0, n_off: int = 0):
    """write one adapter (A [r,K], B [N,r], fp32) into the block-structured bf16 operands of a fused projection group"""
    L = _l.load()
    _chk(A, F32, "A"); _chk(Bm, F32, "B")
    r, K = A.shape
    N = Bm.shape[0]
    K2 = A_cat.shape[0]
    N_total = B_blk.shape[0]
    if A_cat.shape != (K2, K) or A_cat_T.shape != (K, K2) or B_blk.shape != (N_total, K2) or B_blk_T.shape != (K2, N_total):
        raise _l.St355Error("lora_pack: operand shapes inconsistent")
    for t in (A_cat, A_cat_T, B_blk, B_blk_T):
        if not t.is_contiguous():
            raise _l.St355Error("lora_pack: packed operands must be contiguous")
    _l.check(L.st355_lora_pack(_stream(), _ptr(A.contiguous()), _ptr(Bm.contiguous()), r, K, N, scale, _ptr(A_cat), _ptr(A_cat_T),
                               _ptr(B_blk), _ptr(B_blk_T), K2, k2_off, N_total, n_off), "lora_pack")


def adamw_bf16_sr_step(p, g, m, v, shift, step: int, lr: float, beta1: float, beta2: float, eps: float, seg_end=None, seg_decay=None,
                       rand_bits=None, seed: int = 0, offset: int = 0, grad_scale: float = 1.0):
    """AdamWBF16.step over flat bf16 arenas (p, exp_avg, exp_avg_sq, shift updated in place).  seg_end int64 / seg_decay fp32 device
    arrays describe the parameter tensors inside the arena and the decay released for each this step; rand_bits int32 [4, n] injects the
    stochastic-rounding draws (tests), else in-kernel Philox."""
    L = _l.load()
    for t, nm in ((p, "p"), (g, "g"), (m, "exp_avg"), (v, "exp_avg_sq"), (shift, "shift")):
        _chk(t, BF16, nm)
        if not t.is_contiguous() or t.numel() != p.numel():
            raise _l.St355Error(f"adamw_bf16_sr_step: {nm} must be a contiguous arena of the same length")
    nseg = 0
    if seg_end is not None:
        if seg_end.dtype != torch.int64 or seg_decay.dtype != F32 or seg_end.numel() != seg_decay.numel():
            raise _l.St355Error("adamw_bf16_sr_step: seg_end must be int64 and seg_decay fp32, same length")
        _dev(seg_end, "seg_end"); _dev(seg_decay, "seg_decay")
        nseg = seg_end.numel()
    if rand_bits is not None:
        if rand_bits.dtype != torch.int32 or rand_bits.numel() != 4 * p.numel() or not rand_bits.is_contiguous():
            raise _l.St355Error("adamw_bf16_sr_step: rand_bits must be a contiguous int32 [4, n] tensor")
        _dev(rand_bits, "rand_bits")
    _l.check(L.st355_adamw_bf16_sr_step(_stream(), _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(shift), p.numel(), int(step), float(lr),
                                        float(beta1), float(beta2), float(eps), _ptr(seg_end), _ptr(seg_decay), nseg, _ptr(rand_bits),
                                        int(seed), int(offset), float(grad_scale)), "adamw_bf16_sr_step")


# ------------------------------------------------------------------------------------------------
# profiler
# ------------------------------------------------------------------------------------------------
def prof_enable(on: bool):
    _l.load().st355_prof_enable(1 if on else 0)


def prof_reset():
    _l.load().st355_prof_reset()


def prof_dump(path: str):
    """one CSV line per recorded launch (class index, ms, algorithmic flops / bytes, shape tag)"""
    _l.check(_l.load().st355_prof_dump(str(path).encode()), "prof_dump")


def prof_collect():
    n = len(_l.KERNEL_CLASSES)
    ms = (C.c_double * n)(); la = (C.c_int64 * n)(); fl = (C.c_double * n)(); by = (C.c_double * n)()
    _l.load().st355_prof_collect(ms, la, fl, by, n)
    return {k: {"ms": ms[i], "launches": la[i], "flops": fl[i], "bytes": by[i]} for i, k in enumerate(_l.KERNEL_CLASSES)}


# ------------------------------------------------------------------------------------------------
# UNet path: grid buffers, convolution-as-GEMM, GroupNorm, GEGLU, affine LayerNorm, cross-attention
# ------------------------------------------------------------------------------------------------
def grid_rows(B: int, H: int, W: int) -> int:
    return int(_l.load().st355_conv_grid_rows(B, H, W))


def grid_zeros(B: int, H: int, W: int, C_: int, device, pool: bool = False):
    """a zero-filled grid buffer [grid_rows, C] (border + 64 tail rows stay zero: kernels never write them non-zero)"""
    return torch.zeros(grid_rows(B, H, W), C_, dtype=BF16, device=device)


def _grid_out(B: int, H: int, W: int, C_: int, device, conv: bool = False):
    """output buffer of a grid kernel WITHOUT the full zero-fill pass: only the rows the kernel does not write are zeroed —
    the 64 tail rows for the layout kernels (they write every grid position, borders as zero), plus the first / last W+3 border positions for
    st355_conv_bf16 (its GEMM covers rows [W+3, rows - W - 3))."""
    n = B * (H + 2) * (W + 2)
    t = torch.empty(n + 64, C_, dtype=BF16, device=device)
    if conv:
        t[:W + 3].zero_()
        t[n - (W + 3):].zero_()
    else:
        t[n:].zero_()
    return t


def grid_from_nchw(x, Cpad: int):
    L = _l.load()
    _chk(x, BF16, "x")
    B, Cn, H, W = x.shape
    g = _grid_out(B, H, W, Cpad, x.device)
    _l.check(L.st355_grid_from_nchw(_stream(), _ptr(x.contiguous()), _ptr(g), B, Cn, H, W, Cpad), "grid_from_nchw")
    return g


def grid_to_nchw(g, B: int, Cn: int, H: int, W: int):
    L = _l.load()
    _chk(g, BF16, "grid")
    y = torch.empty(B, Cn, H, W, dtype=BF16, device=g.device)
    _l.check(L.st355_grid_to_nchw(_stream(), _ptr(g), _ptr(y), B, Cn, H, W, g.shape[1]), "grid_to_nchw")
    return y


def conv(x, w, B: int, H: int, W: int, bias=None, img_add=None, residual=None, taps: int = 9, out=None):
    """grid conv (3x3 stride 1 pad 1 for taps=9; 1x1 / pre-gathered columns for taps=1).  x: grid [.., Cin]; w: [Cout, taps*Cin]"""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(w, BF16, "w")
    Cin = x.shape[1]
    Cout = w.shape[0]
    if w.shape[1] != taps * Cin or not w.is_contiguous() or not x.is_contiguous():
        raise _l.St355Error(f"conv: weight {tuple(w.shape)} does not match taps*Cin = {taps}*{Cin} (or non-contiguous operands)")
    if x.shape[0] != grid_rows(B, H, W):
        raise _l.St355Error(f"conv: x has {x.shape[0]} rows, a ({B},{H},{W}) grid has {grid_rows(B, H, W)}")
    if out is None:
        out = _grid_out(B, H, W, Cout, x.device, conv=True)
    if bias is not None:
        _chk(bias, BF16, "bias")
    if img_add is not None:
        _chk(img_add, BF16, "img_add")
    if residual is not None:
        _chk(residual, BF16, "residual")
    _l.check(L.st355_conv_bf16(_stream(), _ptr(x), _ptr(w), _ptr(bias), _ptr(img_add), _rows(img_add, "img_add") if img_add is not None else 0,
                               _ptr(residual), _ptr(out), B, H, W, Cin, Cout, taps), "conv_bf16")
    return out


def conv_wgrad(x, dy, dw, B: int, H: int, W: int, taps: int = 9, accumulate: bool = False):
    L = _l.load()
    _chk(x, BF16, "x"); _chk(dy, BF16, "dy"); _chk(dw, BF16, "dw")
    Cin, Cout = x.shape[1], dy.shape[1]
    if tuple(dw.shape) != (Cout, taps * Cin) or not dw.is_contiguous():
        raise _l.St355Error(f"conv_wgrad: dw must be a contiguous [{Cout}, {taps * Cin}] tensor")
    ws = _gemm_workspace(x.device)
    _l.check(L.st355_conv_wgrad_bf16(_stream(), _ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cin, Cout, taps, 1 if accumulate else 0, _ptr(ws),
                                     ws.numel()), "conv_wgrad_bf16")
    return dw


def conv_plan(B: int, H: int, W: int, Cin: int, Cout: int, taps: int = 9, residual: bool = False):
    """st355_conv_plan, forward: what conv() would launch for this shape, without launching.  {"kernel": "pq_conv" | "s2", "epilogue": "NONE" | "ADD",
    "tiles", "dead": 64-column wave groups of the last column tile that issue no MFMAs}"""
    d = (C.c_int64 * 8)(B, H, W, Cin, Cout, taps, 1 if residual else 0, 0)
    out = (C.c_int32 * 8)()
    _l.check(_l.load().st355_conv_plan(1, d, out), "conv_plan")
    return {"kernel": {1: "pq_conv", 2: "s2"}[out[0]], "epilogue": {EPI_NONE: "NONE", EPI_ADD: "ADD"}[out[1]], "tiles": int(out[2]), "dead": int(out[3])}


def conv_wgrad_plan(B: int, H: int, W: int, Cin: int, Cout: int, taps: int = 9, accumulate: bool = False, workspace_bytes: int = -1):
    """st355_conv_plan, weight gradient: what conv_wgrad() would launch.  workspace_bytes: -1 = the workspace conv_wgrad() passes on the current device.
    {"taps": 9 | 1, "tiles", "ks": K-slices (1 = direct store), "Mc": rounded contraction rows, "store": "SPLITK" | "NONE" | "ADD"}"""
    if workspace_bytes < 0:
        workspace_bytes = _gemm_workspace(torch.device("cuda", torch.cuda.current_device())).numel()
    d = (C.c_int64 * 8)(B, H, W, Cin, Cout, taps, 1 if accumulate else 0, workspace_bytes)
    out = (C.c_int32 * 8)()
    _l.check(_l.load().st355_conv_plan(2, d, out), "conv_plan")
    ks = int(out[2])
    return {"taps": int(out[0]), "tiles": int(out[1]), "ks": ks, "Mc": int(out[3]), "store": "SPLITK" if ks >= 2 else {EPI_NONE: "NONE", EPI_ADD: "ADD"}[out[4]]}


def im2col3x3(x, B: int, H: int, W: int, stride: int = 1, pad: int = 1):
    L = _l.load()
    _chk(x, BF16, "x")
    Cn = x.shape[1]
    Kpad = (9 * Cn + 63) // 64 * 64
    col = _grid_out(B, H // stride, W // stride, Kpad, x.device)
    _l.check(L.st355_im2col3x3(_stream(), _ptr(x), _ptr(col), B, H, W, Cn, stride, Kpad, pad), "im2col3x3")
    return col


def col2im3x3(dcol, B: int, H: int, W: int, Cn: int, stride: int = 1, pad: int = 1):
    L = _l.load()
    _chk(dcol, BF16, "dcol")
    dx = _grid_out(B, H, W, Cn, dcol.device)
    _l.check(L.st355_col2im3x3(_stream(), _ptr(dcol), _ptr(dx), B, H, W, Cn, stride, dcol.shape[1], pad), "col2im3x3")
    return dx


def upsample2x(x, B: int, H: int, W: int):
    L = _l.load()
    _chk(x, BF16, "x")
    y = _grid_out(B, 2 * H, 2 * W, x.shape[1], x.device)
    _l.check(L.st355_upsample2x(_stream(), _ptr(x), _ptr(y), B, H, W, x.shape[1]), "upsample2x")
    return y


def upsample2x_bwd(dy, B: int, H: int, W: int):
    L = _l.load()
    _chk(dy, BF16, "dy")
    dx = _grid_out(B, H, W, dy.shape[1], dy.device)
    _l.check(L.st355_upsample2x_bwd(_stream(), _ptr(dy), _ptr(dx), B, H, W, dy.shape[1]), "upsample2x_bwd")
    return dx


BLOCK_CALLS = {}          # block-level entry point -> how often it ran (the GPU suite asserts that the engines really take them)


def _fill(st, **kw):
    """tensors -> device pointers, None -> NULL, numbers as they are"""
    keep = []
    names = {f[0] for f in type(st)._fields_}
    for k, v in kw.items():
        if k not in names:
            raise _l.St355Error(f"{type(st).__name__}: no field {k!r} (include/st355.h)")
        if torch.is_tensor(v):
            _dev(v, k)
            keep.append(v)
            v = v.data_ptr()
        setattr(st, k, v)
    st._keep = keep
    return st


def _block_call(name: str, a):
    """st355_<name>(stream, &a), checked and counted in BLOCK_CALLS[name]"""
    _l.check(getattr(_l.load(), "st355_" + name)(_stream(), C.byref(a)), name)
    BLOCK_CALLS[name] = BLOCK_CALLS.get(name, 0) + 1


def block_flux_single_fwd(**kw):
    """st355_block_flux_single_fwd: one FluxSingleTransformerBlock forward as ONE C call (field names of st355_flux_single_fwd_args)"""
    ws = _gemm_workspace(kw["x"].device)
    _block_call("block_flux_single_fwd", _fill(_l.FluxSingleFwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), **kw))


def block_flux_double_fwd(**kw):
    """st355_block_flux_double_fwd: one FluxTransformerBlock forward as ONE C call (field names of st355_flux_double_fwd_args)"""
    ws = _gemm_workspace(kw["img"].device)
    _block_call("block_flux_double_fwd", _fill(_l.FluxDoubleFwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), **kw))


def block_flux_double_bwd(grads, **kw):
    """st355_block_flux_double_bwd (field names of st355_flux_double_bwd_args); grads: {"gA_qkv": [...], "gB_qkv": [...], "gA_out": [...], "gB_out": [...]}"""
    dev = kw["img"].device
    B, S, H, D = kw["B"], kw["Si"] + kw["St"], kw["H"], kw["D"]
    ws = _gemm_workspace(dev)
    aws = _attn_bwd_scratch(dev, B, H, S, S, 128)
    sws = _skinny_scratch(dev, B * kw["Si"], D, 128) if kw.get("K2_qkv") or kw.get("K2_out") else None
    a = _fill(_l.FluxDoubleBwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), attn_ws=aws, skinny_ws=sws, **kw)
    for name, ts in (grads or {}).items():
        arr = getattr(a, name)
        for i, t in enumerate(ts or []):
            _chk(t, F32, name); arr[i] = t.data_ptr()
    _block_call("block_flux_double_bwd", a)


def block_flux_single_bwd(gA, gB, **kw):
    """st355_block_flux_single_bwd (field names of st355_flux_single_bwd_args); gA / gB: lists of the adapters' fp32 gradient views"""
    dev = kw["x"].device
    B, S, H, D = kw["B"], kw["S"], kw["H"], kw["D"]
    ws = _gemm_workspace(dev)
    aws = _attn_bwd_scratch(dev, B, H, S, S, 128)
    sws = _skinny_scratch(dev, B * S, D, 128) if kw.get("K2") else None
    a = _fill(_l.FluxSingleBwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), attn_ws=aws, skinny_ws=sws, **kw)
    for i, t in enumerate(gA or []):
        _chk(t, F32, "gA"); a.gA[i] = t.data_ptr()
    for i, t in enumerate(gB or []):
        _chk(t, F32, "gB"); a.gB[i] = t.data_ptr()
    _block_call("block_flux_single_bwd", a)


def block_pixart_fwd(**kw):
    """st355_block_pixart_fwd: one PixArt BasicTransformerBlock(ada_norm_single) forward as ONE C call (field names of st355_pixart_block_fwd_args)"""
    _block_call("block_pixart_fwd", _fill(_l.PixartBlockFwdArgs(), **kw))


def block_pixart_bwd(**kw):
    """st355_block_pixart_bwd: the data path of that block's backward as ONE C call (field names of st355_pixart_block_bwd_args)"""
    aws = _attn_bwd_scratch(kw["h"].device, kw["B"], kw["H"], kw["S"], (kw["S"] + 63) // 64 * 64, kw["d_pad"])
    _block_call("block_pixart_bwd", _fill(_l.PixartBlockBwdArgs(), attn_ws=aws, **kw))


def block_sd3_joint_fwd(**kw):
    """st355_block_sd3_joint_fwd: one SD3 JointTransformerBlock forward as ONE C call (field names of st355_sd3_joint_fwd_args)"""
    ws = _gemm_workspace(kw["img"].device)
    _block_call("block_sd3_joint_fwd", _fill(_l.Sd3JointFwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), **kw))


def block_sd3_joint_bwd(**kw):
    """st355_block_sd3_joint_bwd: the data path of that block's backward as ONE C call (field names of st355_sd3_joint_bwd_args)"""
    dev = kw["img"].device
    S = kw["Si"] + kw["St"]
    aws = _attn_bwd_scratch(dev, kw["B"], kw["H"], S, (S + 63) // 64 * 64, kw["hd"])
    ws = _gemm_workspace(dev)
    if kw.get("dmod_img") is not None:          # the fused-statistics form (full fine-tune): fp32 partial rows of its column sums
        rmax = max(kw["Si"], kw["St"])
        kw["stats_ws"] = _scratch("stats", dev, _l.load().st355_stats_workspace(kw["B"] * rmax, 4 * kw["D"], rmax, 1))
    _block_call("block_sd3_joint_bwd", _fill(_l.Sd3JointBwdArgs(), gemm_ws=ws, gemm_ws_bytes=ws.numel(), attn_ws=aws, **kw))


class VaeEncoderTable:
    """the architecture + device-pointer table st355_vae_encode walks (include/st355.h lists the order); keeps the tensors alive"""

    def __init__(self, in_channels: int, latent_channels: int, block_out_channels, layers_per_block: int, norm_num_groups: int, tensors):
        self.tensors = list(tensors)
        for t in self.tensors:
            _chk(t, BF16, "vae tensor")
            if not t.is_contiguous():
                raise _l.St355Error("vae_encode: table tensors must be contiguous")
        n = len(self.tensors)
        self._ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in self.tensors])
        st = _l.VaeEncoder()
        st.in_channels, st.latent_channels, st.n_levels, st.layers_per_block, st.norm_num_groups = in_channels, latent_channels, len(block_out_channels), layers_per_block, norm_num_groups
        for i, c in enumerate(block_out_channels):
            st.block_out_channels[i] = int(c)
        st.n_tensors, st.tensors = n, C.cast(self._ptrs, C.POINTER(C.c_void_p))
        self.struct = st


def vae_encode(table: VaeEncoderTable, x):
    """AutoencoderKL.encode as one C call: pixels [B, C, H, W] bf16 -> moments [B, 2L, H/2^(n-1), W/2^(n-1)] bf16"""
    L = _l.load()
    _chk(x, BF16, "x")
    x = x.contiguous()
    B, _, H, W = x.shape
    st = table.struct
    f = 1 << (st.n_levels - 1)
    need = L.st355_vae_encode_workspace(C.byref(st), B, H, W)
    if need == 0:
        raise _l.St355Error("vae_encode: " + L.st355_last_error().decode("utf-8", "replace"))
    ws = _scratch("vae_encode", x.device, need)
    out = torch.empty(B, 2 * st.latent_channels, H // f, W // f, dtype=BF16, device=x.device)
    _l.check(L.st355_vae_encode(_stream(), C.byref(st), _ptr(x), _ptr(out), B, H, W, _ptr(ws), ws.numel()), "vae_encode")
    return out


def tokens_to_grid(tokens, B: int, H: int, W: int, residual=None):
    L = _l.load()
    _chk(tokens, BF16, "tokens")
    if tokens.shape[0] != B * H * W or not tokens.is_contiguous():          # st355_tokens_to_grid takes no row stride
        raise _l.St355Error("tokens_to_grid: tokens must be a dense [B*H*W, C] tensor")
    g = _grid_out(B, H, W, tokens.shape[1], tokens.device)
    _l.check(L.st355_tokens_to_grid(_stream(), _ptr(tokens), _ptr(residual), _ptr(g), B, H, W, tokens.shape[1]), "tokens_to_grid")
    return g


def grid_to_tokens(g, B: int, H: int, W: int):
    L = _l.load()
    _chk(g, BF16, "grid")
    t = torch.empty(B * H * W, g.shape[1], dtype=BF16, device=g.device)
    _l.check(L.st355_grid_to_tokens(_stream(), _ptr(g), _ptr(t), B, H, W, g.shape[1]), "grid_to_tokens")
    return t


def _gn_workspace(B, H, W, Cn, device):
    return _scratch("groupnorm", device, _l.load().st355_groupnorm_workspace(B, H, W, Cn))


def gn_set_apply(form: int) -> int:
    """st355_gn_set_apply: GroupNorm apply form for the calls that follow, 2 = row-walking passes (default), 1 = flat-index passes, -1 = the initial form
    (ST355_GN_APPLY), 0 = unchanged; returns the previous form"""
    return int(_l.load().st355_gn_set_apply(int(form)))


NORM_PLAN_KINDS = {"ln": 1, "ln_params": 2, "ln_stats": 3, "cols": 4, "gn": 5, "qk": 6}      # ST355_NORM_PLAN_* (st355.h)


def norm_plan(kind: str, *dims):
    """st355_norm_plan: the instance a normalisation / token-sum entry point would run for this shape, without launching anything.
    ln (D) -> {"nc"}; ln_params (D) -> {"nc"}; ln_stats (D, rows_per_batch, gs) -> {"nc", "gs", "chunks"}; cols (rows_per_batch) -> {"chunks"};
    gn (B, H, W, C) -> {"form", "nch", "rows_per_chunk", "nwin", "cw", "RT"}; qk (d, B, H, S_part) -> {"hd", "nblk", "ns", "per"}"""
    keys = {"ln": ("nc",), "ln_params": ("nc",), "ln_stats": ("nc", "gs", "chunks"), "cols": ("chunks",),
            "gn": ("form", "nch", "rows_per_chunk", "nwin", "cw", "RT"), "qk": ("hd", "nblk", "ns", "per")}[kind]
    d = (C.c_int64 * 8)(*[int(v) for v in dims])
    out = (C.c_int32 * 8)()
    _l.check(_l.load().st355_norm_plan(NORM_PLAN_KINDS[kind], d, out), "norm_plan")
    return {k: int(out[i]) for i, k in enumerate(keys)}


def groupnorm_fwd(x, gamma, beta, B: int, H: int, W: int, groups: int = 32, eps: float = 1e-5, silu: bool = True, out_tokens: bool = False):
    """returns (y, stats).  y: grid [.., C] or dense tokens [B*H*W, C]; stats [B,C,2] fp32 for the backward"""
    L = _l.load()
    _chk(x, BF16, "x"); _chk(gamma, BF16, "gamma"); _chk(beta, BF16, "beta")
    Cn = x.shape[1]
    y = torch.empty(B * H * W, Cn, dtype=BF16, device=x.device) if out_tokens else _grid_out(B, H, W, Cn, x.device)
    stats = torch.empty(B, Cn, 2, dtype=F32, device=x.device)
    _l.check(L.st355_groupnorm_fwd(_stream(), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(stats), B, H, W, Cn, groups, eps, 1 if silu else 0,
                                   1 if out_tokens else 0, _ptr(_gn_workspace(B, H, W, Cn, x.device))), "groupnorm_fwd")
    return y, stats


def groupnorm_bwd(dy, x, gamma, beta, stats, B: int, H: int, W: int, groups: int = 32, silu: bool = True, dy_tokens: bool = False, dadd=None,
                  dgamma=None, dbeta=None, accumulate_params: bool = False):
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x"); _chk(stats, F32, "stats")
    Cn = x.shape[1]
    if dy_tokens and (tuple(dy.shape) != (B * H * W, Cn) or not dy.is_contiguous()):          # st355_groupnorm_bwd takes no row stride
        raise _l.St355Error("groupnorm_bwd: dy_tokens must be a dense [B*H*W, C] tensor")
    dx = _grid_out(B, H, W, Cn, x.device)
    _l.check(L.st355_groupnorm_bwd(_stream(), _ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(dadd), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                   B, H, W, Cn, groups, 1 if silu else 0, 1 if dy_tokens else 0, 1 if accumulate_params else 0,
                                   _ptr(_gn_workspace(B, H, W, Cn, x.device))), "groupnorm_bwd")
    return dx


def layernorm_fwd(x, weight, bias, eps: float = 1e-5, out=None):
    L = _l.load()
    _chk(x, BF16, "x"); _chk(weight, BF16, "weight"); _chk(bias, BF16, "bias")
    rows, D = x.shape
    if out is None:
        out = torch.empty(rows, D, dtype=BF16, device=x.device)
    _l.check(L.st355_layernorm_fwd(_stream(), _ptr(x), _rows(x, "x"), _ptr(weight), _ptr(bias), _ptr(out), _rows(out, "out"), rows, D, eps), "layernorm_fwd")
    return out


def layernorm_bwd(dy, x, weight, dres=None, eps: float = 1e-5):
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x"); _chk(weight, BF16, "weight")
    rows, D = x.shape
    dx = torch.empty(rows, D, dtype=BF16, device=x.device)
    _l.check(L.st355_layernorm_bwd(_stream(), _ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), _ptr(weight), _ptr(dres),
                                   _rows(dres, "dres") if dres is not None else 0, _ptr(dx), _rows(dx, "dx"), rows, D, eps), "layernorm_bwd")
    return dx


def layernorm_param_grads(dy, x, dweight, dbias, eps: float = 1e-5, accumulate: bool = False):
    L = _l.load()
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x"); _chk(dweight, F32, "dweight"); _chk(dbias, F32, "dbias")
    rows, D = x.shape
    ws = _scratch("layernorm_param_grads", x.device, L.st355_layernorm_param_grads_workspace(D))
    _l.check(L.st355_layernorm_param_grads(_stream(), _ptr(dy), _rows(dy, "dy"), _ptr(x), _rows(x, "x"), rows, D, eps, _ptr(dweight), _ptr(dbias),
                                           1 if accumulate else 0, _ptr(ws)), "layernorm_param_grads")


def geglu_fwd(h):
    L = _l.load()
    _chk(h, BF16, "h")
    M, F2 = h.shape
    out = torch.empty(M, F2 // 2, dtype=BF16, device=h.device)
    _l.check(L.st355_geglu_fwd(_stream(), _ptr(h), _rows(h, "h"), _ptr(out), M, F2 // 2), "geglu_fwd")
    return out


def geglu_bwd(h, dout):
    L = _l.load()
    _chk(h, BF16, "h"); _chk(dout, BF16, "dout")
    M, F2 = h.shape
    dh = torch.empty(M, F2, dtype=BF16, device=h.device)
    _l.check(L.st355_geglu_bwd(_stream(), _ptr(h), _rows(h, "h"), _ptr(dout.contiguous()), _ptr(dh), _rows(dh, "dh"), M, F2 // 2), "geglu_bwd")
    return dh


def head_split(src, B: int, H: int, d: int, S: int, want_x: bool = True, want_xt: bool = True, d_src: Optional[int] = None):
    """src: 2-D column-block view [B*S, H*d_src] (row stride free) -> (X [B,H,S,d] | None, Xt [B,H,d,Sp] | None, Sp); d_src < d: zero-padded heads"""
    L = _l.load()
    _chk(src, BF16, "src")
    Sp = (S + 63) // 64 * 64
    X = torch.empty(B, H, S, d, dtype=BF16, device=src.device) if want_x else None
    Xt = None
    if want_xt:                               # only the pad columns [S, Sp) need zeros: the kernel writes every column < S (a full-size fill per attention before r6)
        Xt = torch.empty(B, H, d, Sp, dtype=BF16, device=src.device)
        if Sp > S:
            Xt[..., S:].zero_()
    _l.check(L.st355_head_split_pad(_stream(), _ptr(src), _rows(src, "src"), _ptr(X), _ptr(Xt), B, H, d if d_src is None else d_src, d, S, Sp), "head_split")
    return X, Xt, Sp


def head_merge(dX, dst, B: int, H: int, d: int, S: int, d_src: Optional[int] = None):
    L = _l.load()
    _chk(dX, BF16, "dX"); _chk(dst, BF16, "dst")
    _l.check(L.st355_head_merge_pad(_stream(), _ptr(dX), _ptr(dst), _rows(dst, "dst"), B, H, d if d_src is None else d_src, d, S), "head_merge")
    return dst


def attn_cross_fwd(Q, K, Vt, O, lse2, B, H, Sq, Sk, Skp, d, scale: float, key_bias=None, O_res=None):
    L = _l.load()
    _chk(Q, BF16, "Q"); _chk(K, BF16, "K"); _chk(Vt, BF16, "Vt"); _chk(O, BF16, "O"); _chk(lse2, F32, "lse2")
    if O_res is not None:
        _res_ok(O, O_res)
        _l.check(L.st355_attn_fwd_res(_stream(), _ptr(Q), _ptr(K), _ptr(Vt), _ptr(key_bias), _ptr(O), _rows(O, "O"), _ptr(O_res), _ptr(lse2),
                                      B, H, Sq, Sk, Skp, d, scale), "attn_fwd_res")
        return
    _l.check(L.st355_attn_cross_fwd(_stream(), _ptr(Q), _ptr(K), _ptr(Vt), _ptr(key_bias), _ptr(O), _rows(O, "O"), _ptr(lse2),
                                    B, H, Sq, Sk, Skp, d, scale), "attn_cross_fwd")


def attn_cross_bwd(Q, K, Qt, Kt, v_rows, O, dO, lse2, dQ, dK, dv_rows, B, H, Sq, Sqp, Sk, Skp, d, scale: float, key_bias=None, O_res=None):
    L = _l.load()
    ws = _attn_bwd_scratch(Q.device, B, H, Sq, Sqp, d)
    if O_res is not None:
        _res_ok(O, O_res)
        _l.check(L.st355_attn_bwd_res(_stream(), _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(v_rows), _rows(v_rows, "v_rows"),
                                      _ptr(O), _rows(O, "O"), _ptr(O_res), _ptr(dO), _rows(dO, "dO"), _ptr(lse2), _ptr(key_bias),
                                      _ptr(dQ), _ptr(dK), _ptr(dv_rows), _rows(dv_rows, "dv_rows"), B, H, Sq, Sqp, Sk, Skp, d, scale, _ptr(ws)), "attn_bwd_res")
        return
    _l.check(L.st355_attn_cross_bwd(_stream(), _ptr(Q), _ptr(K), _ptr(Qt), _ptr(Kt), _ptr(v_rows), _rows(v_rows, "v_rows"),
                                    _ptr(O), _rows(O, "O"), _ptr(dO), _rows(dO, "dO"), _ptr(lse2), _ptr(key_bias),
                                    _ptr(dQ), _ptr(dK), _ptr(dv_rows), _rows(dv_rows, "dv_rows"), B, H, Sq, Sqp, Sk, Skp, d, scale, _ptr(ws)),
             "attn_cross_bwd")


def softmax_rows_(x, scale: float = 1.0):
    """in place: x[r, :] = softmax(scale * x[r, :]) over the last dim of a 2-D bf16 view"""
    L = _l.load()
    _chk(x, BF16, "x")
    _l.check(L.st355_softmax_rows(_stream(), _ptr(x), _rows(x, "x"), x.shape[0], x.shape[1], scale), "softmax_rows")
    return x


def softmax_rows_bwd_(p, dp, scale: float = 1.0):
    """in place on dp: ds = scale * p * (dp - rowsum(dp * p))"""
    L = _l.load()
    _chk(p, BF16, "p"); _chk(dp, BF16, "dp")
    if _rows(p, "p") != _rows(dp, "dp"):
        raise _l.St355Error("softmax_rows_bwd: p and dp must share a row stride")
    _l.check(L.st355_softmax_rows_bwd(_stream(), _ptr(p), _ptr(dp), _rows(dp, "dp"), p.shape[0], p.shape[1], scale), "softmax_rows_bwd")
    return dp

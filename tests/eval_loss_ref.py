"""Evaluation loss (eval_steps_interval) — TEST INFRASTRUCTURE ONLY.

  * the fp64 restatement of the two kernels' rules (csrc/eval_loss.hip): `views64`, `loss64`;
  * `dtype_chain`: the executed reference's chain from a grid timestep to (sigma, model timestep), restated with explicit roundings
    (tests/golden/eval_loss_vectors.pt records the reference's own results);
  * CPU stand-ins with the contract of the two `ops` wrappers (eval_flow_views, eval_loss), monkeypatched in next to tests/ops_emulator.py by the new tests:
    fp64 on the given operands, each output rounded once to its dtype.
"""
import torch

from tests import ops_emulator as EMU
from tests import twinflow_ref as TR

F32, F64 = torch.float32, torch.float64
LOSS_TYPES = ("l2", "huber", "smooth_l1")
MAX_STACK = 64


def views64(latents, noise, sigma):
    """[K, B, ...] fp64: (1 - sigma_k) x + sigma_k n on the given operands"""
    x, n = latents.detach().to(F64).cpu(), noise.detach().to(F64).cpu()
    s = sigma.detach().to(F64).cpu().reshape(-1, *([1] * x.dim()))
    return (1.0 - s) * x[None] + s * n[None]


def element64(d, loss_type, c):
    """the element loss on fp64 differences; c broadcastable to d"""
    if loss_type == "l2":
        return d * d
    root = torch.sqrt(d * d + c * c) - c
    return (2.0 * c if loss_type == "huber" else 2.0) * root


def loss64(pred, target, loss_type="l2", huber_c=None):
    """(loss [K], per_sample [K, B]) in fp64: element loss -> per-sample mean -> batch mean, per slab.  huber_c: K * B values (slab-major) or a float"""
    p, t = pred.detach().to(F64).cpu(), target.detach().to(F64).cpu()
    K, B = p.shape[0], t.shape[0]
    c = None
    if loss_type != "l2":
        c = (huber_c.detach().to(F64).cpu() if torch.is_tensor(huber_c) else torch.full((K * B,), float(torch.tensor(float(huber_c), dtype=F32)), dtype=F64))
        c = c.reshape(K, B, *([1] * (t.dim() - 1)))
    el = element64(p - t[None], loss_type, c)
    per = el.reshape(K, B, -1).mean(dim=2)
    return per.mean(dim=1), per


def dtype_chain(grid_timesteps, weight_dtype=torch.bfloat16, latents_dtype=torch.bfloat16, timesteps_dtype=F32, num_train_timesteps=1000.0):
    """(sigma in the latents' dtype, model timestep in the prepared timesteps' dtype), every rounding spelled out: the grid value rounds to the weight dtype; the
    sigma is that value / T rounded to the latents' dtype (a value of at most 1 is taken as a sigma), clamped to [0, 1]; the model's timestep is sigma * T rounded to
    the latents' dtype (the sigma itself for a value of at most 1), then carried in the timesteps' dtype"""
    t = grid_timesteps.detach().to(F64)
    t = t.to(weight_dtype).to(timesteps_dtype)
    s = t.to(latents_dtype)
    s = torch.where(s > 1.0, (s.to(F64) / num_train_timesteps).to(latents_dtype), s).clamp(0.0, 1.0)          # per grid value: at most 1 means "already a sigma"
    return s, torch.where(t.float() > 1.0, (s.to(F64) * num_train_timesteps).to(latents_dtype), s).to(timesteps_dtype)


# ---- the stand-ins (contract of simpletuner_amd.ops.eval_flow_views / eval_loss) ----
def eval_flow_views(latents, noise, sigma, out=None):
    EMU._need(latents.dtype == EMU.BF16 and noise.dtype == EMU.BF16 and sigma.dtype == F32, "eval_flow_views: bf16 latents / noise, fp32 sigma")
    B = latents.shape[0]
    K = sigma.numel()
    EMU._need(noise.shape == latents.shape and B > 0 and (latents.numel() // B) % 8 == 0 and latents.numel() > 0, "eval_flow_views: noise of latents' shape, N % 8 == 0")
    EMU._need(sigma.dim() == 1 and 1 <= K <= MAX_STACK, "eval_flow_views: 1 <= K <= 64")
    res = views64(latents, noise, sigma).to(EMU.BF16).to(latents.device)
    if out is None:
        return res
    EMU._need(out.dtype == EMU.BF16 and out.is_contiguous() and out.numel() == res.numel(), "eval_flow_views: out contiguous bf16 of K * latents.numel() elements")
    EMU._need(out.data_ptr() not in (latents.data_ptr(), noise.data_ptr()), "eval_flow_views: out must not overlap latents or noise")
    out.view(res.shape).copy_(res)
    return out


def eval_loss(pred, target, loss_type="l2", huber_c=0.1, loss_out=None):
    EMU._need(pred.dtype == EMU.BF16 and target.dtype == EMU.BF16 and loss_type in LOSS_TYPES, "eval_loss: bf16 pred / target, a known loss type")
    EMU._need(pred.dim() == target.dim() + 1 and tuple(pred.shape[1:]) == tuple(target.shape), "eval_loss: pred [K, *target.shape]")
    K, B = pred.shape[0], target.shape[0]
    EMU._need(1 <= K <= MAX_STACK and 0 < B < 65536 and (target.numel() // B) % 8 == 0 and target.numel() > 0, "eval_loss: 1 <= K <= 64, batch < 65536, N % 8 == 0")
    if loss_type != "l2" and torch.is_tensor(huber_c):
        EMU._need(huber_c.dtype == F32 and huber_c.numel() == K * B, "eval_loss: huber_c fp32 of K * B values")
    loss, per = loss64(pred, target, loss_type, huber_c)
    loss, per = loss.to(F32).to(pred.device), per.to(F32).to(pred.device)
    if loss_out is None:
        return loss, per
    EMU._need(loss_out.dtype == F32 and loss_out.is_contiguous() and loss_out.numel() == K, "eval_loss: loss_out contiguous fp32 [K]")
    loss_out.copy_(loss)
    return loss_out, per


STAND_INS = {"eval_flow_views": eval_flow_views, "eval_loss": eval_loss}


def install(monkeypatch):
    """the emulator and every earlier feature's stand-ins (tests.twinflow_ref.install) + the two evaluation-loss stand-ins"""
    ops = TR.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn, raising=False)          # (a tree without the wrappers still installs: its tests then fail on what they assert)
    monkeypatch.setattr(ops, "EVAL_MAX_STACK", MAX_STACK, raising=False)
    return ops

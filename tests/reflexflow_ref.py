"""Scheduled sampling / ReflexFlow — TEST INFRASTRUCTURE ONLY.

  * the fp64 restatement of the ReflexFlow loss (common.py:6287-6318, 6426-6429), once through differentiable torch operations (`loss64`: what autograd checks) and
    once in closed form with the gradient as the kernel computes it (`reflexflow64`), the stats and the Euler step;
  * CPU stand-ins with the contract of the three new `ops` wrappers (reflexflow_stats, reflexflow_loss, flow_euler_step), monkeypatched in next to
    tests/ops_emulator.py by the new tests: fp64 on the given operands, each output rounded once to its dtype.
"""
import torch

from tests import dora_ref as DR
from tests import ops_emulator as EMU

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6


def _flat(t, dtype=F64):
    return None if t is None else t.detach().to(dtype).reshape(t.shape[0], -1)


def _mask_full(emask, B, N, dtype=F64):
    if emask is None:
        return None
    m = emask.detach().to(dtype).reshape(B, -1)
    return m.repeat(1, N // m.shape[1])          # element i of a sample reads emask[b, i % period]: the [B, 1, H, W] mask broadcast over the channels


def element_loss(d, loss_type, c):
    """conditional_loss(reduction="none") on d = pred - target; c [B, 1]"""
    if loss_type == "l2":
        return d * d
    r = torch.sqrt(d * d + c * c)
    return (2 * c if loss_type == "huber" else 2.0) * (r - c)


def _huber(huber_c, B, dtype=F64):
    if torch.is_tensor(huber_c):
        return huber_c.detach().to(dtype).reshape(-1).expand(B).reshape(B, 1)
    return torch.full((B, 1), float(0.0 if huber_c is None else huber_c), dtype=dtype)


def loss64(pred, target, noisy, latents, clean, biased, loss_type="l2", huber_c=0.1, emask=None, alpha=1.0, beta1=10.0, beta2=1.0):
    """the reference's expression, operation for operation, on fp64 [B, N] tensors; differentiable in `pred`.  Returns (loss, per_sample, adr term)"""
    B, N = pred.shape
    l = element_loss(pred - target, loss_type, _huber(huber_c, B))
    if clean is not None and biased is not None and alpha != 0.0:
        e = (clean - biased).detach()
        l = l * (1.0 + alpha * e / e.abs().sum(1, keepdim=True).clamp_min(EPS))
    if beta2 != 1.0:
        l = l * beta2
    m = _mask_full(emask, B, N)
    if m is not None:
        l = l * m
    per = l.mean(1)
    term = torch.zeros(B, dtype=F64)
    if beta1 != 0.0:
        tau = noisy - latents
        t_dir = tau / torch.norm(tau, dim=1, keepdim=True).clamp_min(EPS)
        p_dir = pred / torch.norm(pred, dim=1, keepdim=True).clamp_min(EPS)
        term = beta1 * (p_dir - t_dir).pow(2).sum(1)
        per = per + term
    return per.mean(), per, term


def stats64(pred, noisy, latents, clean=None, biased=None):
    p, tau = _flat(pred), _flat(noisy) - _flat(latents)
    se = (_flat(clean) - _flat(biased)).abs().sum(1) if clean is not None else torch.zeros(p.shape[0], dtype=F64)
    return torch.stack([se, (p * p).sum(1), (tau * tau).sum(1), (p * tau).sum(1)], dim=1)


def reflexflow64(pred, target, noisy, latents, clean=None, biased=None, loss_type="l2", huber_c=0.1, emask=None, alpha=1.0, beta1=10.0, beta2=1.0, grad_scale=1.0,
                 stats=None):
    """closed form in fp64 on the given operands: dict(loss, per_sample, adr, dpred, stats).  `stats` given (fp32, a kernel's): the weight and the ADR term use
    them as the loss kernel does; else they are formed here."""
    p, t = _flat(pred), _flat(target)
    B, N = p.shape
    c = _huber(huber_c, B)
    d = p - t
    if loss_type == "l2":
        l, g = d * d, 2 * d
    else:
        r = torch.sqrt(d * d + c * c)
        k = 2 * c if loss_type == "huber" else torch.full_like(c, 2.0)
        l, g = k * (r - c), k * d / r
    st = stats64(pred, noisy, latents, clean, biased) if stats is None else stats.detach().to(F64).cpu()
    w = torch.full_like(p, float(beta2))
    m = _mask_full(emask, B, N)
    if m is not None:
        w = w * m
    if clean is not None and alpha != 0.0:
        w = w * (1.0 + alpha * (_flat(clean) - _flat(biased)) / st[:, 0:1].clamp_min(EPS))
    per = (l * w).sum(1) / N
    dpred = grad_scale * g * w / (N * B)
    adr = torch.zeros(B, dtype=F64)
    if beta1 != 0.0:
        tau = _flat(noisy) - _flat(latents)
        pnorm, tnorm = st[:, 1:2].sqrt(), st[:, 2:3].sqrt()
        pn, tn = pnorm.clamp_min(EPS), tnorm.clamp_min(EPS)
        u, th = p / pn, tau / tn
        q = u - th
        udot = torch.where(pnorm > EPS, st[:, 1:2] / (pn * pn) - st[:, 3:4] / (pn * tn), torch.zeros_like(pn))
        adr = beta1 * (q * q).sum(1)
        dpred = dpred + grad_scale * 2.0 * beta1 / (B * pn) * (q - u * udot)
    per = per + adr
    return dict(loss=per.mean(), per_sample=per, adr=adr, dpred=dpred.reshape(pred.shape), stats=st)


def euler64(x, v, dt):
    B = x.shape[0]
    return x.detach().to(F64) + dt.detach().to(F64).reshape(B, *([1] * (x.dim() - 1))) * v.detach().to(F64)


# ---- the stand-ins (contract of simpletuner_amd.ops.reflexflow_stats / reflexflow_loss / flow_euler_step) ----
def _rows(ts, names):
    for t, n in zip(ts, names):
        EMU._need(torch.is_tensor(t) and t.dtype == BF16 and t.shape == ts[0].shape, f"{n}: expected bf16 of {names[0]}'s shape")
    B = ts[0].shape[0]
    N = ts[0].numel() // B
    EMU._need(N % 8 == 0 and 0 < B < 65536, f"{names[0]}: per-sample size must be a multiple of 8, batch < 65536")
    return B, N


def reflexflow_stats(pred, noisy, latents, clean=None, biased=None):
    EMU._need((clean is None) == (biased is None), "reflexflow_stats: clean and biased come together or not at all")
    _rows([pred, noisy, latents] + ([clean, biased] if clean is not None else []), ["pred", "noisy", "latents", "clean", "biased"])
    return stats64(pred, noisy, latents, clean, biased).to(F32).to(pred.device)


def reflexflow_loss(pred, target, noisy, latents, stats, loss_type="l2", huber_c=0.1, clean=None, biased=None, alpha=1.0, beta1=10.0, beta2=1.0, want_grad=True,
                    grad_scale=1.0, emask=None):
    EMU._need((clean is None) == (biased is None), "reflexflow_loss: clean and biased come together or not at all")
    B, N = _rows([pred, target, noisy, latents] + ([clean, biased] if clean is not None else []), ["pred", "target", "noisy", "latents", "clean", "biased"])
    EMU._need(stats.dtype == F32 and tuple(stats.shape) == (B, 4), "stats: fp32 [B, 4]")
    EMU._need(loss_type in ("l2", "huber", "smooth_l1"), "loss_type")
    if emask is not None:
        period = emask.reshape(B, -1).shape[1]
        EMU._need(emask.dtype == F32 and period % 8 == 0 and N % period == 0, "emask: fp32 [B, period], period a multiple of 8 dividing the per-sample size")
    r = reflexflow64(pred, target, noisy, latents, clean, biased, loss_type, huber_c if loss_type != "l2" else None, emask, float(alpha), float(beta1), float(beta2),
                     float(grad_scale), stats=stats)
    dev = pred.device
    return (r["loss"].to(F32).reshape(1).to(dev), r["per_sample"].to(F32).to(dev), r["adr"].to(F32).to(dev), r["dpred"].to(BF16).to(dev) if want_grad else None)


def flow_euler_step(x, v, dt):
    EMU._need(x.dtype == BF16 and v.dtype == BF16 and dt.dtype == F32 and x.shape == v.shape and x.is_contiguous() and dt.numel() == x.shape[0]
              and (x.numel() // x.shape[0]) % 8 == 0 and x.data_ptr() != v.data_ptr(), "flow_euler_step: bf16 x (contiguous, in place) / v of one shape, fp32 dt [B]")
    x.copy_(euler64(x, v, dt).to(BF16))
    return x


STAND_INS = {"reflexflow_stats": reflexflow_stats, "reflexflow_loss": reflexflow_loss, "flow_euler_step": flow_euler_step}


def install(monkeypatch):
    """tests.dora_ref.install (the emulator and every earlier feature's stand-ins) + the three ReflexFlow stand-ins"""
    ops = DR.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops

"""Self-Transcendence (helpers/distillation/self_transcendence/distiller.py) restated — TEST INFRASTRUCTURE ONLY.

  * `factor_grid64` / `vae_target_tokens64`: `_factor_grid` / `_vae_target_tokens` for a 2-D latent.
  * `forward64` / `loss64`: the projector Linear(D -> Hp) -> SiLU -> Linear(Hp -> Hp) -> SiLU -> Linear(Hp -> D) on h [B, S, D], the masked per-sample MSE of either
    stage and its backward in fp64, closed form (no autograd): U1 = X W1^T + b1, A1 = silu(U1), U2 = A1 W2^T + b2, A2 = silu(U2), proj = A2 W3^T + b3;
    pred = proj[..., :P]; per_b = mean_{S, P} (pred - t)^2; m_b = [tmin <= sigma_b <= tmax]; guide = sum_b m_b per_b / n (0 when n = 0).  With
    G = 2 (pred - t) m_b and s = w / (n S P): d b3[:P] = s sum G, dW3[:P] = s G^T A2, dA2 = G W3[:P], dU2 = dA2 silu'(U2), d b2 = s sum dU2, dW2 = s dU2^T A1,
    dA1 = dU2 W2, dU1 = dA1 silu'(U1), d b1 = s sum dU1, dW1 = s dU1^T X, dh = s dU1 W1; rows P.. of dW3 / d b3 are zero.  Pinned against the executed reference
    by tests/golden/self_transcendence_vectors.pt (tools/gen_self_transcendence_golden.py); the GPU tests bound the kernels against it.
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/self_transcendence.hip with the kernels' contracts (fp32 arithmetic, one rounding per
    store, in place into the tensors given); `install()` puts them on top of tests.self_flow_ref.install (the emulator and every earlier stand-in).
  * `guide_autograd` / `sd3_oracle`: the oracle side of the engine tests — the reference arithmetic through autograd on the block outputs recorded by
    layersync_ref.record_sd3_blocks.
"""
import math

import torch
import torch.nn.functional as F

from tests import layersync_ref as LS
from tests import ops_emulator as EMU
from tests import self_flow_ref as SF

F32, F64 = torch.float32, torch.float64          # (the storage type is read as EMU.BF16: this module binds no constant of its own)
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
PREFIX = "self_transcendence_projector."
KEY = "self_transcendence_guide_loss"


# ---- the token grid and the patchified target ----
def factor_grid64(source_shape, token_count: int):
    H, W = (int(v) for v in source_shape)
    if H * W == token_count:
        return (H, W)
    best = None
    for f in range(1, token_count + 1):
        if token_count % f == 0 and H % f == 0 and W % (token_count // f) == 0:
            score = abs((f / (token_count // f)) - (H / W))
            if best is None or score < best[0]:
                best = (score, (f, token_count // f))
    if best is None:
        raise ValueError(f"Self-Transcendence could not map {token_count} tokens onto latent spatial shape {(H, W)}.")
    return best[1]


def vae_target_tokens64(target, token_count: int):
    """target [B, C, H, W] -> [B, S, C ph pw] fp64: token (i, j) holds target[b, c, i ph + a, j pw + e] in (c, a, e) order"""
    B, C, H, W = target.shape
    gh, gw = factor_grid64((H, W), token_count)
    ph, pw = H // gh, W // gw
    return target.to(F64).reshape(B, C, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, token_count, C * ph * pw)


# ---- the projector and the loss ----
def silu64(u):
    sg = torch.sigmoid(u)
    return u * sg, sg * (1.0 + u * (1.0 - sg))


def forward64(h, params):
    """h [B, S, D]; params in NAMES order -> the fp64 intermediates on the M = B S rows"""
    W1, b1, W2, b2, W3, b3 = (q.to(F64) for q in params)
    X = h.to(F64).reshape(-1, h.shape[-1])
    U1 = X @ W1.t() + b1
    A1, g1 = silu64(U1)
    U2 = A1 @ W2.t() + b2
    A2, g2 = silu64(U2)
    return dict(X=X, U1=U1, A1=A1, g1=g1, U2=U2, A2=A2, g2=g2, proj=A2 @ W3.t() + b3)


def mask64(sigmas, tmin: float, tmax: float):
    """the reference compares the batch's fp32 sigmas with the configured python floats (fp32 tensor against a double scalar: torch compares in fp32)"""
    s = sigmas.to(F32).reshape(sigmas.shape[0], -1)[:, 0]
    return (s >= tmin) & (s <= tmax)


def cfg_target64(cond, uncond, scale: float):
    return uncond.to(F64) + float(scale) * (cond.to(F64) - uncond.to(F64))


def loss64(h, params, target_tokens, sigmas, tmin: float, tmax: float, weight: float = 1.0):
    """target_tokens [B, S, P] (P <= D) -> dict(guide, per_sample [B], mask [B], n, inv, pred [B, S, P], G [M, P], dh [B, S, D], grads {name: gradient}) at upstream
    weight `weight`"""
    W1, b1, W2, b2, W3, b3 = (q.to(F64) for q in params)
    B, S, D = h.shape
    P = target_tokens.shape[-1]
    f = forward64(h, params)
    pred = f["proj"].view(B, S, D)[..., :P]
    diff = pred - target_tokens.to(F64)
    per = (diff * diff).flatten(1).mean(1)
    m = mask64(sigmas, tmin, tmax)
    n = int(m.sum())
    guide = per[m].mean() if n else torch.zeros((), dtype=F64)
    inv = 1.0 / (n * S * P) if n else 0.0
    G = (2.0 * diff * m.to(F64)[:, None, None]).reshape(B * S, P)
    s = weight * inv
    dA2 = G @ W3[:P]
    dU2 = dA2 * f["g2"]
    dA1 = dU2 @ W2
    dU1 = dA1 * f["g1"]
    gW3, gb3 = torch.zeros_like(W3), torch.zeros_like(b3)
    gW3[:P], gb3[:P] = s * G.t() @ f["A2"], s * G.sum(dim=0)
    grads = {"net.0.weight": s * dU1.t() @ f["X"], "net.0.bias": s * dU1.sum(dim=0), "net.2.weight": s * dU2.t() @ f["A1"], "net.2.bias": s * dU2.sum(dim=0),
             "net.4.weight": gW3, "net.4.bias": gb3}
    return dict(guide=guide, per_sample=per, mask=m, n=n, inv=inv, pred=pred, G=G, dh=(s * dU1 @ W1).view(B, S, D), grads=grads, f=f)


# ---- stand-ins with the kernels' contracts ----
def _params(name, W1, b1, W2, b2, W3, b3):
    ts = (W1, b1, W2, b2, W3, b3)
    EMU._need(all(t.dtype == F32 and t.is_contiguous() for t in ts), f"{name}: six contiguous fp32 tensors")
    EMU._need(W1.dim() == 2 and W2.dim() == 2 and W3.dim() == 2, f"{name}: W1 [Hp, D], W2 [Hp, Hp], W3 [D, Hp]")
    Hp, D = W1.shape
    EMU._need(D % 8 == 0 and Hp % 8 == 0 and D <= 16384 and Hp <= 16384, f"{name}: D and Hp multiples of 8, at most 16384")
    EMU._need(tuple(W2.shape) == (Hp, Hp) and tuple(W3.shape) == (D, Hp) and b1.numel() == Hp and b2.numel() == Hp and b3.numel() == D, f"{name}: the projector's shapes")
    for t in ts:
        EMU._al(t, 16, name)
    return D, Hp


def st_fold(W1, b1, W2, b2, W3, b3, W1h, W1T, b1h, W2h, W2T, b2h, W3h, W3T, b3h):
    D, Hp = _params("st_fold", W1, b1, W2, b2, W3, b3)
    outs = (W1h, W1T, b1h, W2h, W2T, b2h, W3h, W3T, b3h)
    P3 = W3T.shape[1] if W3T.dim() == 2 else 0
    EMU._need(0 < P3 <= D and P3 % 8 == 0, "st_fold: W3T [Hp, P3] with 0 < P3 <= D, a multiple of 8")
    EMU._need(all(t.dtype == EMU.BF16 and t.is_contiguous() for t in outs) and tuple(W1h.shape) == (Hp, D) and tuple(W1T.shape) == (D, Hp) and tuple(W2h.shape) == (Hp, Hp)
              and tuple(W2T.shape) == (Hp, Hp) and tuple(W3h.shape) == (D, Hp) and tuple(W3T.shape) == (Hp, P3) and b1h.numel() == Hp and b2h.numel() == Hp
              and b3h.numel() == D, "st_fold: outputs")
    for t in outs:
        EMU._al(t, 16, "st_fold")
    w1, w2, w3 = W1.to(EMU.BF16), W2.to(EMU.BF16), W3[:P3].to(EMU.BF16)
    W1h.copy_(w1); W1T.copy_(w1.t()); b1h.copy_(b1.to(EMU.BF16))
    W2h.copy_(w2); W2T.copy_(w2.t()); b2h.copy_(b2.to(EMU.BF16))
    W3h[:P3].copy_(w3); W3T.copy_(w3.t()); b3h[:P3].copy_(b3[:P3].to(EMU.BF16))
    return outs


def _loss_operands(name, pred, sigmas, tmin, tmax, B, S, Pc, per_sample, stats):
    EMU._need(float(tmin) <= float(tmax), f"{name}: the timestep range must satisfy min <= max")
    EMU._need(pred.dtype == EMU.BF16 and pred.is_contiguous() and tuple(pred.shape) == (B * S, Pc) and Pc % 8 == 0, f"{name}: pred [B S, Pc] contiguous bf16, Pc % 8 == 0")
    EMU._need(all(t.dtype == F32 and t.is_contiguous() for t in (sigmas, per_sample, stats)) and sigmas.numel() == B and per_sample.numel() == B and stats.numel() == 3
              and B <= 4096, f"{name}: sigmas [B], per_sample [B], stats [3] fp32, B <= 4096")
    EMU._al(pred, 16, name)


def _finish(pred, t32, sigmas, tmin, tmax, B, S, per_sample, stats):
    """the kernels' arithmetic: d in fp32, fp32 sums, the mask from fp32 comparisons against the fp32-rounded bounds"""
    d = pred.float().view(B, S, -1) - t32
    per = (d * d).flatten(1).sum(1) * torch.tensor(1.0 / (S * d.shape[-1]), dtype=F32)
    lo, hi = torch.tensor(float(tmin), dtype=F32), torch.tensor(float(tmax), dtype=F32)
    m = (sigmas >= lo) & (sigmas <= hi)
    n = int(m.sum())
    per_sample.copy_(per)
    stats[0] = (per[m].sum() / n) if n else 0.0
    stats[1] = float(n)
    stats[2] = float(torch.tensor(1.0 / (S * d.shape[-1]), dtype=F32) / n) if n else 0.0
    pred.copy_(torch.where(m[:, None, None], 2.0 * d, torch.zeros_like(d)).reshape(pred.shape).to(EMU.BF16))
    return stats


def st_vae_loss(pred, target, grid, sigmas, tmin, tmax, per_sample, stats):
    EMU._need(target.dtype in (EMU.BF16, F32) and target.dim() == 4, "st_vae_loss: target [B, C, H, W] bf16 or fp32")
    B, C, H, W = target.shape
    gh, gw = (int(v) for v in grid)
    EMU._need(gh > 0 and gw > 0 and H % gh == 0 and W % gw == 0, "st_vae_loss: the token grid does not divide the latent shape")
    S, ph, pw = gh * gw, H // gh, W // gw
    P = C * ph * pw
    EMU._need(target[0].is_contiguous() and (B == 1 or target.stride(0) >= C * H * W), "st_vae_loss: contiguous samples")
    _loss_operands("st_vae_loss", pred, sigmas, tmin, tmax, B, S, P, per_sample, stats)
    t = target.float().reshape(B, C, gh, ph, gw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, S, P)
    return _finish(pred, t, sigmas, tmin, tmax, B, S, per_sample, stats)


def st_cfg_loss(pred, capture, cfg_scale, sigmas, tmin, tmax, per_sample, stats):
    LS._view3(capture, "capture")
    B2, S, D = capture.shape
    EMU._need(B2 % 2 == 0 and B2 > 0, "st_cfg_loss: an even batch (conditional rows, then unconditional)")
    B = B2 // 2
    _loss_operands("st_cfg_loss", pred, sigmas, tmin, tmax, B, S, D, per_sample, stats)
    c, u = capture[:B].float(), capture[B:].float()
    EMU._al(capture[B:], 16, "st_cfg_loss")
    t = torch.addcmul(u, torch.tensor(float(cfg_scale), dtype=F32), c - u)          # one fma per element, fp32
    return _finish(pred, t, sigmas, tmin, tmax, B, S, per_sample, stats)


def _scale(name, s):
    EMU._need(torch.is_tensor(s) and s.dtype == F32 and s.numel() == 1, f"{name}: the scale is ONE fp32")


def st_wgrad(P, db, scale, g_W, g_b, accumulate=False):
    _scale("st_wgrad", scale)
    EMU._need(P.dtype == EMU.BF16 and P.dim() == 2 and P.shape[1] % 8 == 0, "st_wgrad: P [R, Cc] bf16, Cc % 8 == 0")
    R, Cc = P.shape
    EMU._need(db.dtype == F32 and g_W.dtype == F32 and g_b.dtype == F32 and tuple(g_W.shape) == (R, Cc) and db.numel() == R and g_b.numel() == R
              and all(t.is_contiguous() for t in (P, db, g_W, g_b)), "st_wgrad: db [R], g_W [R, Cc], g_b [R] fp32, contiguous")
    EMU._al(P, 16, "P"); EMU._al(g_W, 16, "g_W")
    s = scale.reshape(())
    g_W.copy_(torch.addcmul(g_W, s, P.float()) if accumulate else s * P.float())
    g_b.copy_((g_b + s * db.reshape(-1)) if accumulate else s * db.reshape(-1))
    return g_W, g_b


def st_dx_add(g, scale, dx):
    LS._view3(dx, "dx")
    _scale("st_dx_add", scale)
    B, rows, D = dx.shape
    EMU._need(g.dtype == EMU.BF16 and g.is_contiguous() and tuple(g.shape) == (B * rows, D), "st_dx_add: g [B rows, D] bf16 contiguous")
    EMU._al(g, 16, "g")
    dx.copy_(torch.addcmul(dx.float(), scale.reshape(()), g.float().view(B, rows, D)).to(EMU.BF16))
    return dx


STAND_INS = {"st_fold": st_fold, "st_vae_loss": st_vae_loss, "st_cfg_loss": st_cfg_loss, "st_wgrad": st_wgrad, "st_dx_add": st_dx_add}


def install(monkeypatch):
    """tests.self_flow_ref.install (the emulator and every earlier stand-in) + the Self-Transcendence stand-ins"""
    ops = SF.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side of the engine tests ----
def projector_autograd(h, params):
    W1, b1, W2, b2, W3, b3 = params
    return F.linear(F.silu(F.linear(F.silu(F.linear(h, W1, b1)), W2, b2)), W3, b3)


def masked_mse_autograd(prediction, target, sigmas, tmin, tmax):
    """distiller.py `_masked_mse`"""
    per = F.mse_loss(prediction.float(), target.float(), reduction="none").flatten(1).mean(1)
    m = mask64(sigmas, tmin, tmax)
    return per[m].mean() if bool(m.any()) else prediction.sum() * 0.0


def guide_autograd(h, params, stage, target, sigmas, tmin, tmax, cfg_scale=1.0):
    """the reference arithmetic on live autograd tensors.  target: stage `vae` the diffusion target [B, C, H, W]; stage `self` (cond, uncond) [B, S, D] teacher rows"""
    proj = projector_autograd(h, params)
    if stage == "vae":
        t = vae_target_tokens64(target, h.shape[1]).to(proj.dtype)
        return masked_mse_autograd(proj[..., :t.shape[-1]], t, sigmas, tmin, tmax)
    c, u = target
    return masked_mse_autograd(proj, (u + cfg_scale * (c - u)).detach(), sigmas, tmin, tmax)


def seed_projector(model, seed: int = 31):
    """projector parameters off their initial values, scaled so that the guide gradient is of the size of the diffusion loss's"""
    g = torch.Generator().manual_seed(seed)
    own = dict(model.named_parameters())
    vals = []
    with torch.no_grad():
        for nm in NAMES:
            p = own[PREFIX + nm]
            v = torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]) if p.dim() == 2 else 0.05 * torch.randn(p.shape, generator=g)
            p.copy_(v.to(p.device))
            vals.append(v)
    return vals


def sd3_oracle(monkeypatch, model, ocfg, d, student: int, weight: float, stage: str, target, sigmas, tmin, tmax, cfg_scale=1.0, lora=None, scale=1.0):
    """autograd through the oracle with the guide loss on the recorded student block output: (pred, loss, guide, lora params, projector parameters {name: tensor
    with .grad}, d(weight guide) / d h_student, the regulariser's share of the adapters' gradient).  d: host tensors (lat, prompt, pooled, t, target)."""
    from oracle import sd3 as OS
    from tests import parity_utils as PU
    outs = LS.record_sd3_blocks(monkeypatch)
    P, _, _ = PU.oracle_state(model)
    P = {k: v for k, v in P.items() if not k.startswith(PREFIX)}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    out = OS.sd3_forward(P, ocfg, d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale)
    own = dict(model.named_parameters())
    head = {nm: own[PREFIX + nm].detach().float().cpu().clone().requires_grad_(True) for nm in NAMES}
    guide = guide_autograd(outs[student], tuple(head[nm] for nm in NAMES), stage, target, sigmas, tmin, tmax, cfg_scale)
    mse = ((out - d["target"].float()) ** 2).mean()
    total = mse + weight * guide
    wrt = [t for ab in lp.values() for t in ab]
    g_mse = torch.autograd.grad(mse, wrt, retain_graph=True, allow_unused=True)
    dh = torch.autograd.grad(weight * guide, outs[student], retain_graph=True)[0]
    total.backward()
    return out.detach(), total.detach(), guide.detach(), lp, head, dh, LS._regulariser_share(wrt, g_mse)

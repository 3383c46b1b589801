"""NextLat (helpers/training/nextlat.py) restated — TEST INFRASTRUCTURE ONLY.

  * `forward64` / `loss64`: the predictor LayerNorm(D, eps 1e-6) -> Linear(D -> 2D) -> GELU(erf) -> Linear(2D -> D) on h[:, :-1] against h[:, 1:] and its backward in
    fp64, closed form (no autograd): xhat, rstd; n = xhat gamma + beta; U = n W_up^T + b_up; A = U Phi(U); pred = A W_down^T + b_down; psi = clamp(pred - t, -1, 1)
    (smooth-L1, beta 1) or 2 (pred - t) (MSE); with s = weight / (M D): d b_down = s sum psi, dW_down = s psi^T A, dA = psi W_down, dU = dA (Phi(U) + U phi(U)),
    d b_up = s sum dU, dW_up = s dU^T n, dn = dU W_up, d beta = s sum dn, d gamma = s sum dn xhat, g = dn gamma, dh[:, :-1] = s rstd (g - mean g - xhat mean(g xhat)),
    dh[:, -1] = 0.  Pinned against the executed reference by tests/golden/nextlat_vectors.pt (tools/gen_nextlat_golden.py); the GPU tests bound the kernels against it.
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/nextlat.hip with the kernels' contracts (bf16 in memory, fp32 arithmetic, one bf16 rounding
    per store, in place into the tensors given); `install()` puts them on top of tests.layersync_ref.install.
  * `sd3_oracle`: the oracle side of the engine tests — the reference arithmetic through autograd on the block output recorded by layersync_ref.record_sd3_blocks.
"""
import math

import torch

from tests import layersync_ref as LS
from tests import ops_emulator as EMU

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
NAMES = ("norm.weight", "norm.bias", "up.weight", "up.bias", "down.weight", "down.bias")
PREFIX = "nextlat_predictor."
MODES = ("smooth_l1", "mse")


def phi64(u):
    """(Phi(u), the standard normal density at u)"""
    return 0.5 * torch.erfc(-u / math.sqrt(2.0)), torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def rows64(x):
    """x [M, D] -> (xhat [M, D], rstd [M]), fp64"""
    x = x.to(F64)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    return (x - mean) * rstd, rstd[:, 0]


def forward64(h, params):
    """h [B, S, D]; params in NAMES order.  Returns a dict of the fp64 intermediates on the M = B (S - 1) predictor rows."""
    ga, be, Wu, bu, Wd, bd = (p.to(F64) for p in params)
    B, S, D = h.shape
    x = h[:, :-1].to(F64).reshape(-1, D)
    t = h[:, 1:].to(F64).reshape(-1, D)
    xhat, rstd = rows64(x)
    n = xhat * ga + be
    U = n @ Wu.t() + bu
    Phi, dens = phi64(U)
    A = U * Phi
    pred = A @ Wd.t() + bd
    return dict(xhat=xhat, rstd=rstd, n=n, U=U, A=A, gelu_grad=Phi + U * dens, pred=pred, target=t)


def psi64(pred, t, mode: str):
    """(per-element loss, psi = d loss / d pred)"""
    d = pred - t
    if mode == "mse":
        return d * d, 2.0 * d
    a = d.abs()
    return torch.where(a < 1.0, 0.5 * d * d, a - 0.5), d.clamp(-1.0, 1.0)


def loss64(h, params, weight: float, mode: str = "smooth_l1"):
    """NextLatRegularizer.compute_loss and its gradient: (loss, logs, pred [B, S-1, D], dh [B, S, D], {name: gradient})"""
    ga, be, Wu, bu, Wd, bd = (p.to(F64) for p in params)
    B, S, D = h.shape
    f = forward64(h, params)
    elem, psi = psi64(f["pred"], f["target"], mode)
    state = elem.mean()
    s = weight / elem.numel()
    dA = psi @ Wd
    dU = dA * f["gelu_grad"]
    dn = dU @ Wu
    g = dn * ga
    xhat = f["xhat"]
    dx = s * f["rstd"][:, None] * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    dh = torch.zeros(B, S, D, dtype=F64)
    dh[:, :-1] = dx.view(B, S - 1, D)
    grads = {"norm.weight": s * (dn * xhat).sum(dim=0), "norm.bias": s * dn.sum(dim=0), "up.weight": s * dU.t() @ f["n"], "up.bias": s * dU.sum(dim=0),
             "down.weight": s * psi.t() @ f["A"], "down.bias": s * psi.sum(dim=0)}
    logs = {"nextlat_loss": (state * weight).item(), "nextlat_state_loss": state.item()}
    return state * weight, logs, f["pred"].view(B, S - 1, D), dh, grads


# ---- stand-ins with the kernels' contracts ----
def _params(name, gamma, beta, W_up, b_up, W_down, b_down):
    ts = (gamma, beta, W_up, b_up, W_down, b_down)
    dt = W_up.dtype
    EMU._need(dt in (F32, BF16) and all(t.dtype == dt for t in ts), f"{name}: the six predictor tensors must share one dtype, fp32 or bf16")
    EMU._need(W_up.dim() == 2 and W_up.shape[0] == 2 * W_up.shape[1], f"{name}: W_up [2D, D]")
    D = W_up.shape[1]
    EMU._need(D % 8 == 0 and D <= 4096, f"{name}: D must be a multiple of 8, at most 4096")
    EMU._need(tuple(W_down.shape) == (D, 2 * D) and gamma.numel() == D and beta.numel() == D and b_up.numel() == 2 * D and b_down.numel() == D
              and all(t.is_contiguous() for t in ts), f"{name}: contiguous gamma [D], beta [D], W_up [2D, D], b_up [2D], W_down [D, 2D], b_down [D]")
    for t in ts:
        EMU._al(t, 16, name)
    return D


def _put(dst, val, accumulate=False):
    dst.copy_(((dst.float() + val) if accumulate else val).to(dst.dtype))


def nextlat_fold(gamma, beta, W_up, b_up, W_down, b_down, W1f, W1fT, c1, Wd, WdT, bd):
    D = _params("nextlat_fold", gamma, beta, W_up, b_up, W_down, b_down)
    outs = (W1f, W1fT, c1, Wd, WdT, bd)
    EMU._need(all(t.dtype == BF16 and t.is_contiguous() for t in outs) and tuple(W1f.shape) == (2 * D, D) and tuple(W1fT.shape) == (D, 2 * D) and c1.numel() == 2 * D
              and tuple(Wd.shape) == (D, 2 * D) and tuple(WdT.shape) == (2 * D, D) and bd.numel() == D, "nextlat_fold: outputs")
    f = (W_up.float() * gamma.float()[None, :]).to(BF16)
    W1f.copy_(f); W1fT.copy_(f.t())
    c1.copy_((W_up.float() @ beta.float() + b_up.float()).to(BF16))
    w = W_down.float().to(BF16)
    Wd.copy_(w); WdT.copy_(w.t())
    bd.copy_(b_down.float().to(BF16))
    return outs


def nextlat_rows(h, xhat, rstd):
    LS._view3(h, "h")
    B, rows, D = h.shape
    M = B * rows
    EMU._need(D % 64 == 0 and D <= 4096, "nextlat_rows: D must be a multiple of 64, at most 4096")
    EMU._need(xhat.dtype == BF16 and xhat.is_contiguous() and tuple(xhat.shape) == (M, D) and rstd.dtype == F32 and rstd.is_contiguous() and rstd.numel() == M,
              "nextlat_rows: xhat [M, D] bf16, rstd [M] fp32, contiguous")
    EMU._al(xhat, 16, "xhat")
    x = h.float().reshape(M, D)
    mean = x.mean(dim=-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    xhat.copy_(((x - mean) * rs).to(BF16))
    rstd.copy_(rs[:, 0])
    return xhat, rstd


def _gelu_operands(name, *ts):
    EMU._need(all(t.dtype == BF16 and t.is_contiguous() and t.shape == ts[0].shape for t in ts) and ts[0].numel() % 8 == 0 and ts[0].numel() > 0,
              f"{name}: contiguous bf16 tensors of one shape, a multiple of 8 elements")
    for t in ts:
        EMU._al(t, 16, name)


def gelu_erf(U, A):
    _gelu_operands("gelu_erf", U, A)
    A.copy_(torch.nn.functional.gelu(U.float()).to(BF16))
    return A


def gelu_erf_bwd(U, dA, dU):
    _gelu_operands("gelu_erf_bwd", U, dA, dU)
    u = U.float()
    grad = 0.5 * torch.erfc(-u / math.sqrt(2.0)) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    dU.copy_((dA.float() * grad).to(BF16))
    return dU


def nextlat_loss(pred, target, mode, loss):
    EMU._need(mode in MODES, "nextlat_loss: mode must be 'smooth_l1' or 'mse'")
    LS._view3(target, "target")
    B, rows, D = target.shape
    M = B * rows
    EMU._need(D <= 4096 and pred.dtype == BF16 and pred.is_contiguous() and tuple(pred.shape) == (M, D) and loss.dtype == F32 and loss.numel() == 1,
              "nextlat_loss: pred [M, D] bf16 contiguous, one fp32 for the loss")
    EMU._al(pred, 16, "pred")
    d = pred.float() - target.float().reshape(M, D)
    if mode == "mse":
        elem, psi = d * d, 2.0 * d
    else:
        elem, psi = torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5), d.clamp(-1.0, 1.0)
    loss.copy_(elem.mean().reshape(loss.shape))
    pred.copy_(psi.to(BF16))
    return loss


def _scale(name, s):
    EMU._need(s.dtype == F32 and s.numel() == 1, f"{name}: the scale is ONE fp32")


def nextlat_ln_bwd_add(g, xhat, rstd, scale, dx):
    LS._view3(dx, "dx")
    _scale("nextlat_ln_bwd_add", scale)
    B, rows, D = dx.shape
    M = B * rows
    EMU._need(D <= 4096 and all(t.is_contiguous() for t in (g, xhat, rstd)) and tuple(g.shape) == (M, D) and tuple(xhat.shape) == (M, D) and rstd.numel() == M
              and g.dtype == BF16 and xhat.dtype == BF16 and rstd.dtype == F32, "nextlat_ln_bwd_add: g [M, D], xhat [M, D] bf16, rstd [M] fp32, contiguous")
    EMU._al(g, 16, "g"); EMU._al(xhat, 16, "xhat")
    gf, x = g.float(), xhat.float()
    dh = (scale.reshape(()) * rstd)[:, None] * (gf - gf.mean(dim=-1, keepdim=True) - x * (gf * x).mean(dim=-1, keepdim=True))
    dx.copy_((dx.float() + dh.view(B, rows, D)).to(BF16))
    return dx


def nextlat_wgrad_up(P1, db1, gamma, beta, W_up, scale, g_gamma, g_beta, g_W, g_b, accumulate=False):
    ts = (gamma, beta, W_up, g_gamma, g_beta, g_W, g_b)
    dt = W_up.dtype
    _scale("nextlat_wgrad_up", scale)
    EMU._need(dt in (F32, BF16) and all(t.dtype == dt for t in ts), "nextlat_wgrad_up: parameters and gradients must share one dtype, fp32 or bf16")
    EMU._need(W_up.dim() == 2 and W_up.shape[0] == 2 * W_up.shape[1], "nextlat_wgrad_up: W_up [2D, D]")
    D = W_up.shape[1]
    EMU._need(D % 8 == 0 and D <= 4096 and P1.dtype == BF16 and db1.dtype == F32 and tuple(P1.shape) == (2 * D, D) and db1.numel() == 2 * D and tuple(g_W.shape) == (2 * D, D)
              and g_b.numel() == 2 * D and all(t.numel() == D for t in (gamma, beta, g_gamma, g_beta)) and all(t.is_contiguous() for t in ts + (P1, db1)),
              "nextlat_wgrad_up: P1 [2D, D] bf16, db1 [2D] fp32, parameters / gradients in the predictor's shapes, contiguous")
    for t in (P1, gamma, beta, W_up, g_W):
        EMU._al(t, 16, "nextlat_wgrad_up")
    s, P, db, W = scale.reshape(()), P1.float(), db1.float().reshape(-1), W_up.float()
    _put(g_W, s * (P * gamma.float()[None, :] + db[:, None] * beta.float()[None, :]), accumulate)
    _put(g_b, s * db, accumulate)
    _put(g_gamma, s * (W * P).sum(dim=0), accumulate)
    _put(g_beta, s * (W * db[:, None]).sum(dim=0), accumulate)
    return g_gamma, g_beta, g_W, g_b


def nextlat_wgrad_down(P2, db2, scale, g_W, g_b, accumulate=False):
    _scale("nextlat_wgrad_down", scale)
    EMU._need(g_W.dtype in (F32, BF16) and g_b.dtype == g_W.dtype, "nextlat_wgrad_down: the gradients must share one dtype, fp32 or bf16")
    EMU._need(g_W.dim() == 2 and g_W.shape[1] == 2 * g_W.shape[0], "nextlat_wgrad_down: g_W [D, 2D]")
    D = g_W.shape[0]
    EMU._need(D % 8 == 0 and D <= 4096 and P2.dtype == BF16 and db2.dtype == F32 and tuple(P2.shape) == (D, 2 * D) and db2.numel() == D and g_b.numel() == D
              and all(t.is_contiguous() for t in (P2, db2, g_W, g_b)), "nextlat_wgrad_down: P2 [D, 2D] bf16, db2 [D] fp32, g_W [D, 2D], g_b [D], contiguous")
    for t in (P2, db2, g_W, g_b):
        EMU._al(t, 16, "nextlat_wgrad_down")
    s = scale.reshape(())
    _put(g_W, s * P2.float(), accumulate)
    _put(g_b, s * db2.float().reshape(-1), accumulate)
    return g_W, g_b


STAND_INS = {"nextlat_fold": nextlat_fold, "nextlat_rows": nextlat_rows, "gelu_erf": gelu_erf, "gelu_erf_bwd": gelu_erf_bwd, "nextlat_loss": nextlat_loss,
             "nextlat_ln_bwd_add": nextlat_ln_bwd_add, "nextlat_wgrad_up": nextlat_wgrad_up, "nextlat_wgrad_down": nextlat_wgrad_down}


def install(monkeypatch):
    """tests.layersync_ref.install + the NextLat stand-ins"""
    ops = LS.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side of the engine tests ----
def state_autograd(h, params, mode: str = "smooth_l1"):
    """the reference arithmetic on live autograd tensors: the state loss of predictor(h[:, :-1]) against h[:, 1:].detach()"""
    import torch.nn.functional as F
    ga, be, Wu, bu, Wd, bd = params
    pred = F.linear(F.gelu(F.linear(F.layer_norm(h[:, :-1], (h.shape[-1],), ga, be, EPS), Wu, bu)), Wd, bd)
    tgt = h[:, 1:].detach()
    return F.smooth_l1_loss(pred.float(), tgt.float(), reduction="mean") if mode == "smooth_l1" else F.mse_loss(pred.float(), tgt.float(), reduction="mean")


def seed_predictor(model, seed: int = 23):
    """non-zero predictor parameters (the reference's zero `down` makes dh and four of the six parameter gradients vanish and would hide the injection)"""
    g = torch.Generator().manual_seed(seed)
    D = model.D
    vals = (1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(2 * D, D, generator=g) / D ** 0.5,
            0.05 * torch.randn(2 * D, generator=g), torch.randn(D, 2 * D, generator=g) / (2 * D) ** 0.5, 0.05 * torch.randn(D, generator=g))
    own = dict(model.named_parameters())
    with torch.no_grad():
        for nm, v in zip(NAMES, vals):
            p = own[PREFIX + nm]
            p.copy_(v.to(p.device, p.dtype))
    return vals


def sd3_oracle(monkeypatch, model, ocfg, d, block: int, weight: float, full: bool, lora=None, scale=1.0, layersync=None, mode: str = "smooth_l1"):
    """autograd through the oracle with the regulariser on the recorded block output: (pred, loss, state, P, lora params, the regulariser's share of the trunk's
    gradient, predictor parameters {name: tensor with .grad}).  d: host tensors (lat, prompt, pooled, t, target).  layersync = (student, teacher, lambda) adds that
    term."""
    from oracle import sd3 as OS
    from tests import parity_utils as PU
    outs = LS.record_sd3_blocks(monkeypatch)
    P, _, _ = PU.oracle_state(model)
    head = {k: P.pop(k).clone().requires_grad_(True) for k in list(P) if k.startswith(PREFIX)}
    P = {k: (v.clone().requires_grad_(True) if full else v) for k, v in P.items()}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = None if lora is None else {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    out = OS.sd3_forward(P, ocfg, d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale)
    state = state_autograd(outs[block], tuple(head[PREFIX + nm] for nm in NAMES), mode)
    mse = ((out - d["target"].float()) ** 2).mean()
    total = mse + weight * state
    if layersync is not None:
        s, t, lam = layersync
        total = total - lam * LS.autograd_similarity(outs[s], outs[t])
    wrt = [t for ab in lp.values() for t in ab] if lp is not None else [v for k, v in P.items() if k != "pos_embed.pos_embed"]
    g_mse = torch.autograd.grad(mse, wrt, retain_graph=True, allow_unused=True)
    total.backward()
    if full:
        P.update(head)                        # check_full_grads walks the model's parameter names: the predictor's among them
    return out.detach(), total.detach(), state.detach(), P, lp, LS._regulariser_share(wrt, g_mse), head

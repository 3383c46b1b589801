"""Internal Guidance (helpers/training/internal_guidance.py) restated — TEST INFRASTRUCTURE ONLY.

  * `reference64` / `loss64`: the head LayerNorm(D, eps 1e-6) -> Linear(D -> 64) and its backward in fp64, closed form (no autograd): per row mean, biased variance,
    rstd = 1 / sqrt(var + 1e-6), xhat, y = (xhat * gamma + beta) W^T + b; given dy: db = sum dy, dW = dy^T n, dn = dy W, d beta = sum dn, d gamma = sum dn * xhat,
    g = dn * gamma, dh = rstd * (g - mean(g) - xhat * mean(g * xhat)).  Pinned against the executed reference by tests/golden/internal_guidance_vectors.pt
    (tools/gen_internal_guidance_golden.py); the GPU tests bound the kernels against it.
  * `ig_fold` / `ig_head_fwd` / `ig_head_bwd` / `ig_wgrad`: plain-torch stand-ins for the four `simpletuner_amd.ops` wrappers with the kernels' contracts (bf16 in
    memory, fp32 arithmetic, one bf16 rounding per store, in place into the tensors given); `install()` puts them on top of tests.layersync_ref.install.
  * `sd3_oracle`: the oracle side of the engine tests — the reference arithmetic through autograd on the block output recorded by layersync_ref.record_sd3_blocks.
"""
import torch

from tests import layersync_ref as LS
from tests import ops_emulator as EMU

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
N = 64
NAMES = ("norm.weight", "norm.bias", "proj.weight", "proj.bias")
PREFIX = "internal_guidance_head."


def unpatchify(y, C: int, H: int, W: int):
    """[B, (H/2)(W/2), 4C] tokens in (dh, dw, c) order -> [B, C, H, W] (differentiable; = ops.unpatchify(order=1))"""
    B = y.shape[0]
    return y.reshape(B, H // 2, W // 2, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def patchify(x):
    """[B, C, H, W] -> [B, (H/2)(W/2), 4C] in (dh, dw, c) order (= ops.patchify(order=1))"""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, (H // 2) * (W // 2), 4 * C)


def reference64(h, gamma, beta, W, b):
    """h [B, rows, D] or [M, D] (any float dtype; read as fp64).  Returns (xhat [M, D], rstd [M], y [M, N]), all fp64."""
    x = h.to(F64).reshape(-1, h.shape[-1])
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (x - mean) * rstd
    y = (xhat * gamma.to(F64) + beta.to(F64)) @ W.to(F64).t() + b.to(F64)
    return xhat, rstd[:, 0], y


def backward64(xhat, rstd, dy, gamma, beta, W):
    """the closed-form backward: (dh [M, D], d gamma, d beta, dW, db), fp64"""
    dy, ga, be, Wd = dy.to(F64), gamma.to(F64), beta.to(F64), W.to(F64)
    n = xhat * ga + be
    db = dy.sum(dim=0)
    dW = dy.t() @ n
    dn = dy @ Wd
    dbeta = dn.sum(dim=0)
    dgamma = (dn * xhat).sum(dim=0)
    g = dn * ga
    dh = rstd[:, None] * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    return dh, dgamma, dbeta, dW, db


def loss64(h, gamma, beta, W, b, target, weight: float):
    """InternalGuidanceRegularizer.compute_loss against a foundation whose loss() is the MSE: (loss, logs, tokens, prediction, dh, d gamma, d beta, dW, db)"""
    B, C, H, Wd = target.shape
    xhat, rstd, y = reference64(h, gamma, beta, W, b)
    pred = unpatchify(y.reshape(B, -1, N), C, H, Wd)
    diff = pred - target.to(F64)
    inter = (diff ** 2).mean()
    loss = inter * weight
    dy = patchify(2.0 * weight * diff / diff.numel()).reshape(-1, N)
    grads = backward64(xhat, rstd, dy, gamma, beta, W)
    logs = {"internal_guidance_loss": loss.item(), "internal_guidance_unweighted_loss": inter.item()}
    return (loss, logs, y.reshape(B, -1, N), pred, grads[0].reshape(h.shape)) + grads[1:]


# ---- stand-ins with the kernels' contracts ----
def _params(name, gamma, beta, W, b):
    dt = W.dtype
    EMU._need(dt in (F32, BF16) and all(t.dtype == dt for t in (gamma, beta, b)), f"{name}: gamma, beta, W and b must share one dtype, fp32 or bf16")
    EMU._need(W.dim() == 2 and W.shape[0] == N, f"{name}: the head has N = {N} output features")
    D = W.shape[1]
    EMU._need(D % 8 == 0 and D <= 4096, f"{name}: D must be a multiple of 8, at most 4096")
    EMU._need(gamma.numel() == D and beta.numel() == D and b.numel() == N and all(t.is_contiguous() for t in (gamma, beta, W, b)), f"{name}: contiguous gamma [D], beta [D], W [N, D], b [N]")
    return D


def ig_fold(gamma, beta, W, b, Wf, WfT, c):
    D = _params("ig_fold", gamma, beta, W, b)
    EMU._need(all(t.dtype == BF16 and t.is_contiguous() for t in (Wf, WfT, c)) and tuple(Wf.shape) == (N, D) and tuple(WfT.shape) == (D, N) and c.numel() == N, "ig_fold: outputs")
    f = (W.float() * gamma.float()[None, :]).to(BF16)
    Wf.copy_(f); WfT.copy_(f.t())
    c.copy_((W.float() @ beta.float() + b.float()).to(BF16))
    return Wf, WfT, c


def ig_head_fwd(h, Wf, c, xhat, rstd, y):
    LS._view3(h, "h")
    B, rows, D = h.shape
    M = B * rows
    EMU._need(D <= 4096 and tuple(Wf.shape) == (N, D) and Wf.dtype == BF16 and c.dtype == BF16 and c.numel() == N, "ig_head_fwd: Wf [64, D] / c [64] bf16")
    EMU._need(xhat.dtype == BF16 and xhat.is_contiguous() and tuple(xhat.shape) == (M, D) and rstd.dtype == F32 and rstd.is_contiguous() and rstd.numel() == M
              and y.dtype == BF16 and y.is_contiguous() and tuple(y.shape) == (M, N), "ig_head_fwd: xhat [M, D] bf16, rstd [M] fp32, y [M, 64] bf16, contiguous")
    EMU._al(xhat, 16, "xhat")
    x = h.float().reshape(M, D)
    mean = x.mean(dim=-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    xhat.copy_(((x - mean) * rs).to(BF16))
    rstd.copy_(rs[:, 0])
    EMU.gemm(xhat, Wf, bias=c, out=y)
    return xhat, rstd, y


def ig_head_bwd(xhat, rstd, dy, WfT, dx):
    LS._view3(dx, "dx")
    B, rows, D = dx.shape
    M = B * rows
    EMU._need(D <= 4096 and dy.dim() == 2 and dy.shape[1] == N and tuple(WfT.shape) == (D, N), "ig_head_bwd: the head has N = 64 output features")
    EMU._need(all(t.is_contiguous() for t in (xhat, rstd, dy, WfT)) and tuple(xhat.shape) == (M, D) and dy.shape[0] == M and rstd.numel() == M and xhat.dtype == BF16
              and dy.dtype == BF16 and WfT.dtype == BF16 and rstd.dtype == F32, "ig_head_bwd: xhat [M, D], dy [M, 64], WfT [D, 64] bf16, rstd [M] fp32, contiguous")
    for t, nm in ((xhat, "xhat"), (dy, "dy"), (WfT, "WfT")):
        EMU._al(t, 16, nm)
    g = dy.float() @ WfT.float().t()
    x = xhat.float()
    dh = rstd[:, None] * (g - g.mean(dim=-1, keepdim=True) - x * (g * x).mean(dim=-1, keepdim=True))
    dx.copy_((dx.float() + dh.view(B, rows, D)).to(BF16))
    return dx


def ig_wgrad(xhat, dy, gamma, beta, W, g_gamma, g_beta, g_W, g_b, accumulate=False):
    D = _params("ig_wgrad", gamma, beta, W, g_b)
    EMU._need(_params("ig_wgrad", g_gamma, g_beta, g_W, g_b) == D and g_W.dtype == W.dtype, "ig_wgrad: gradients in the parameters' dtype and shapes")
    EMU._need(xhat.dtype == BF16 and dy.dtype == BF16 and xhat.is_contiguous() and dy.is_contiguous() and xhat.dim() == 2 and tuple(dy.shape) == (xhat.shape[0], N)
              and xhat.shape[1] == D, "ig_wgrad: xhat [M, D], dy [M, 64] bf16, contiguous")
    P = dy.float().t() @ xhat.float()
    db = dy.float().sum(dim=0)
    Wf32 = W.float()
    outs = ((g_gamma, (Wf32 * P).sum(dim=0)), (g_beta, (Wf32 * db[:, None]).sum(dim=0)), (g_W, P * gamma.float()[None, :] + db[:, None] * beta.float()[None, :]), (g_b, db))
    for dst, val in outs:
        dst.copy_(((dst.float() + val) if accumulate else val).to(dst.dtype))
    return g_gamma, g_beta, g_W, g_b


STAND_INS = {"ig_fold": ig_fold, "ig_head_fwd": ig_head_fwd, "ig_head_bwd": ig_head_bwd, "ig_wgrad": ig_wgrad}


def install(monkeypatch):
    """tests.layersync_ref.install + the four Internal Guidance stand-ins"""
    ops = LS.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side of the engine tests ----
def head_autograd(h, gamma, beta, W, b, C: int, H: int, Wd: int):
    """the reference arithmetic on live autograd tensors: unpatchify(proj(norm(h)))"""
    import torch.nn.functional as F
    y = F.linear(F.layer_norm(h, (h.shape[-1],), gamma, beta, EPS), W, b)
    return unpatchify(y, C, H, Wd)


def seed_head(model, seed: int = 17):
    """non-zero head parameters (a zero projection makes dn = 0 and would hide the injection): gamma ~ 1 + 0.25 n, beta ~ 0.1 n, W ~ n / sqrt(D), b ~ 0.05 n"""
    g = torch.Generator().manual_seed(seed)
    D = model.D
    vals = (1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(N, D, generator=g) / D ** 0.5, 0.05 * torch.randn(N, generator=g))
    own = dict(model.named_parameters())
    with torch.no_grad():
        for nm, v in zip(NAMES, vals):
            p = own[PREFIX + nm]
            p.copy_(v.to(p.device, p.dtype))
    return vals


def sd3_oracle(monkeypatch, model, ocfg, d, block: int, weight: float, full: bool, lora=None, scale=1.0, layersync=None):
    """autograd through the oracle with the regulariser on the recorded block output: (pred, loss, ig_pred, P, lora params, the regulariser's share of the trunk's
    gradient, head parameters {name: tensor with .grad}).  d: host tensors (lat, prompt, pooled, t, target).  layersync = (student, teacher, lambda) adds that term."""
    from oracle import sd3 as OS
    from tests import parity_utils as PU
    outs = LS.record_sd3_blocks(monkeypatch)
    P, _, _ = PU.oracle_state(model)
    head = {k: P.pop(k).clone().requires_grad_(True) for k in list(P) if k.startswith(PREFIX)}
    P = {k: (v.clone().requires_grad_(True) if full else v) for k, v in P.items()}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    lp = None if lora is None else {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    out = OS.sd3_forward(P, ocfg, d["lat"].float(), d["prompt"].float(), d["pooled"].float(), d["t"], lora=lp, lora_scale=scale)
    tgt = d["target"].float()
    igp = head_autograd(outs[block], *(head[PREFIX + nm] for nm in NAMES), tgt.shape[1], tgt.shape[2], tgt.shape[3])
    mse = ((out - tgt) ** 2).mean()
    total = mse + weight * ((igp - tgt) ** 2).mean()
    if layersync is not None:
        s, t, lam = layersync
        total = total - lam * LS.autograd_similarity(outs[s], outs[t])
    wrt = [t for ab in lp.values() for t in ab] if lp is not None else [v for k, v in P.items() if k != "pos_embed.pos_embed"]
    g_mse = torch.autograd.grad(mse, wrt, retain_graph=True, allow_unused=True)
    total.backward()
    if full:
        P.update(head)                        # check_full_grads walks the model's parameter names: the head's among them
    return out.detach(), total.detach(), igp.detach(), P, lp, LS._regulariser_share(wrt, g_mse), head

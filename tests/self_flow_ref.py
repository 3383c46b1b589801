"""Self-Flow (the reference's CREPA with crepa_feature_source=self_flow) restated — TEST INFRASTRUCTURE ONLY.

  * `views64`: common.py `_prepare_image_crepa_self_flow_batch` in fp64 from the recorded draws: the token mask `uniforms < ratio`, the student's sigma grid
    (repeated over each p x p patch) and token timesteps, the teacher's min(sigma, sigma_alt) / min(t, t_alt), both noisy views (1 - s) x + s n.
  * `forward64` / `loss64`: crepa.py `compute_loss` in self_flow / image mode and its backward in fp64, closed form (no autograd): xhat, rstd (eps 1e-5, nn.LayerNorm's
    default); n = xhat gamma + beta; proj = n W^T + b; c = <normalize(proj), normalize(f)> per token row, sim = mean(c) (one frame: no neighbour terms, the
    per-sample means of equal token counts are the global mean); loss = -w sim.  With G = d sim / d proj = (f^ - c proj^) / |proj| / M and s = -w:
    d b = s sum G, dW = s G^T n, dn = G W, d beta = s sum dn, d gamma = s sum dn xhat, g = dn gamma, dh = s rstd (g - mean g - xhat mean(g xhat)).
    Pinned against the executed reference by tests/golden/self_flow_vectors.pt (tools/gen_self_flow_golden.py); the GPU tests bound the kernels against it.
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/self_flow.hip with the kernels' contracts (fp32 arithmetic, one rounding per store, in
    place into the tensors given); `install()` puts them on top of tests.tlora_ref.install (the emulator and every earlier stand-in).
  * `similarity_autograd` / `sd3_oracle_blocks`: the oracle side of the engine tests — the reference arithmetic through autograd on the block outputs recorded by
    layersync_ref.record_sd3_blocks.
"""
import torch
import torch.nn.functional as F

from tests import layersync_ref as LS
from tests import ops_emulator as EMU
from tests import tlora_ref as TR

F32, F64 = torch.float32, torch.float64          # (the storage type is read as EMU.BF16: this module binds no constant of its own)
EPS = 1e-5
NAMES = ("0.weight", "0.bias", "1.weight", "1.bias")
PREFIX = "crepa_projector."


# ---- the views ----
def views64(latents, noise, sigma, sigma_alt, t, t_alt, uniforms, ratio: float, p: int):
    lat, n = latents.to(F64), noise.to(F64)
    B, C, H, W = lat.shape
    assert H % p == 0 and W % p == 0
    s0, s1, t0, t1 = (v.to(F64).reshape(B) for v in (sigma, sigma_alt, t, t_alt))
    mask = uniforms.to(F64) < float(ratio)                                         # [B, H/p, W/p]
    tok_s = torch.where(mask, s1[:, None, None], s0[:, None, None])
    grid = tok_s.repeat_interleave(p, dim=1).repeat_interleave(p, dim=2)[:, None]      # [B, 1, H, W]
    tok_t = torch.where(mask, t1[:, None, None], t0[:, None, None]).flatten(1)
    sT, tT = torch.minimum(s0, s1), torch.minimum(t0, t1)
    sTv = sT.view(B, 1, 1, 1)
    return dict(mask=mask, sigma_grid=grid, token_timesteps=tok_t, sigma_teacher=sT, timestep_teacher=tT,
                noisy_student=(1 - grid) * lat + grid * n, noisy_teacher=(1 - sTv) * lat + sTv * n)


# ---- the projector and the alignment ----
def rows64(x):
    x = x.to(F64)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    return (x - mean) * rstd, rstd[:, 0]


def forward64(h, params):
    """h [B, S, D]; params in NAMES order -> the fp64 intermediates on the M = B S rows"""
    ga, be, W, b = (q.to(F64) for q in params)
    D = h.shape[-1]
    xhat, rstd = rows64(h.reshape(-1, D))
    n = xhat * ga + be
    return dict(xhat=xhat, rstd=rstd, n=n, proj=n @ W.t() + b)


def loss64(h, teacher, params, weight: float):
    """-> (loss = -w sim, sim, cos [M], proj [M, D], dh [B, S, D], {name: gradient}) of the alignment term at scheduler weight w"""
    ga, be, W, b = (q.to(F64) for q in params)
    f = forward64(h, params)
    cos, sim, G, _ = LS.reference64(f["proj"].view(h.shape), teacher)
    s = -float(weight)
    dn = G @ W
    g = dn * ga
    xhat = f["xhat"]
    dh = s * f["rstd"][:, None] * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    grads = {"0.weight": s * (dn * xhat).sum(dim=0), "0.bias": s * dn.sum(dim=0), "1.weight": s * G.t() @ f["n"], "1.bias": s * G.sum(dim=0)}
    return s * sim, sim, cos, f["proj"], dh.view(h.shape), grads


# ---- stand-ins with the kernels' contracts ----
def self_flow_views(latents, noise, sigma, sigma_alt, timesteps, timesteps_alt, uniforms, ratio, patch=2, want_sigma_grid=False, out=None):
    EMU._need(latents.dtype in (EMU.BF16, F32) and noise.dtype == latents.dtype, "self_flow_views: latents and noise must share one dtype, bf16 or fp32")
    EMU._need(latents.dim() == 4 and noise.shape == latents.shape, "self_flow_views: latents and noise [B, C, H, W] of one shape")
    B, C, H, W = latents.shape
    patch = int(patch)
    EMU._need(patch >= 1 and H % patch == 0 and W % patch == 0, "self_flow_views: H % patch_size != 0 or W % patch_size != 0")
    EMU._need(0.0 <= float(ratio) <= 0.5, "self_flow_views: the mask ratio must lie in [0, 0.5]")
    vec = 8 if latents.dtype == EMU.BF16 else 4
    for t in (latents, noise):
        EMU._need(t[0].is_contiguous() and (B == 1 or (t.stride(0) >= C * H * W and t.stride(0) % vec == 0)), "self_flow_views: contiguous samples, batch stride a multiple of the vector")
        EMU._al(t, 16, "self_flow_views")
    EMU._need((C * H * W) % vec == 0, "self_flow_views: C * H * W must be a multiple of the vector width")
    for t in (sigma, sigma_alt, timesteps, timesteps_alt):
        EMU._need(t.dtype == F32 and t.dim() == 1 and t.numel() == B and t.is_contiguous(), "self_flow_views: [B] fp32 vectors")
    EMU._need(uniforms.dtype == F32 and tuple(uniforms.shape) == (B, H // patch, W // patch) and uniforms.is_contiguous(), "self_flow_views: uniforms [B, H/p, W/p] fp32")
    mask = uniforms < torch.tensor(float(ratio), dtype=F32)                        # the kernel compares in fp32
    s0, s1 = sigma.view(B, 1, 1), sigma_alt.view(B, 1, 1)
    grid = torch.where(mask, s1, s0).repeat_interleave(patch, dim=1).repeat_interleave(patch, dim=2)[:, None]
    tok = torch.where(mask, timesteps_alt.view(B, 1, 1), timesteps.view(B, 1, 1)).flatten(1).contiguous()
    sT, tT = torch.minimum(sigma, sigma_alt), torch.minimum(timesteps, timesteps_alt)
    lat, n = latents.float(), noise.float()
    mix = lambda sg: ((1.0 - sg) * lat + sg * n).to(latents.dtype).contiguous()
    res = (mix(grid), mix(sT.view(B, 1, 1, 1)), tok, sT, tT)
    if out is not None:
        for dst, src in zip(out, res):
            EMU._need(dst.dtype == src.dtype and tuple(dst.shape) == tuple(src.shape) and dst.is_contiguous(), "self_flow_views: preallocated outputs")
            dst.copy_(src)
        res = tuple(out)
    return (*res, grid.contiguous() if want_sigma_grid else None)


def _params(name, gamma, beta, W, b):
    ts = (gamma, beta, W, b)
    EMU._need(all(t.dtype == F32 and t.is_contiguous() for t in ts), f"{name}: four contiguous fp32 tensors")
    EMU._need(W.dim() == 2 and W.shape[0] == W.shape[1], f"{name}: W [D, D]")
    D = W.shape[1]
    EMU._need(D % 8 == 0 and D <= 4096 and all(t.numel() == D for t in (gamma, beta, b)), f"{name}: D a multiple of 8, at most 4096; gamma, beta, b [D]")
    for t in (gamma, beta, W):
        EMU._al(t, 16, name)
    return D


def self_flow_fold(gamma, beta, W, b, Wf, WfT, c):
    D = _params("self_flow_fold", gamma, beta, W, b)
    EMU._need(all(t.dtype == EMU.BF16 and t.is_contiguous() for t in (Wf, WfT, c)) and tuple(Wf.shape) == (D, D) and tuple(WfT.shape) == (D, D) and c.numel() == D,
              "self_flow_fold: outputs")
    f = (W * gamma[None, :]).to(EMU.BF16)
    Wf.copy_(f); WfT.copy_(f.t())
    c.copy_((W @ beta + b).to(EMU.BF16))
    return Wf, WfT, c


def self_flow_rows(h, xhat, rstd):
    LS._view3(h, "h")
    B, rows, D = h.shape
    M = B * rows
    EMU._need(D % 64 == 0 and D <= 4096, "self_flow_rows: D must be a multiple of 64, at most 4096")
    EMU._need(xhat.dtype == EMU.BF16 and xhat.is_contiguous() and tuple(xhat.shape) == (M, D) and rstd.dtype == F32 and rstd.is_contiguous() and rstd.numel() == M,
              "self_flow_rows: xhat [M, D] bf16, rstd [M] fp32, contiguous")
    EMU._al(xhat, 16, "xhat")
    x = h.float().reshape(M, D)
    mean = x.mean(dim=-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + EPS)
    xhat.copy_(((x - mean) * rs).to(EMU.BF16))
    rstd.copy_(rs[:, 0])
    return xhat, rstd


def self_flow_wgrad(P, db, gamma, beta, W, scale, g_gamma, g_beta, g_W, g_b, accumulate=False):
    D = _params("self_flow_wgrad", gamma, beta, W, g_b)
    _params("self_flow_wgrad", g_gamma, g_beta, g_W, g_b)
    EMU._need(scale.dtype == F32 and scale.numel() == 1, "self_flow_wgrad: the scale is ONE fp32")
    EMU._need(P.dtype == EMU.BF16 and P.is_contiguous() and tuple(P.shape) == (D, D) and db.dtype == F32 and db.is_contiguous() and db.numel() == D, "self_flow_wgrad: P [D, D] bf16, db [D] fp32")
    EMU._al(P, 16, "P")
    s, Pf, d = scale.reshape(()), P.float(), db.reshape(-1)
    put = lambda dst, val: dst.copy_((dst + val) if accumulate else val)
    put(g_W, s * (Pf * gamma[None, :] + d[:, None] * beta[None, :]))
    put(g_b, s * d)
    put(g_gamma, s * (W * Pf).sum(dim=0))
    put(g_beta, s * (W * d[:, None]).sum(dim=0))
    return g_gamma, g_beta, g_W, g_b


STAND_INS = {"self_flow_views": self_flow_views, "self_flow_fold": self_flow_fold, "self_flow_rows": self_flow_rows, "self_flow_wgrad": self_flow_wgrad}


def install(monkeypatch):
    """tests.tlora_ref.install (the emulator and every earlier stand-in) + the Self-Flow stand-ins"""
    ops = TR.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side of the engine tests ----
def similarity_autograd(h, teacher, params):
    """the reference arithmetic on live autograd tensors: mean over tokens of <normalize(projector(h)), normalize(teacher.detach())>"""
    ga, be, W, b = params
    proj = F.linear(F.layer_norm(h, (h.shape[-1],), ga, be, EPS), W, b)
    return (F.normalize(proj, dim=-1) * F.normalize(teacher.detach(), dim=-1)).sum(dim=-1).mean()


def seed_projector(model, seed: int = 29):
    """projector parameters off their initial values (gamma = 1, beta = 0 would leave the affine's gradients the only non-trivial ones untested against a general fold)"""
    g = torch.Generator().manual_seed(seed)
    D = model.D
    vals = (1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(D, D, generator=g) / D ** 0.5, 0.05 * torch.randn(D, generator=g))
    own = dict(model.named_parameters())
    with torch.no_grad():
        for nm, v in zip(NAMES, vals):
            own[PREFIX + nm].copy_(v)
    return vals


def sd3_oracle_blocks(monkeypatch, model, ocfg, d, lat, t, lora, scale):
    """one forward of the oracle on (lat, t) with the given adapters: (prediction, the list of every joint block's image-stream output)"""
    from oracle import sd3 as OS
    from tests import parity_utils as PU
    outs = LS.record_sd3_blocks(monkeypatch)
    P, _, _ = PU.oracle_state(model)
    P = {k: v for k, v in P.items() if not k.startswith(PREFIX)}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    out = OS.sd3_forward(P, ocfg, lat.float(), d["prompt"].float(), d["pooled"].float(), t, lora=lora, lora_scale=scale)
    return out, outs

"""DoRA (`use_dora`; Liu et al. 2024, "DoRA: Weight-Decomposed Low-Rank Adaptation"; peft's DoraLinearLayer) restated — TEST INFRASTRUCTURE ONLY.

peft is not installed and the reference does not vendor it, so nothing here executes reference code: the rule is the published one,
    V = W + s B A,  norm_n = ||V[n, :]||_2 (DETACHED),  g = m / norm,  y = g . (x W^T + s (x A^T) B^T) + b,
which is peft's `base(x) + (g - 1) . (x W^T) + g . s B A x` with the bias outside the scale.

  * `dora64`: the fp64 restatement of forward and hand-derived backward (dm = (1 / norm) sum_rows dy . y0; dx, dA, dB those of a plain LoRA under g . dy).
  * `dora_autograd`: the same formula on live autograd tensors, `.detach()` on the norm (or not: the test that pins the choice).
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/dora.hip with the kernels' contracts (bf16 in memory, fp32 arithmetic, one bf16 rounding
    per store, in place into the tensors given); `install()` puts them on top of tests.lora_dropout_ref.install.
  * `dora_linear`: the oracle's `linear` with the DoRA row scale, to monkeypatch over oracle.sd3.linear from a test.
"""
import torch
import torch.nn.functional as F

from tests import lora_dropout_ref as LD
from tests import ops_emulator as EMU

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KEY = ".lora_magnitude_vector.default.weight"


# ---- the rule ----
def dora_autograd(x, W, b, A, Bm, m, s: float, detach: bool = True):
    V = W + s * (Bm @ A)
    norm = V.norm(dim=1)
    if detach:
        norm = norm.detach()
    g = m / norm
    y0 = x @ W.t() + s * ((x @ A.t()) @ Bm.t())
    y = g * y0
    return y if b is None else y + b


def dora64(x, W, b, A, Bm, m, s: float, dy):
    """fp64 closed forms: (y, dx, dA, dB, dm, g, norm)"""
    x, W, A, Bm, m, dy = (t.to(F64) for t in (x, W, A, Bm, m, dy))
    norm = (W + s * (Bm @ A)).norm(dim=1)
    g = m / norm
    T = x @ A.t()
    y0 = x @ W.t() + s * (T @ Bm.t())
    y = g * y0 + (0.0 if b is None else b.to(F64))
    dyg = dy * g
    U = s * (dyg @ Bm)
    return y, dyg @ W + U @ A, U.t() @ x, s * (dyg.t() @ T), (dy * y0).sum(0) / norm, g, norm


# ---- stand-ins with the kernels' contracts ----
def dora_fold(W, A_cat_T, B_blk, m, targets, r_pad, inv_norm, g, Wf, WfT, Bf, BfT, init=False):
    for t in (W, A_cat_T, B_blk, Wf, WfT, Bf, BfT):
        EMU._need(t.dtype == BF16 and t.is_contiguous(), "dora_fold: contiguous bf16 operands")
    for t in (m, inv_norm, g):
        EMU._need(t.dtype == F32 and t.is_contiguous(), "dora_fold: contiguous fp32 vectors")
    N, K = W.shape
    K2 = B_blk.shape[1]
    EMU._need(K % 8 == 0 and K2 % 64 == 0 and r_pad in (32, 64, 128) and 1 <= len(targets) <= 4 and len(targets) * r_pad <= K2, "dora_fold: shapes")
    EMU._need(tuple(A_cat_T.shape) == (K, K2) and tuple(B_blk.shape) == (N, K2) and tuple(Wf.shape) == (N, K) and tuple(WfT.shape) == (K, N)
              and tuple(Bf.shape) == (N, K2) and tuple(BfT.shape) == (K2, N) and m.numel() == inv_norm.numel() == g.numel() == N, "dora_fold: operand shapes")
    for i, (n_off, n) in enumerate(targets):
        rows, slab = slice(n_off, n_off + n), slice(i * r_pad, (i + 1) * r_pad)
        V = W[rows].float() + B_blk[rows, slab].float() @ A_cat_T[:, slab].float().t()
        norm = (V * V).sum(1).sqrt()
        if init:
            m[rows] = norm
        gv = m[rows] / norm
        inv_norm[rows] = 1.0 / norm
        g[rows] = gv
        Wf[rows] = (gv[:, None] * W[rows].float()).to(BF16)
        Bf[rows] = (gv[:, None] * B_blk[rows].float()).to(BF16)
        WfT[:, rows] = Wf[rows].t()
        BfT[:, rows] = Bf[rows].t()
    return g


def dora_y0_scratch(dev, M, N):
    return torch.empty(M, N, dtype=BF16, device=dev)


def dora_db_scratch(dev, N, rank):
    return torch.empty(N, rank, dtype=F32, device=dev)


def dora_dmag(dy, y0, inv_norm, dm, accumulate=False):
    EMU._need(dy.dtype == BF16 and y0.dtype == BF16 and inv_norm.dtype == F32 and dm.dtype == F32 and dy.stride(-1) == 1, "dora_dmag: dtypes")
    d2 = dy.reshape(-1, dy.shape[-1])
    EMU._need(tuple(y0.shape) == tuple(d2.shape) and d2.shape[1] % 8 == 0 and dm.numel() == d2.shape[1] == inv_norm.numel(), "dora_dmag: shapes")
    val = inv_norm * (d2.float() * y0.float()).sum(0)
    dm.copy_(dm + val if accumulate else val)
    return dm


def dora_db_finish(P, g, gB, accumulate=False):
    EMU._need(P.dtype == F32 and g.dtype == F32 and gB.dtype == F32 and P.shape == gB.shape and g.numel() == P.shape[0] and P.is_contiguous() and gB.is_contiguous(),
              "dora_db_finish: contiguous fp32 P / gB [N, rank], g [N]")
    val = g[:, None] * P
    gB.copy_(gB + val if accumulate else val)
    return gB


STAND_INS = {"dora_fold": dora_fold, "dora_y0_scratch": dora_y0_scratch, "dora_db_scratch": dora_db_scratch, "dora_dmag": dora_dmag, "dora_db_finish": dora_db_finish}


def install(monkeypatch):
    """tests.lora_dropout_ref.install (LayerSync, NextLat, LoRA dropout) + the Internal Guidance, Lion and Adafactor stand-ins + the DoRA stand-ins"""
    from tests import adafactor_ref, internal_guidance_ref, lion_bounds
    ops = LD.install(monkeypatch)
    for name, fn in internal_guidance_ref.STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    lion_bounds.install(monkeypatch)
    adafactor_ref.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side ----
def magnitudes(model, device="cpu"):
    """{adapted Linear's name: its magnitude vector (fp32, a detached copy)}"""
    return {n[:-len(KEY)]: p.detach().to(device, F32).clone() for n, p in model.named_parameters() if n.endswith(KEY)}


def dora_linear(mags: dict):
    """oracle.sd3.linear with the DoRA row scale on the adapted Linears: y = (m / ||W + s B A||.detach()) . (W x + s B A x) + b"""
    def linear(x, P, name, lora=None, lora_scale: float = 1.0):
        W, b = P[name + ".weight"], P.get(name + ".bias")
        if lora is None or name not in lora:
            return F.linear(x, W, b)
        A, Bm = lora[name]
        return dora_autograd(x, W, b, A.to(x.dtype), Bm.to(x.dtype), mags[name].to(x.dtype), lora_scale)
    return linear

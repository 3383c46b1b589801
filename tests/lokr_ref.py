"""LyCORIS LoKr (`lora_type=lycoris`, `algo: lokr`, both factors full) restated — TEST INFRASTRUCTURE ONLY.

The LyCORIS package is not installed and the reference does not vendor it, so nothing here executes LyCORIS code: the rule is the one the issue states,
    dW = s kron(w1, w2),  dW[i ok + k, j in + l] = s w1[i, j] w2[k, l],  y = x bf16(W + dW)^T + b   (the merged-weight forward),
with (ol, ok) = factorization(N, factor), (im, in) = factorization(K, factor).

  * `lokr_autograd`: the formula on live autograd tensors through torch.kron (round=True: the bf16 rounding of the merged weight, straight-through).
  * `lokr64`: the fp64 restatement of the forward and of the structured backward (mix, dw2, P, dw1, dx) — no [N, K] gradient is formed.
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/lokr.hip with the kernels' contracts (bf16 in memory, fp32 arithmetic, one bf16 rounding
    per store, in place into the tensors given); `install()` puts them on top of tests.dora_ref.install.
  * `lokr_linear`: the oracle's `linear` with the merged, rounded weight on the adapted Linears, to monkeypatch over oracle.sd3.linear from a test.
"""
import torch
import torch.nn.functional as F

from tests import dora_ref as DR
from tests import ops_emulator as EMU

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
K1, K2 = ".lokr_w1", ".lokr_w2"


# ---- the rule ----
def merged(W, w1, w2, s: float, round_bf16: bool = False):
    V = W + s * torch.kron(w1, w2)
    if round_bf16:          # the value the GEMM multiplies with; the rounding has no gradient (straight-through)
        V = V + (V.detach().to(BF16).to(V.dtype) - V.detach())
    return V


def lokr_autograd(x, W, b, w1, w2, s: float, round_bf16: bool = False):
    return F.linear(x, merged(W, w1, w2, s, round_bf16), b)


def lokr64(x, W, b, w1, w2, s: float, dy):
    """fp64 closed forms through the structure: (y, dx, dw1, dw2)"""
    x, W, w1, w2, dy = (t.to(F64) for t in (x, W, w1, w2, dy))
    (ol, im), (ok, in_) = w1.shape, w2.shape
    M = x.shape[0]
    Wm = W + s * torch.einsum("ij,kl->ikjl", w1, w2).reshape(ol * ok, im * in_)
    y = x @ Wm.t() + (0.0 if b is None else b.to(F64))
    dy3, x2 = dy.reshape(M, ol, ok), x.reshape(M * im, in_)
    dP = torch.einsum("ij,mik->mjk", w1, dy3)                        # the mix
    dw2 = s * (dP.reshape(M * im, ok).t() @ x2)
    P = (x2 @ w2.t()).reshape(M, im, ok)
    dw1 = s * torch.einsum("mik,mjk->ij", dy3, P)
    return y, dy @ Wm, dw1, dw2


# ---- stand-ins with the kernels' contracts ----
def lokr_fold(W, targets, s, Wf, WfT):
    for t in (W, Wf, WfT):
        EMU._need(t.dtype == BF16 and t.is_contiguous(), "lokr_fold: contiguous bf16 operands")
    N, K = W.shape
    EMU._need(K % 8 == 0 and 1 <= len(targets) <= 4 and tuple(Wf.shape) == (N, K) and tuple(WfT.shape) == (K, N), "lokr_fold: shapes")
    Wf.copy_(W)
    end = 0
    for (n_off, n, w1, w2, w2b) in targets:
        EMU._need(w1.dtype == F32 and w2.dtype == F32 and w2b.dtype == BF16 and w1.is_contiguous() and w2.is_contiguous() and w2b.is_contiguous(), "lokr_fold: factors")
        (ol, im), (ok, in_) = w1.shape, w2.shape
        EMU._need(ol <= 16 and im <= 16 and ok % 8 == 0 and in_ % 8 == 0 and ol * ok == n and im * in_ == K and n_off >= end and n_off + n <= N and w2b.shape == w2.shape,
                  "lokr_fold: ol, im <= 16, ok % 8 == 0, in % 8 == 0, the targets in rising row order")
        end = n_off + n
        a = (torch.tensor(float(s), dtype=F32) * w1)                                      # fl(s w1)
        d = torch.einsum("ij,kl->ikjl", a.double(), w2.double()).reshape(n, K)              # exact products of two fp32
        Wf[n_off:n_off + n] = (d + W[n_off:n_off + n].double()).to(F32).to(BF16)            # the fma's one rounding, then the bf16 store
        w2b.copy_(w2.to(BF16))
    WfT.copy_(Wf.t())
    return Wf


def lokr_scratch(which, dev, M, cols):
    return torch.empty(M, cols, dtype=BF16, device=dev)


def _rows(t):
    EMU._need(t.dtype == BF16 and t.stride(-1) == 1 and t.dim() in (2, 3), "lokr: a bf16 [M, C] operand or a [B, rows, C] view")
    return t.reshape(-1, t.shape[-1])


def lokr_mix(dy, n_off, w1, ok, out):
    d = _rows(dy)
    ol, im = w1.shape
    EMU._need(w1.dtype == F32 and out.dtype == BF16 and out.is_contiguous() and tuple(out.shape) == (d.shape[0], im * ok) and ok % 8 == 0 and n_off % 8 == 0
              and ol <= 16 and im <= 16 and n_off + ol * ok <= d.shape[1], "lokr_mix: shapes")
    acc = torch.zeros(d.shape[0], im, ok, dtype=F32)
    d3 = d[:, n_off:n_off + ol * ok].float().reshape(-1, ol, ok)
    for i in range(ol):                                                                     # the fma chain in rising i
        acc = (acc.double() + w1[i].double()[None, :, None] * d3[:, i].double()[:, None, :]).to(F32)
    out.copy_(acc.reshape(d.shape[0], im * ok).to(BF16))
    return out


def lokr_dw2(dP, x, im, out, alpha=1.0, accumulate=False):
    xr = _rows(x)
    M = xr.shape[0]
    ok, in_ = out.shape
    EMU._need(dP.dtype == BF16 and dP.is_contiguous() and out.dtype == F32 and out.is_contiguous() and tuple(dP.shape) == (M, im * ok) and xr.shape[1] == im * in_
              and ok % 8 == 0 and in_ % 8 == 0 and im <= 16, "lokr_dw2: shapes")
    val = float(alpha) * (dP.float().reshape(M * im, ok).t() @ xr.float().reshape(M * im, in_))
    out.copy_(out + val if accumulate else val)
    return out


def lokr_dw1(dy, n_off, P, out, ok, alpha=1.0, accumulate=False):
    d = _rows(dy)
    M = d.shape[0]
    ol, im = out.shape
    EMU._need(P.dtype == BF16 and P.is_contiguous() and out.dtype == F32 and out.is_contiguous() and tuple(P.shape) == (M, im * ok) and ok % 8 == 0 and n_off % 8 == 0
              and ol <= 16 and im <= 16 and n_off + ol * ok <= d.shape[1], "lokr_dw1: shapes")
    val = float(alpha) * torch.einsum("mik,mjk->ij", d[:, n_off:n_off + ol * ok].float().reshape(M, ol, ok), P.float().reshape(M, im, ok))
    out.copy_(out + val if accumulate else val)
    return out


STAND_INS = {"lokr_fold": lokr_fold, "lokr_scratch": lokr_scratch, "lokr_mix": lokr_mix, "lokr_dw2": lokr_dw2, "lokr_dw1": lokr_dw1}


def install(monkeypatch):
    """tests.dora_ref.install (the emulator and every stand-in on top of it) + the LoKr stand-ins"""
    ops = DR.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side ----
def factors_of(model, device="cpu"):
    """{adapted Linear's name: (w1, w2) fp32 detached copies}"""
    named = dict(model.named_parameters())
    return {n[:-len(K1)]: (p.detach().to(device, F32).clone(), named[n[:-len(K1)] + K2].detach().to(device, F32).clone()) for n, p in named.items() if n.endswith(K1)}


def lokr_linear(facs: dict, s: float, round_bf16: bool = True):
    """oracle.sd3.linear with the merged weight on the adapted Linears: y = x bf16(W + s kron(w1, w2))^T + b, whatever `lora` the caller passes"""
    def linear(x, P, name, lora=None, lora_scale: float = 1.0):
        W, b = P[name + ".weight"], P.get(name + ".bias")
        if name not in facs:
            return F.linear(x, W, b)
        w1, w2 = facs[name]
        return lokr_autograd(x, W, b, w1.to(x.dtype), w2.to(x.dtype), s, round_bf16)
    return linear

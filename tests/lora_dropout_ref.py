"""LoRA dropout (peft `lora_dropout`: y = base(x) + (alpha / r) B A dropout(x)) restated — TEST INFRASTRUCTURE ONLY.

  * `philox4x32_10`: Philox4x32-10 in plain torch integer arithmetic (int64 tensors holding 32-bit words; the 32 x 32 -> 64 bit products through 16-bit halves so
    nothing overflows), pinned to the Random123 known-answer vectors by tests/test_lora_dropout_cpu.py.
  * `keep_mask`: the counter lay-out of include/st355.h's st355_lora_drop — (c0, c1) = the 64-bit group index (row * K + col) / 8, c2 = the stream id, c3 = the
    call counter, key = (key0, key1); element j of a group takes bits 16 (j % 2) of word j / 2 and is dropped iff that 16-bit value < T = round(p * 65536).
  * plain-torch stand-ins for the `simpletuner_amd.ops` wrappers of csrc/lora_dropout.hip with the kernels' contracts (bf16 in memory, fp32 arithmetic, the scale
    on the fp32 sums, one bf16 rounding per store, in place into the tensors given); `install()` puts them on top of tests.nextlat_ref.install.
  * `masked_linear`: the oracle's `linear` with the mask on the adapter branch's input, to monkeypatch over oracle.sd3.linear / oracle.flux.linear from a test.
  * fp64 closed forms of the LoRA linear's forward and gradients under an explicit mask (`lora64`).
"""
import torch
import torch.nn.functional as F

from tests import nextlat_ref as NL
from tests import ops_emulator as EMU

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _mulhilo(m: int, a):
    """(high, low) 32-bit words of m * a for a 32-bit constant m and an int64 tensor a of 32-bit words: a = ah 2^16 + al, m a = (m ah) 2^16 + m al with every
    partial product below 2^48"""
    al, ah = a & 0xFFFF, a >> 16
    pl = al * m
    t = ah * m + (pl >> 16)                      # = floor(m a / 2^16), below 2^49
    return t >> 16, ((t & 0xFFFF) << 16) | (pl & 0xFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """ten rounds; c*: int64 tensors (or ints) of 32-bit words, broadcast together.  Returns the four output words as int64 tensors."""
    c = [torch.as_tensor(v, dtype=I64) & M32 for v in (c0, c1, c2, c3)]
    c = list(torch.broadcast_tensors(*c))
    k0, k1 = int(k0) & M32, int(k1) & M32
    for _ in range(10):
        hi0, lo0 = _mulhilo(PHILOX_M0, c[0])
        hi1, lo1 = _mulhilo(PHILOX_M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def threshold(p: float) -> int:
    return int(round(float(p) * 65536.0))


def scale_f32(T: int) -> torch.Tensor:
    """1 / (1 - p') with p' = T / 65536, rounded once to fp32"""
    return torch.tensor(1.0 / (1.0 - T / 65536.0), dtype=F32)


def key_of(seed: int, rank: int):
    """engine.LoraDropout's key: the seed's low word; its high word xor rank * 0x9E3779B9"""
    seed, rank = int(seed), int(rank)
    return seed & M32, ((seed >> 32) ^ (rank * 0x9E3779B9)) & M32


def lanes16(M: int, K: int, key, call: int, stream: int):
    """the 16-bit lane of every element of an [M, K] input: int64 [M, K]"""
    assert K % 8 == 0
    grp = torch.arange(M * (K // 8), dtype=I64)
    w = philox4x32_10(grp & M32, grp >> 32, int(stream) & M32, int(call) & M32, key[0], key[1])
    lanes = torch.stack([(w[j // 2] >> (16 * (j % 2))) & 0xFFFF for j in range(8)], dim=1)          # [groups, 8]
    return lanes.reshape(M, K)


def keep_mask(M: int, K: int, key, call: int, stream: int, T: int):
    """bool [M, K]: True = kept (lane >= T)"""
    return lanes16(M, K, key, call, stream) >= int(T)


class Drop:
    """the state object the wrappers take (engine.LoraDropout's attributes), on the host"""

    def __init__(self, p: float, seed: int = 0, rank: int = 0, calls: int = 0, device="cpu"):
        self.p, self.thr = float(p), threshold(p)
        self.key0, self.key1 = key_of(seed, rank)
        self.call = torch.zeros(1, dtype=torch.int32, device=device)
        self.set_calls(calls)

    def set_calls(self, calls: int):
        c = int(calls) & M32
        self.call.fill_(c - (1 << 32) if c >= (1 << 31) else c)

    def calls(self) -> int:
        return int(self.call.item()) & M32


def _state(drop):
    return (int(drop.key0) & M32, int(drop.key1) & M32), int(drop.call.item()) & M32, int(drop.thr)


def _keep(drop, stream, M, K):
    key, call, T = _state(drop)
    return keep_mask(M, K, key, call, stream, T)


def _rows2d(t):
    """a 2-D operand or a [B, rows, C] view as the [B * rows, C] logical rows (the mask's row index)"""
    return t.reshape(-1, t.shape[-1])


# ---- stand-ins with the kernels' contracts ----
def lora_dropout_threshold(p):
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"lora_dropout must lie in [0, 1), got {p}")
    T = threshold(p)
    if not 1 <= T <= 65535:
        raise ValueError(f"lora_dropout={p} rounds to the threshold {T} / 65536: outside the 16-bit lanes of the mask generator")
    return T


def lora_dropout_advance(call):
    EMU._need(call.dtype == torch.int32 and call.numel() == 1, "lora_dropout_advance: ONE int32")
    c = (int(call.item()) + 1) & M32
    call.fill_(c - (1 << 32) if c >= (1 << 31) else c)
    return call


def lora_dropout_mask(M, K, drop, stream):
    return _keep(drop, stream, M, K).to(torch.uint8)


def _group_checks(name, K, K2, r_pad, streams):
    EMU._need(K % 8 == 0, f"{name}: K % 8")
    EMU._need(r_pad in (32, 64, 128) and 1 <= len(streams) <= 4 and len(streams) * r_pad <= K2, f"{name}: r_pad 32 / 64 / 128, 1 .. 4 targets inside K2")


def lora_down_drop(x, A_cat, r_pad, streams, drop, out=None):
    EMU._need(x.dtype == BF16 and A_cat.dtype == BF16 and A_cat.is_contiguous() and x.stride(-1) == 1, "lora_down_drop: bf16 operands, unit inner stride")
    x2 = _rows2d(x)
    M, K = x2.shape
    K2 = A_cat.shape[0]
    EMU._need(A_cat.shape[1] == K, "lora_down_drop: A_cat [K2, K]")
    _group_checks("lora_down_drop", K, K2, r_pad, streams)
    if out is None:
        out = torch.empty(M, K2, dtype=BF16)
    EMU._need(out.dtype == BF16 and tuple(out.shape) == (M, K2), "lora_down_drop: out [M, K2] bf16")
    s = scale_f32(drop.thr)
    T = torch.zeros(M, K2, dtype=F32)
    xf, Af = x2.float(), A_cat.float()
    for g, st in enumerate(streams):
        c = slice(g * r_pad, (g + 1) * r_pad)
        T[:, c] = s * ((xf * _keep(drop, st, M, K)) @ Af[c].t())
    out.copy_(T.to(BF16))
    return out


def lora_dx_drop(dx, U, A_cat_T, r_pad, streams, drop):
    EMU._need(dx.dtype == BF16 and U.dtype == BF16 and A_cat_T.dtype == BF16 and A_cat_T.is_contiguous() and dx.stride(-1) == 1, "lora_dx_drop: bf16 operands")
    K, K2 = A_cat_T.shape
    M = dx.numel() // K
    EMU._need(dx.shape[-1] == K and tuple(U.shape) == (M, K2), "lora_dx_drop: dx [.., K], U [M, K2]")
    _group_checks("lora_dx_drop", K, K2, r_pad, streams)
    s = scale_f32(drop.thr)
    Uf, Af = U.float(), A_cat_T.float()
    add = torch.zeros(M, K, dtype=F32)
    for g, st in enumerate(streams):
        c = slice(g * r_pad, (g + 1) * r_pad)
        add += (Uf[:, c] @ Af[:, c].t()) * _keep(drop, st, M, K)
    dx.copy_((dx.float() + (s * add).view(dx.shape)).to(BF16))          # (a view is written through)
    return dx


def _strided_out(out, P, so_p, so_r, r_used):
    return torch.as_strided(out, (P, r_used), (so_p, so_r), out.storage_offset())


def skinny_tn_drop(Lm, R, out, so_p, so_r, r_used, stream, drop, alpha=1.0, accumulate=False):
    EMU._need(Lm.dtype == BF16 and R.dtype == BF16 and out.dtype == F32, "skinny_tn_drop: bf16 operands, fp32 out")
    L2, R2 = _rows2d(Lm), _rows2d(R)
    M, P = L2.shape
    EMU._need(R2.shape[0] == M and R2.shape[1] in (32, 64) and 0 < r_used <= R2.shape[1] and P % 8 == 0, "skinny_tn_drop: shapes")
    val = (alpha * scale_f32(drop.thr)) * ((L2.float() * _keep(drop, stream, M, P)).t() @ R2.float()[:, :r_used])
    o = _strided_out(out, P, so_p, so_r, r_used)
    o.copy_(o + val if accumulate else val)
    return out


def skinny_tn_drop_multi(Lm, R, outs, so_p, so_r, r_used, streams, drop, alpha=1.0, accumulate=False):
    EMU._need(Lm.dtype == BF16 and R.dtype == BF16 and all(o.dtype == F32 for o in outs), "skinny_tn_drop_multi: bf16 operands, fp32 outs")
    L2, R2 = _rows2d(Lm), _rows2d(R)
    M, P = L2.shape
    EMU._need(R2.shape[0] == M and R2.shape[1] >= 128 and 1 <= len(outs) <= 4 and len(streams) == len(outs) and 0 < r_used <= 32 and P % 8 == 0,
              "skinny_tn_drop_multi: shapes")
    for g, (o_, st) in enumerate(zip(outs, streams)):
        val = (alpha * scale_f32(drop.thr)) * ((L2.float() * _keep(drop, st, M, P)).t() @ R2.float()[:, 32 * g:32 * g + r_used])
        o = _strided_out(o_, P, so_p, so_r, r_used)
        o.copy_(o + val if accumulate else val)
    return outs


STAND_INS = {"lora_dropout_threshold": lora_dropout_threshold, "lora_dropout_advance": lora_dropout_advance, "lora_dropout_mask": lora_dropout_mask,
             "lora_down_drop": lora_down_drop, "lora_dx_drop": lora_dx_drop, "skinny_tn_drop": skinny_tn_drop, "skinny_tn_drop_multi": skinny_tn_drop_multi}


def install(monkeypatch):
    """tests.nextlat_ref.install + the LoRA-dropout stand-ins"""
    ops = NL.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side ----
def stream_ids(model):
    """{adapted Linear's name: its mask stream id} of a component"""
    return {name: st for g in model.lora_groups for (name, _, _), st in zip(g.targets, g.streams)}


def masked_linear(streams: dict, key, call: int, T: int):
    """oracle.flux.linear with dropout on the adapter branch: y = W x + b + lora_scale * B A (keep . x / (1 - p')), the mask of the Linear's stream over the logical
    rows of x ([B, rows, K] -> b * rows + s).  T = 0: the plain linear."""
    def linear(x, P, name, lora=None, lora_scale: float = 1.0):
        y = F.linear(x, P[name + ".weight"], P.get(name + ".bias"))
        if lora is not None and name in lora:
            A, Bm = lora[name]
            xa = x
            if T:
                K = x.shape[-1]
                keep = keep_mask(x.numel() // K, K, key, call, streams[name], T).view(x.shape)
                xa = x * keep.to(x.dtype) * (1.0 / (1.0 - T / 65536.0))
            y = y + lora_scale * F.linear(F.linear(xa, A.to(x.dtype)), Bm.to(x.dtype))
        return y
    return linear


def lora64(x, W, A, Bm, s: float, keep, scale: float, dy):
    """fp64 closed forms of y = x W^T + s ((x . keep) scale) A^T B^T and of its gradients for an upstream dy: (y, dx, dA, dB)"""
    x, W, A, Bm, dy = (t.to(F64) for t in (x, W, A, Bm, dy))
    xm = x * keep.to(F64) * scale
    T = xm @ A.t()
    y = x @ W.t() + s * (T @ Bm.t())
    U = s * (dy @ Bm)
    return y, dy @ W + (U @ A) * keep.to(F64) * scale, U.t() @ xm, s * (dy.t() @ T)

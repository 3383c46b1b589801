"""T-LoRA (LyCORIS `algo: tlora`: y_b = base(x_b) + s (mask_b . (x_b down^T)) up^T, mask_b = the first r_b rank columns) restated — TEST INFRASTRUCTURE ONLY.

  * `active_rank`: the rule of the reference's documentation/experimental/T_LORA.md in Python floats, written on its own (the engine's copy is
    simpletuner_amd.engine.tlora_active_rank); `active_rank_exact`: the same value from exact rational arithmetic where the exponent allows it.
  * `timestep_index`: int(t) of a timestep held in fp32 / bf16 / int64, clamped to the table.
  * `restate`: the mask kernel's contract as ONE dense torch.where over the logical [M, columns] operand — what the stand-in and the kernel are compared with.
  * `tlora_mask`: the plain-torch stand-in of `simpletuner_amd.ops.tlora_mask` with the kernel's contract (bf16, in place, 2-D or a [B, rows, C] view, survivors and
    padding columns not touched); `install()` puts it on top of tests.lokr_ref.install (the emulator and every other stand-in).
  * `masked_linear`: the oracle's `linear` with the per-sample rank mask on the adapter branch, to monkeypatch over oracle.sd3.linear from a test.
"""
import math
from fractions import Fraction

import torch
import torch.nn.functional as F

from tests import lokr_ref as LR
from tests import ops_emulator as EMU

F32, F64 = torch.float32, torch.float64          # (the storage type is read as EMU.BF16: this module binds no constant of its own)
DOWN, UP = ".lora_down.weight", ".lora_up.weight"


def active_rank(t: int, T: int, R: int, Rmin: int, alpha: float) -> int:
    return min(R, int(((T - t) / T) ** alpha * (R - Rmin)) + Rmin)


def active_rank_exact(t: int, T: int, R: int, Rmin: int, alpha) -> int:
    """exact: alpha an integer (a rational power) or 1/2 (floor of a square root by integer comparison)"""
    span = R - Rmin
    if Fraction(alpha).denominator == 1:
        v = Fraction(T - t, T) ** int(alpha) * span
        return min(R, math.floor(v) + Rmin)
    assert Fraction(alpha) == Fraction(1, 2)
    k = 0                                            # the largest k with k <= sqrt((T - t) / T) span, i.e. k^2 T <= (T - t) span^2
    while (k + 1) ** 2 * T <= (T - t) * span * span:
        k += 1
    return min(R, k + Rmin)


def rank_table(T: int, R: int, Rmin: int, alpha: float):
    return torch.tensor([active_rank(t, T, R, Rmin, alpha) for t in range(T + 1)], dtype=torch.int32)


def timestep_index(timesteps, T: int):
    """int64 [B]: int(t) (truncation towards zero) of every timestep as its dtype holds it, clamped to [0, T]"""
    t = timesteps.detach().reshape(-1)
    if t.dtype.is_floating_point:
        t = torch.nan_to_num(t.to(F64), nan=0.0).trunc()
    return t.to(torch.int64).clamp(0, T)


def restate(t, r_pad: int, rank: int, G: int, rows_per_sample: int, table, timesteps):
    """a NEW tensor of t's logical shape: column g r_pad + j of row m is +0 iff j >= table[int(timesteps[m // rows_per_sample])], g < G, j < rank"""
    t2 = t.reshape(-1, t.shape[-1])
    M, C = t2.shape
    r = table.to(torch.int64)[timestep_index(timesteps, table.numel() - 1)]                  # [B]
    r_row = r.repeat_interleave(rows_per_sample)                                              # [M]
    col = torch.arange(C)
    g, j = col // r_pad, col % r_pad
    dead = (g < G)[None] & (j < rank)[None] & (j[None] >= r_row[:, None])
    return torch.where(dead, torch.zeros((), dtype=t.dtype), t2).reshape(t.shape)


def tlora_mask(t, r_pad, rank, G, rows_per_sample, ranks_table, timesteps):
    EMU._need(t.dtype == EMU.BF16 and t.stride(-1) == 1 and t.dim() in (2, 3), "tlora_mask: a bf16 2-D operand or [B, rows, C] view")
    EMU._need(r_pad == 32 or (r_pad >= 64 and r_pad % 64 == 0), "tlora_mask: r_pad 32 or a multiple of 64")
    EMU._need(1 <= G <= 4 and 1 <= rank <= r_pad and G * r_pad <= t.shape[-1], "tlora_mask: 1 .. 4 targets of rank <= r_pad inside the operand")
    EMU._need(ranks_table.dtype == torch.int32 and ranks_table.dim() == 1 and ranks_table.numel() >= 2, "tlora_mask: int32 table [T + 1]")
    EMU._need(timesteps.dim() == 1 and timesteps.dtype in (F32, torch.bfloat16, torch.int64), "tlora_mask: [B] timesteps of fp32 / bf16 / int64")
    M = t.numel() // t.shape[-1]
    EMU._need(M == timesteps.numel() * rows_per_sample, "tlora_mask: M == B rows_per_sample")
    r = ranks_table.to(torch.int64)[timestep_index(timesteps, ranks_table.numel() - 1)].clamp(0, rank)
    v = t if t.dim() == 3 else t.unsqueeze(0)          # [segments, seg, C]: slices of the operand itself — a view is written through, nothing else is touched
    seg = v.shape[1]
    for b in range(timesteps.numel()):
        m0, m1 = b * rows_per_sample, (b + 1) * rows_per_sample          # sample b's logical rows
        for s in range(m0 // seg, (m1 - 1) // seg + 1):
            i0, i1 = max(m0, s * seg) - s * seg, min(m1, (s + 1) * seg) - s * seg
            for g in range(G):
                lo, hi = g * r_pad + int(r[b]), g * r_pad + rank
                if lo < hi:
                    v[s, i0:i1, lo:hi] = 0
    return t


STAND_INS = {"tlora_mask": tlora_mask}


# ---- the mask cases the stand-in (CPU) and the kernel (GPU) are both held to ----
MASK_B = 3
MASK_ROWS = (5, 77)
MASK_SHAPES = ((1, 4), (3, 4), (3, 32), (3, 64), (4, 128), (1, 33))          # (targets, rank)
MASK_LAYOUTS = ("compact", "view")
MASK_TIMESTEPS = ((0.0, 499.5, 1000.0), (0.99, 999.9, 499.5))                  # the five values over two batches of three
MASK_DTYPES = (F32, torch.bfloat16)          # (of the timesteps)
GUARD = 64                                                                     # bf16 elements in front of and behind the operand (128 bytes: rows stay 16-byte aligned)


def r_pad_of(rank: int) -> int:
    return 32 if rank <= 32 else (rank + 63) // 64 * 64          # engine.LoraGroup's rule


def _operand_view(whole, layout: str, rows: int, K2: int):
    body = whole[GUARD:whole.numel() - GUARD]
    return body.view(MASK_B * rows, K2) if layout == "compact" else body.view(MASK_B, rows + 9, K2)[:, 4:4 + rows]


def mask_operand(layout: str, rows: int, G: int, rank: int, device, seed: int = 0):
    """-> (whole, view): `whole` the 1-D bf16 buffer (guards, the operand and — `view` — the other stream's rows of a joint [B, S, C] buffer around it), filled with
    nonzero values; `view` the operand inside it: compact [B rows, K2], or the [B, rows, K2] rows [4, 4 + rows) of the joint buffer.  K2 = G r_pad rounded up to 64,
    so targets of 32 columns leave padding columns behind the last one."""
    r_pad = r_pad_of(rank)
    K2 = (G * r_pad + 63) // 64 * 64
    S = rows if layout == "compact" else rows + 9
    n = MASK_B * S * K2
    g = torch.Generator().manual_seed(seed)
    vals = (torch.rand(GUARD + n + GUARD, generator=g) + 0.5) * (torch.randint(0, 2, (GUARD + n + GUARD,), generator=g) * 2 - 1)
    whole = vals.to(EMU.BF16).to(device)
    return whole, _operand_view(whole, layout, rows, K2)


def bits(t):
    return t.contiguous().view(torch.int16)


def check_mask_case(fn, device, layout, rows, G, rank, ts, ts_dtype, seed=0, T=1000):
    """runs fn (an `ops.tlora_mask`) on one case and holds the whole buffer, bit for bit, to the dense restatement: the operand's dead columns are +0, its survivors,
    its padding columns, the guards and every other row of the joint buffer are what they were.  Returns the buffer after the call (on the host)."""
    r_pad = r_pad_of(rank)
    table = rank_table(T, rank, 1, 1.0)
    tt = torch.tensor(ts, dtype=F32).to(ts_dtype)
    whole, view = mask_operand(layout, rows, G, rank, device, seed)
    before = whole.detach().cpu().clone()
    K2 = view.shape[-1]
    want = before.clone()
    _operand_view(want, layout, rows, K2).copy_(restate(_operand_view(before, layout, rows, K2), r_pad, rank, G, rows, table, tt))
    out = fn(view, r_pad, rank, G, rows, table.to(device), tt.to(device))
    assert out is view
    got = whole.detach().cpu()
    assert torch.equal(bits(got), bits(want)), (layout, rows, G, rank, ts, ts_dtype)
    dead = int((bits(want) != bits(before)).sum())
    return got, dead


def install(monkeypatch):
    """tests.lokr_ref.install (the emulator and every stand-in on top of it) + the T-LoRA stand-in"""
    ops = LR.install(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    return ops


# ---- the oracle side ----
def factors_of(model, dtype=F64):
    """{adapted Linear's name: (down, up) detached copies}"""
    named = dict(model.named_parameters())
    return {n[:-len(DOWN)]: (p.detach().cpu().to(dtype).clone(), named[n[:-len(DOWN)] + UP].detach().cpu().to(dtype).clone()) for n, p in named.items() if n.endswith(DOWN)}


def masked_linear(facs: dict, scale: float, ranks):
    """oracle.sd3.linear with the T-LoRA branch: y_b = W x_b + bias + scale ((x_b down^T) . mask_b) up^T for every name in `facs`; ranks: the active rank of each
    sample (None: no mask).  The adapted Linears see x as [B, rows, K]."""
    def linear(x, P, name, lora=None, lora_scale: float = 1.0):
        y = F.linear(x, P[name + ".weight"], P.get(name + ".bias"))
        if name in facs:
            down, up = facs[name]
            T = F.linear(x, down.to(x.dtype))
            if ranks is not None:
                assert x.dim() == 3 and x.shape[0] == len(ranks)
                keep = (torch.arange(down.shape[0])[None] < torch.as_tensor(ranks)[:, None]).to(x.dtype)          # [B, r]
                T = T * keep[:, None, :]
            y = y + scale * F.linear(T, up.to(x.dtype))
        return y
    return linear

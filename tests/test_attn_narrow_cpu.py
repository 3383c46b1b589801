"""ST355_ATTN_NARROW on the CPU: the UNet's routing of 40- and 80-wide heads to the fused token-major attention (the two wrappers restated in fp32 torch), the
padded route exactly as before with the switch off, and the ABI listing of the three entry points."""
from pathlib import Path

import pytest
import torch

from tests import test_unet_host_sequencing_cpu as HS
from tests.test_attn_wide_cpu import LN2, _heads, _rows

ROOT = Path(__file__).resolve().parent.parent


def _narrow_fwd(q, k, v, o, lse2, B, H, Sq, Sk, d, scale, o_res=None):
    s = _heads(q, B, Sq, H) @ _heads(k, B, Sk, H).transpose(-1, -2) * scale
    lse2.copy_(torch.logsumexp(s, -1) / LN2)
    o32 = _rows(torch.softmax(s, -1) @ _heads(v, B, Sk, H))
    o.copy_(o32)
    if o_res is not None:
        o_res.copy_(o32 - o.float())


def _narrow_bwd(q, k, v, o, dO, lse2, dq, dk, dv, B, H, Sq, Sk, d, scale, o_res=None):
    Q, K, V, G = _heads(q, B, Sq, H), _heads(k, B, Sk, H), _heads(v, B, Sk, H), _heads(dO, B, Sq, H)
    out = _heads(o, B, Sq, H) if o_res is None else _heads(o, B, Sq, H) + _heads(o_res, B, Sq, H)
    p = torch.exp2(Q @ K.transpose(-1, -2) * (scale / LN2) - lse2[..., None])
    ds = p * (G @ V.transpose(-1, -2) - (G * out).sum(-1, keepdim=True))          # delta from sum_c dO (o + o_res)
    dq.copy_(_rows(ds @ K * scale)); dk.copy_(_rows(ds.transpose(-1, -2) @ Q * scale)); dv.copy_(_rows(p.transpose(-1, -2) @ G))


@pytest.mark.parametrize("switch", [True, False])
def test_the_switch_routes_40_and_80_wide_heads(monkeypatch, switch):
    """sd15_narrow_heads, forward and hand-written backward against the oracle at tests/test_unet_host_sequencing_cpu.py's tolerances: switch on -> every
    attention (two widths, self with o_res and cross without) on _attention_narrow and no head split; off -> none, the padded route as before"""
    from simpletuner_amd import ops
    seen = {"fwd": [], "bwd": [], "split": 0}
    split = HS.EMU.head_split
    monkeypatch.setattr(ops, "ATTN_NARROW", switch)
    monkeypatch.setattr(ops, "attn_narrow_fwd", lambda *a, o_res=None: (seen["fwd"].append((a[9], o_res is not None)), _narrow_fwd(*a, o_res=o_res))[1])
    monkeypatch.setattr(ops, "attn_narrow_bwd", lambda *a, o_res=None: (seen["bwd"].append((a[13], o_res is not None)), _narrow_bwd(*a, o_res=o_res))[1])
    monkeypatch.setattr(HS.EMU, "head_split", lambda *a, **kw: (seen.__setitem__("split", seen["split"] + 1), split(*a, **kw))[1])
    HS.test_full_finetune_gradients_through_the_emulator_match_autograd(monkeypatch, "sd15_narrow_heads")
    # seven transformers (two down, mid, four up), self (o_res kept) + cross (none) attention each; the padded route splits q, k and v of every attention
    want = sorted([(40, True), (40, False)] * 3 + [(80, True), (80, False)] * 4)
    assert (sorted(seen["fwd"]), sorted(seen["bwd"]), seen["split"]) == ((want, want, 0) if switch else ([], [], 42)), seen


def test_abi_lists_the_three_narrow_attention_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    for n in ("st355_attn_narrow_fwd", "st355_attn_narrow_bwd", "st355_attn_narrow_bwd_workspace"):
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    if Path(lib.LIB_PATH).exists():
        assert all(hasattr(lib.load(), n) for n in lib.SYMBOLS if "attn_narrow" in n)

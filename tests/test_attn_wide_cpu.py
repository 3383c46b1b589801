"""ST355_ATTN_WIDE on the CPU: the UNet's routing of 160-wide heads to the fused token-major attention (the two wrappers restated in fp32 torch), the unchanged
routing and launch stream with the switch off, and the ABI listing of the three entry points."""
import hashlib
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import test_unet_host_sequencing_cpu as HS

ROOT = Path(__file__).resolve().parent.parent
LN2 = math.log(2.0)


def _heads(t, B, S, H):          # token-major column block [B S, H d] (any row stride) -> fp32 [B, H, S, d]
    return t.float().reshape(B, S, H, -1).permute(0, 2, 1, 3)


def _rows(t):                    # [B, H, S, d] -> [B S, H d]
    B, H, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * d)


def _wide_fwd(q, k, v, o, lse2, B, H, Sq, Sk, d, scale):
    s = _heads(q, B, Sq, H) @ _heads(k, B, Sk, H).transpose(-1, -2) * scale
    lse2.copy_(torch.logsumexp(s, -1) / LN2)
    o.copy_(_rows(torch.softmax(s, -1) @ _heads(v, B, Sk, H)))


def _wide_bwd(q, k, v, dO, lse2, dq, dk, dv, B, H, Sq, Sk, d, scale):
    Q, K, V, G = _heads(q, B, Sq, H), _heads(k, B, Sk, H), _heads(v, B, Sk, H), _heads(dO, B, Sq, H)
    p = torch.exp2(Q @ K.transpose(-1, -2) * (scale / LN2) - lse2[..., None])
    dp = G @ V.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))          # delta from sum_j P dP: O is not an operand
    dq.copy_(_rows(ds @ K * scale)); dk.copy_(_rows(ds.transpose(-1, -2) @ Q * scale)); dv.copy_(_rows(p.transpose(-1, -2) @ G))


@pytest.mark.parametrize("switch", [True, False])
def test_the_switch_routes_160_wide_heads(monkeypatch, switch):
    """sd15_wide_heads, forward and hand-written backward against the oracle at tests/test_unet_host_sequencing_cpu.py's tolerances: switch on -> _attention_wide
    (self and cross attention of every transformer, forward and backward), off -> _attention_unfused exactly as before"""
    from simpletuner_amd import ops
    from simpletuner_amd.unet.unet import UNet2DConditionModel as U
    seen = {"fwd": 0, "bwd": 0, "unfused": 0}
    count = lambda key, fn: (lambda *a, **kw: (seen.__setitem__(key, seen[key] + 1), fn(*a, **kw))[1])
    monkeypatch.setattr(ops, "ATTN_WIDE", switch)
    monkeypatch.setattr(ops, "attn_wide_fwd", count("fwd", _wide_fwd))
    monkeypatch.setattr(ops, "attn_wide_bwd", count("bwd", _wide_bwd))
    monkeypatch.setattr(U, "_attention_unfused", count("unfused", U._attention_unfused))
    HS.test_full_finetune_gradients_through_the_emulator_match_autograd(monkeypatch, "sd15_wide_heads")
    # four transformers at the 160-wide level (down, mid, two up), self + cross attention each
    assert seen == ({"fwd": 8, "bwd": 8, "unfused": 0} if switch else {"fwd": 0, "bwd": 0, "unfused": 8}), seen


def test_launch_stream_with_the_switch_off_is_the_parents(tmp_path):
    """tools/launch_trace.py over the UNet engine tests gives, byte for byte, the file it gave at the parent commit (tests/golden/attn_wide_flag_off_launch_trace.sha256)"""
    out = tmp_path / "trace.txt"
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "launch_trace.py"), str(out), "-k", "unet_host_sequencing"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = (ROOT / "tests" / "golden" / "attn_wide_flag_off_launch_trace.sha256").read_text().strip()
    assert out.stat().st_size > 10000 and hashlib.sha256(out.read_bytes()).hexdigest() == want


def test_abi_lists_the_three_wide_attention_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    for n in ("st355_attn_wide_fwd", "st355_attn_wide_bwd", "st355_attn_wide_bwd_workspace"):
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    if Path(lib.LIB_PATH).exists():
        assert all(hasattr(lib.load(), n) for n in lib.SYMBOLS if "attn_wide" in n)

"""ST355_ATTN_D72 on the CPU: PixArt's routing of its 72-wide heads to the fused token-major attention (the two wrappers restated in fp32 torch, pad lanes
zeroed), against the padded route with the switch off."""
import torch

from tests import ops_emulator as EMU
from tests import test_pixart_host_sequencing_cpu as HS
from tests.test_attn_wide_cpu import LN2


def _lanes(t, B, S, H, d):          # column block [B S, H pitch] -> fp32 [B, H, S, d]: the data lanes of every head
    return t.float().reshape(B, S, H, -1)[..., :d].permute(0, 2, 1, 3)


def _put(dst, x):                   # [B, H, S, d] -> the data lanes of a column block, zeros on its pad lanes
    B, H, S, d = x.shape
    dst.zero_()
    dst.unflatten(1, (H, -1))[:, :, :d].copy_(x.permute(0, 2, 1, 3).reshape(B * S, H, d))


def _scores(q, k, B, H, Sq, Sk, d, scale, key_bias):
    s = _lanes(q, B, Sq, H, d) @ _lanes(k, B, Sk, H, d).transpose(-1, -2) * scale
    return s if key_bias is None else s + key_bias[:, None, None, :]


def _d72_fwd(q, k, v, o, lse2, B, H, Sq, Sk, d, scale, pitch=None, key_bias=None):
    s = _scores(q, k, B, H, Sq, Sk, d, scale, key_bias)
    lse2.copy_(torch.logsumexp(s, -1) / LN2)
    _put(o, torch.softmax(s, -1) @ _lanes(v, B, Sk, H, d))


def _d72_bwd(q, k, v, o, dO, lse2, dq, dk, dv, B, H, Sq, Sk, d, scale, pitch=None, key_bias=None):
    Q, K, V, G = _lanes(q, B, Sq, H, d), _lanes(k, B, Sk, H, d), _lanes(v, B, Sk, H, d), _lanes(dO, B, Sq, H, d)
    p = torch.exp2(_scores(q, k, B, H, Sq, Sk, d, scale, key_bias) / LN2 - lse2[..., None])
    ds = p * (G @ V.transpose(-1, -2) - (G * _lanes(o, B, Sq, H, d)).sum(-1, keepdim=True))          # delta from the bf16 o
    _put(dq, ds @ K * scale); _put(dk, ds.transpose(-1, -2) @ Q * scale); _put(dv, p.transpose(-1, -2) @ G)


def _lora_step(monkeypatch, switch, seen):
    """tests/test_pixart_host_sequencing_cpu.py's trunk-LoRA case (no TREAD): prediction and every adapter gradient"""
    from simpletuner_amd import ops
    from simpletuner_amd.pixart.transformer import PixArtTransformer2DModel
    EMU.install(monkeypatch)
    monkeypatch.setattr(ops, "ATTN_D72", switch)
    monkeypatch.setattr(ops, "attn_d72_fwd", lambda *a, **kw: (seen.append(("fwd", a[7] == a[8], kw.get("key_bias") is not None)), _d72_fwd(*a, **kw))[1])
    monkeypatch.setattr(ops, "attn_d72_bwd", lambda *a, **kw: (seen.append(("bwd", a[11] == a[12], kw.get("key_bias") is not None)), _d72_bwd(*a, **kw))[1])
    m = PixArtTransformer2DModel(device="cpu", **HS.ARCH)
    m.init_synthetic(5)
    m.add_lora_adapter(rank=8, alpha=16.0, init_b_std=0.05)
    m.train()
    lat, _, enc, mask, t = HS._inputs()
    out = m(lat, encoder_hidden_states=enc, timestep=t, encoder_attention_mask=mask, return_dict=False)[0]
    (out.float() ** 2).mean().backward()
    return out.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if ".lora_" in n}


def test_the_switch_routes_pixart_attention_to_the_d72_wrappers(monkeypatch):
    """switch on: every block's self-attention (Sq == Sk, no bias) and cross-attention (the caption mask's bias) on attn_d72_fwd / _bwd, the prediction and every
    adapter gradient within the host-sequencing test's tolerances (2e-2 / 6e-2 rel-L2) of the switch-off run; switch off: the wrappers are never called"""
    on, off = [], []
    out1, g1 = _lora_step(monkeypatch, True, on)
    out0, g0 = _lora_step(monkeypatch, False, off)
    n = HS.ARCH["num_layers"]
    assert not off and sorted(on) == sorted([(w, s, not s) for w in ("fwd", "bwd") for s in (True, False)] * n), (on, off)
    assert HS._rel(out1, out0) < 2e-2
    for k in g0:
        assert HS._rel(g1[k], g0[k]) < 6e-2, (k, HS._rel(g1[k], g0[k]))

"""AutoencoderKL._mid_attention's routing under ops.VAE_ATTN_FUSED (ST355_VAE_ATTN) on the CPU emulator (tests/ops_emulator.py has no attn_d512_fwd: the wrapper is
patched here): off — the fused wrapper is never reached; on at mid width 512 — one call on the qkv buffer's column blocks replaces the per-image loop and the
decode still matches the oracle; on at mid width 128 — the old path."""
import math

import pytest
import torch

from oracle.vae import VAEConfig, decode
from tests import ops_emulator as EMU


def _torch_attention(q, k, v, o, lse2, B, H, Sq, Sk, d, scale):
    assert lse2 is None and H == 1 and q.stride(0) == k.stride(0) == v.stride(0) == 3 * d and k.data_ptr() - q.data_ptr() == 2 * d      # thirds of one buffer
    p = torch.softmax(q.float().view(B, Sq, d) @ k.float().view(B, Sk, d).transpose(1, 2) * scale, -1)
    o.copy_((p @ v.float().view(B, Sk, d)).view(B * Sq, d))


@pytest.mark.parametrize("switch,mid,want_calls", [(False, 512, 0), (True, 512, 1), (True, 128, 0)])
def test_mid_attention_routing_on_the_emulator(monkeypatch, switch, mid, want_calls):
    ops = EMU.install(monkeypatch)
    from simpletuner_amd.vae.autoencoder_kl import AutoencoderKL
    calls = []
    monkeypatch.setattr(ops, "VAE_ATTN_FUSED", switch)
    monkeypatch.setattr(ops, "attn_d512_fwd", lambda *a: (calls.append(a[5:]), _torch_attention(*a))[1])
    cfg = VAEConfig(block_out_channels=(64, 64, 128, mid))
    vae = AutoencoderKL(block_out_channels=cfg.block_out_channels, device="cpu")
    sd = vae.synthetic_state_dict(5, decoder=True)
    vae.load_state_dict(sd)
    z = torch.randn(2, cfg.latent_channels, 12, 8, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    got = vae.decode(z).sample
    assert calls == [(2, 1, 96, 96, 512, 1.0 / math.sqrt(512))][:want_calls]
    ref = decode(sd, cfg, z.float())
    assert ((got.float() - ref).norm() / ref.norm()).item() < 2e-2

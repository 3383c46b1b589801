"""The fused head_dim-512 forward attention (csrc/attention_d512.hip) on token-major column blocks, element-wise against the fp64 model of tests/attn_bounds.py
(O and lse2), inside sentinel buffers, launched twice (bit-identical), with and without lse2; the refusals by name; and the AutoencoderKL with ST355_VAE_ATTN on
(mid width 512): the C entry point, the per-kernel sequencing and the decoder all take the fused route, against the fp32 oracle.

The model's rounding points are the kernel's: one fp32 chain over d per score; P rounded to bf16 once; l sums the fp32 values.  Its per-tile terms hold as they
stand: a lane adds its 8 exponentials of a 32-key tile in 3 levels and folds them into l with one fma (the rescale), the four lane groups of a query meet once
at the end — Sk / 8 + 2 roundings on any path to l against the model's Sk + 2 ceil(Sk / 64); O sees one MFMA chain of 32 keys and one rescale per tile,
Sk + ceil(Sk / 32) <= Sk + 2 ceil(Sk / 64) + 8.  The aggregate cap beside the bound is the wide test's rel-L2 < 8e-3: a torch restatement of the rounding points
(fp32 scores, bf16 P, fp32 l) gives 1.2e-3 .. 1.7e-3 on these inputs."""
import math

import pytest
import torch

from oracle.vae import VAEConfig, decode, encode_moments
from tests import attn_bounds as AB
from tests.test_attn_bounds_gpu import _bits, _guard, _sent, dev
from tests.test_attn_wide_gpu import _blocks, _data

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
D_HEAD = 512
# (B, H, Sq, Sk, self): one exact query block | the small VAE's S: ragged query block, ragged key tile, batch stride | second head's column offset, Sq % 8 != 0,
# a 13-key last tile | everything inside one partial tile | ten key tiles: the staging ring wraps
CASES = [(1, 1, 64, 64, True), (2, 1, 96, 96, True), (1, 2, 200, 77, False), (1, 1, 7, 2, False), (1, 1, 320, 320, True)]


@pytest.mark.parametrize("B,H,Sq,Sk,self_attn", CASES)
def test_d512_attention_against_the_fp64_bounds(B, H, Sq, Sk, self_attn):
    from simpletuner_amd import ops
    d, D, scale = D_HEAD, H * D_HEAD, 1.0 / math.sqrt(D_HEAD)
    name = f"d512 B{B} H{H} Sq{Sq} Sk{Sk}"
    g = torch.Generator(device=dev()).manual_seed(Sq + Sk)
    q, k, v, _ = _data(g, B, H, Sq, Sk, d, 3.0 if self_attn else 0.0, scale)
    _, (q2, k2, v2), _ = _blocks(B, Sq, Sk, D, self_attn, fill=(q, k, v))
    inside = torch.zeros(B * Sq + 7, D + 32, dtype=torch.bool, device=dev())
    inside[:B * Sq, :D] = True
    runs = []
    for with_lse in (True, True) + ((False,) if Sq == 96 else ()):
        O_buf, lse_buf = _sent((B * Sq + 7, D + 32)), _sent((B * H * Sq + 64,), torch.float32)
        O, lse2 = O_buf[:B * Sq, :D], lse_buf[:B * H * Sq].view(B, H, Sq)
        before = _bits(O_buf).clone(), _bits(lse_buf).clone()
        ops.attn_d512_fwd(q2, k2, v2, O, lse2 if with_lse else None, B, H, Sq, Sk, d, scale)
        torch.cuda.synchronize()
        _guard(f"{name} O", O_buf, inside, before[0])
        if with_lse:
            _guard(f"{name} lse2", lse_buf, torch.arange(lse_buf.numel(), device=dev()) < B * H * Sq, before[1])
        else:
            assert torch.equal(_bits(lse_buf), before[1]), f"{name}: lse2=None wrote the buffer it was not given"
        runs.append((O, lse2))
    assert all(torch.equal(_bits(r[0]), _bits(runs[0][0])) for r in runs[1:]), f"{name}: O differs between launches / with and without lse2"
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), f"{name}: lse2 differs between launches"
    O, lse2 = runs[0]
    heads = lambda t2d, S_: t2d.reshape(B, S_, H, d).permute(0, 2, 1, 3)
    f = AB.attn_fwd_model(q, k, v, scale)
    reps = [AB.check(f"{name} O", heads(O, Sq), f.O, f.e_O, f.var_O), AB.check_lse2(f"{name} lse2", lse2, f.lse2, f.e_lse2)]
    r = AB.rel_l2(heads(O, Sq), f.O)
    print(f"{name}: O rel-L2 {r:.2e}")
    for rep in reps:
        AB.assert_bound(rep)
    assert r < 8e-3


@pytest.mark.parametrize("d", [160, 256])
def test_other_head_widths_are_refused_by_name(d):
    from simpletuner_amd import lib, ops
    t = torch.zeros(64, 2 * d, dtype=BF16, device=dev())
    with pytest.raises(lib.St355Error, match=rf"rc=-38\): attn_d512_fwd: head_dim {d} not built"):          # ST355_ENOSYS
        ops.attn_d512_fwd(t, t, t, torch.empty_like(t), None, 1, 2, 64, 64, d, 0.1)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("kind", ["sdxl", "flux"])
def test_vae_with_the_switch_on(monkeypatch, kind):
    """96 x 64 px, widths (64, 64, 128, 512): S = 96 tokens at mid width 512.  encode_moments (the C entry point) and decode against the fp32 oracle at the
    suite's 2e-2, the entry point bit-equal to the per-kernel sequencing under the same switch, one fused call per mid block, a smaller workspace."""
    import ctypes as C

    from simpletuner_amd import lib, ops
    from simpletuner_amd.vae.autoencoder_kl import AutoencoderKL
    from tests import test_vae_gpu as TV
    widths = (64, 64, 128, 512)
    cfg = VAEConfig(block_out_channels=widths) if kind == "sdxl" else VAEConfig(latent_channels=16, scaling_factor=0.3611, shift_factor=0.1159,
                                                                                use_quant_conv=False, block_out_channels=widths)
    vae = AutoencoderKL(latent_channels=cfg.latent_channels, block_out_channels=widths, scaling_factor=cfg.scaling_factor, shift_factor=cfg.shift_factor,
                        use_quant_conv=cfg.use_quant_conv, device="cuda:0")
    sd = vae.synthetic_state_dict(3, decoder=True)
    vae.load_state_dict(sd)
    x = torch.randn(2, 3, 96, 64, generator=torch.Generator().manual_seed(1)).clamp(-1, 1).to(BF16)
    z = torch.randn(2, cfg.latent_channels, 12, 8, generator=torch.Generator().manual_seed(2)).to(BF16)
    ref_m, ref_d = encode_moments(sd, cfg, x.float()), decode(sd, cfg, z.float())
    unfused = _rel(vae.encode_moments(x.to("cuda:0")).cpu(), ref_m), _rel(vae.decode(z.to("cuda:0")).sample.cpu(), ref_d)

    calls, fwd = [], ops.attn_d512_fwd
    monkeypatch.setattr(ops, "VAE_ATTN_FUSED", True)
    monkeypatch.setattr(ops, "attn_d512_fwd", lambda *a, **kw: (calls.append(a[5:10]), fwd(*a, **kw))[1])
    got_m = vae.encode_moments(x.to("cuda:0"))
    assert calls == []                                       # the entry point launches the kernel itself
    got_d = vae.decode(z.to("cuda:0")).sample
    assert calls == [(2, 1, 96, 96, 512)], calls
    fused = _rel(got_m.cpu(), ref_m), _rel(got_d.cpu(), ref_d)
    print(f"[vae {kind} mid 512] moments rel-L2 fused {fused[0]:.3e} unfused {unfused[0]:.3e}; decode rel-L2 fused {fused[1]:.3e} unfused {unfused[1]:.3e}")
    assert fused[0] < 2e-2 and fused[1] < 2e-2

    # the per-kernel sequencing of tests/test_vae_gpu.py under the same switch: bit-equal moments, one more wrapper call
    monkeypatch.setattr(TV, "VAEConfig", lambda **kw: VAEConfig(**dict(kw, block_out_channels=widths)))
    TV.test_vae_encode_c_entry_point_equals_the_per_kernel_sequencing(kind, (96, 64))
    assert len(calls) == 2, calls

    # dry runs at 2048^2 (S = 65536: the [S, S] scores are the workspace's peak): the fused route reports less
    st = vae._encoder_table().struct
    L = lib.load()
    ws = [L.st355_vae_encode_workspace_flags(C.byref(st), 1, 2048, 2048, f) for f in (0, 1)]
    assert 0 < ws[1] < ws[0] and ws[0] == L.st355_vae_encode_workspace(C.byref(st), 1, 2048, 2048), ws

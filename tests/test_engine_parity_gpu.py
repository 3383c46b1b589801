"""The device's gradients, every slab, no skip.  On the MI355X the engines run bf16 kernels, so the yardstick is rounding noise — taken from the REFERENCE side: a CPU twin
of the device model (same weights, same adapter state, same inputs) run through the kernel-contract emulator at bf16 (tests/ops_emulator.py, inside the kernels' fp64
bounds wrapper by wrapper).  Per slab (tests/engine_parity.py; slabs under 1024 elements pooled per block and kind)

    E_gpu = ||g_gpu - g_ref64||,  E_emu = ||g_emu - g_ref64||,      E_gpu <= 3 * E_emu + 1/2 ulp_bf16(||slab||_inf) * sqrt(n)

with g_ref64 autograd on the fp64 oracle.  The two errors are independent draws of one rounding model, so the ratio of their norms concentrates near 1; the 3 covers
accumulation orders and fused paths that round less or elsewhere than the host sequencing; the last term is the one store rounding both sides share.  A slab over 3
means a leaf's rounding points differ between the device path and the emulator (or a gradient term is wrong): find it — the constant is not set from the device.

The model GPU tests (tests/test_*_model_gpu.py) stay: whole-tensor parity through the plugin surface.  Shapes: the CPU case tables' (width 128, 2-3 blocks)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.pixart import PixArtConfig, controlnet_forward, pixart_forward  # noqa: E402
from oracle.unet import UNetConfig, unet_forward  # noqa: E402
from tests import engine_parity as EP  # noqa: E402
from tests import ops_emulator as EMU  # noqa: E402
from tests import parity_utils as PU  # noqa: E402
from tests import test_engine_algebra_cpu as ALG  # noqa: E402
from tests import test_flux_host_sequencing_cpu as FX  # noqa: E402
from tests import test_pixart_host_sequencing_cpu as PX  # noqa: E402
from tests import test_sd3_host_sequencing_cpu as S3  # noqa: E402
from tests import test_unet_host_sequencing_cpu as UN  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64


def _copy_params(src, dst):
    """the twin's parameters := the device model's, name by name"""
    a, b = dict(src.named_parameters()), dict(dst.named_parameters())
    assert a.keys() == b.keys(), sorted(a.keys() ^ b.keys())[:5]
    with torch.no_grad():
        for k, p in a.items():
            b[k].data.copy_(p.data)
    if hasattr(dst, "_prepared"):
        dst._prepared = False


def _cpu(grads):
    return {k: (None if g is None else g.detach().float().cpu()) for k, g in grads.items()}


def _to_dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _finish(case, gpu, emu, ref64, width, pred):
    rep = EP.check_device(case, _cpu(gpu), _cpu(emu), ref64, width, {"prediction": pred})
    EP.record_device(rep)
    rep.assert_ok()


# ------------------------------------------------------------------------------------------------
# Flux: default fast paths on (fused QKV, block entry points) on the device; the twin sequences the blocks from the host
# ------------------------------------------------------------------------------------------------
def _flux_seed(model, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm_q" in name or "norm_k" in name or "norm_added" in name:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p.shape[1] ** 0.5))


def _flux_run(model, d):
    out = model(hidden_states=d["packed"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], img_ids=d["img_ids"], txt_ids=d["txt_ids"],
                guidance=d["guidance"], return_dict=False)[0]
    ((out.float() - d["target"].float()) ** 2).mean().backward()
    return out.detach().float().cpu(), ALG._engine_grads(model)


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full-rank"])
def test_flux_device_gradients_slab_by_slab(monkeypatch, full):
    from simpletuner_amd.flux import transformer as T
    assert T._FUSED_QKV and T._BLOCK_ABI                      # the default fast paths
    arch = PU.small_flux_cfg(layers=2, single=2)

    def build(device):
        return T.FluxTransformer2DModel(device=device, **arch)

    def arm(m):
        if full:
            m.enable_full_finetune()
        else:
            m.add_lora_adapter(rank=16, alpha=16.0, targets="all", init_b_std=0.02)

    dev = build(DEV)
    _flux_seed(dev)
    arm(dev)
    d = FX._inputs(2, 16, 8, 24)
    out_g, g_gpu = _flux_run(dev, _to_dev(d))
    torch.cuda.synchronize()
    g_gpu = _cpu(g_gpu)
    EMU.install(monkeypatch)
    monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
    twin = build("cpu")
    _flux_seed(twin)
    arm(twin)
    _copy_params(dev, twin)
    out_e, g_emu = _flux_run(twin, d)
    o64, _, g64 = ALG._flux_oracle(twin, ALG._wide(d), F64)
    _finish(f"flux {'full-rank' if full else 'LoRA all'} 2+2 B2", g_gpu, g_emu, g64, twin.D, (out_g, out_e, o64))


# ------------------------------------------------------------------------------------------------
# SD3 / SD3.5
# ------------------------------------------------------------------------------------------------
def _sd3_seed(model, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".norm_q." in name or ".norm_k." in name or ".norm_added_" in name:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = model.config
        model.pos_embed.pos_embed.copy_(T.sincos_2d(model.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])


def _sd3_run(model, d):
    out = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0]
    ((out.float() - d["target"].float()) ** 2).mean().backward()
    return out.detach().float().cpu(), ALG._engine_grads(model)


@pytest.mark.parametrize("mode,sd35", [("lora", False), ("full", False), ("full", True)], ids=["lora-r16", "full", "sd35-full"])
def test_sd3_device_gradients_slab_by_slab(monkeypatch, mode, sd35):
    """LoRA r16; full fine-tune (3 blocks, B 2, 16x24, text 33); SD3.5 dual attention + q/k RMSNorm weights"""
    from simpletuner_amd.sd3 import transformer as T
    arch = S3._arch(3, **(dict(qk_norm="rms_norm", dual=(0, 1)) if sd35 else {}))

    def build(device):
        m = T.SD3Transformer2DModel(device=device, **arch)
        _sd3_seed(m, T)
        if mode == "full":
            m.enable_full_finetune()
        else:
            m.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
        return m

    dev = build(DEV)
    d = S3._inputs(2, 16, 24, 33)
    out_g, g_gpu = _sd3_run(dev, _to_dev(d))
    torch.cuda.synchronize()
    g_gpu = _cpu(g_gpu)
    EMU.install(monkeypatch)
    twin = build("cpu")
    _copy_params(dev, twin)
    out_e, g_emu = _sd3_run(twin, d)
    o64, _, g64 = ALG._sd3_oracle(twin, ALG._wide(d), F64)
    _finish(f"sd3{'.5' if sd35 else ''} {mode} L3 B2", g_gpu, g_emu, g64, twin.D, (out_g, out_e, o64))


# ------------------------------------------------------------------------------------------------
# PixArt
# ------------------------------------------------------------------------------------------------
def _pixart_true(m, HP):
    """adapter gradients in their true (un-padded) shapes; the pad lanes carry exactly zero"""
    H, hd = PX.ARCH["num_attention_heads"], PX.ARCH["attention_head_dim"]
    out = {}
    for name, p in m.named_parameters():
        if ".lora_" not in name:
            continue
        which, g = name.split(".lora_")[1], p.grad.detach().float().cpu()
        if which.startswith("A") and g.shape[1] == H * HP:
            g3 = g.view(g.shape[0], H, HP)
            assert float(g3[:, :, hd:].abs().max()) == 0, name
            g = g3[:, :, :hd].reshape(g.shape[0], H * hd)
        if which.startswith("B") and g.shape[0] == H * HP:
            g3 = g.view(H, HP, g.shape[1])
            assert float(g3[:, hd:].abs().max()) == 0, name
            g = g3[:, :hd].reshape(H * hd, g.shape[1])
        out[name] = g
    return out


def test_pixart_trunk_adapter_device_gradients_slab_by_slab(monkeypatch):
    from simpletuner_amd.pixart.transformer import HP, PixArtTransformer2DModel
    ARCH = PX.ARCH
    lat, cond, enc, mask, t = PX._inputs()
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))

    def run(m, device):
        m.train()
        out = m(lat.to(device), encoder_hidden_states=enc.to(device), timestep=t.to(device), encoder_attention_mask=mask.to(device), return_dict=False)[0]
        ((out.chunk(2, dim=1)[0].float() - target.to(device)) ** 2).mean().backward()
        return out.detach().float().cpu(), _pixart_true(m, HP)

    dev = PixArtTransformer2DModel(device=DEV, **ARCH)
    dev.init_synthetic(5)
    dev.add_lora_adapter(rank=8, alpha=16.0, init_b_std=0.05)
    out_g, g_gpu = run(dev, DEV)
    torch.cuda.synchronize()
    EMU.install(monkeypatch)
    twin = PixArtTransformer2DModel(device="cpu", **ARCH)
    twin.add_lora_adapter(rank=8, alpha=16.0, init_b_std=0.05)
    _copy_params(dev, twin)
    out_e, g_emu = run(twin, "cpu")
    P = {k: v.detach().to(F64) for k, v in twin.named_parameters() if ".lora_" not in k}
    lp = {k: tuple(x.detach().to(F64).requires_grad_(True) for x in ab) for k, ab in PX._true_lora(twin).items()}
    res, ar = torch.tensor([[16.0, 16.0]], dtype=F64).expand(2, -1), torch.tensor([[1.0]], dtype=F64).expand(2, -1)
    ref = pixart_forward(P, PixArtConfig(**ARCH), lat.to(F64), enc.to(F64), mask, t.to(F64), res, ar, lora=lp, lora_scale=16.0 / 8)
    ((ref.chunk(2, dim=1)[0] - target.to(F64)) ** 2).mean().backward()
    g64 = {n: lp[n.split(".lora_")[0]][0 if n.split(".lora_")[1].startswith("A") else 1].grad for n in g_emu}
    _finish("pixart trunk LoRA", g_gpu, g_emu, g64, ARCH["num_attention_heads"] * ARCH["attention_head_dim"], (out_g, out_e, ref.detach()))


def test_pixart_controlnet_branch_device_gradients_slab_by_slab(monkeypatch):
    from simpletuner_amd.pixart.transformer import PixArtSigmaControlNetTransformerModel, PixArtTransformer2DModel
    ARCH = PX.ARCH
    lat, cond, enc, mask, t = PX._inputs()
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))

    def run(cn, device):
        out = cn(lat.to(device), encoder_hidden_states=enc.to(device), timestep=t.to(device), controlnet_cond=cond.to(device), encoder_attention_mask=mask.to(device),
                 return_dict=False)[0]
        ((out.chunk(2, dim=1)[0].float() - target.to(device)) ** 2).mean().backward()
        g = {}
        for i, (blk, ex) in enumerate(cn.cblocks):
            g.update({f"controlnet_blocks.{i}.transformer_block.{k}": v for k, v in blk.G.items()})
            g.update({f"controlnet_blocks.{i}.{k}": v for k, v in ex.G.items()})
        return out.detach().float().cpu(), _cpu(g)

    m = PixArtTransformer2DModel(device=DEV, **ARCH)
    m.init_synthetic(5)
    cn = PixArtSigmaControlNetTransformerModel(m, num_layers=2)
    cn.init_adapter_synthetic(seed=9, std=0.05)
    with torch.no_grad():                           # de-correlate the copied blocks from the trunk so a swapped-weights bug cannot hide
        for blk, _ in cn.cblocks:
            for v in blk.P.values():
                v.add_(0.01 * torch.randn(v.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.bfloat16))
    out_g, g_gpu = run(cn, DEV)
    torch.cuda.synchronize()
    EMU.install(monkeypatch)
    mt = PixArtTransformer2DModel(device="cpu", **ARCH)
    _copy_params(m, mt)
    cnt = PixArtSigmaControlNetTransformerModel(mt, num_layers=2)
    with torch.no_grad():
        for (blk, ex), (blk_t, ex_t) in zip(cn.cblocks, cnt.cblocks):
            assert blk.P.keys() == blk_t.P.keys()
            for k, v in blk.P.items():
                blk_t.P[k].copy_(v)
            for k in vars(ex):
                if k.endswith("proj_weight") or k.endswith("proj_bias"):
                    getattr(ex_t, k).copy_(getattr(ex, k))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(cn.adapter_state_dict().values(), cnt.adapter_state_dict().values()))
    out_e, g_emu = run(cnt, "cpu")
    P = {k: v.detach().to(F64) for k, v in mt.named_parameters()}
    C = {k: v.detach().to(F64).clone().requires_grad_(True) for k, v in cnt.adapter_state_dict().items()}
    ref = controlnet_forward(P, C, PixArtConfig(**ARCH), 2, lat.to(F64), cond.to(F64), enc.to(F64), mask, t.to(F64), torch.tensor([[16.0, 16.0]], dtype=F64).expand(2, -1),
                             torch.tensor([[1.0]], dtype=F64).expand(2, -1))
    ((ref.chunk(2, dim=1)[0] - target.to(F64)) ** 2).mean().backward()
    g64 = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in C.items()}
    _finish("pixart ControlNet branch", g_gpu, g_emu, g64, ARCH["num_attention_heads"] * ARCH["attention_head_dim"], (out_g, out_e, ref.detach()))


# ------------------------------------------------------------------------------------------------
# UNet
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "lora"])
def test_unet_sdxl_small_device_gradients_slab_by_slab(monkeypatch, mode):
    from simpletuner_amd.unet.unet import UNet2DConditionModel as Cls
    rank, alpha = 16, 16.0
    sample, t, ehs, te, ti = UN._inputs(2, 16, 16, seed=1)
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9))

    def layout(s, x):
        if s.name.startswith("conv_in.weight"):
            return x[:, :72].reshape(-1, 9, 8)[:, :, :4]
        return x[:4] if s.name.startswith("conv_out") else x

    def arm(m):
        if mode == "full":
            m.enable_full_finetune()
        else:
            m.add_lora_adapter(rank=rank, alpha=alpha, seed=3, init_b_std=0.05)

    def run(m, device):
        out = m(sample.to(device), t.to(device), ehs.to(device), None, added_cond_kwargs={"text_embeds": te.to(device), "time_ids": ti.to(device)}, return_dict=False)[0]
        ((out.float() - target.to(device)) ** 2).mean().backward()
        g = {s.name: layout(s, s.g) for s in m._specs} if mode == "full" else {n: p.grad for n, p in m.named_parameters() if ".lora_" in n}
        return out.detach().float().cpu(), _cpu(g)

    dev = Cls(device=DEV, **UN.SMALL)
    dev.init_synthetic(5)
    arm(dev)
    out_g, g_gpu = run(dev, DEV)
    torch.cuda.synchronize()
    EMU.install(monkeypatch)
    twin = Cls(device="cpu", **UN.SMALL)
    with torch.no_grad():
        twin.arena.copy_(dev.arena)
    arm(twin)
    if mode == "lora":
        _copy_params(dev, twin)
        twin._refresh_transposed()
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dev.diffusers_state_dict().values(), twin.diffusers_state_dict().values()))
    out_e, g_emu = run(twin, "cpu")
    sd = twin.diffusers_state_dict()
    P = {k: v.detach().to(F64).clone().requires_grad_(mode == "full") for k, v in sd.items()}
    Pe, lora = dict(P), {}
    if mode == "lora":
        lora = {n: p.detach().to(F64).clone().requires_grad_(True) for n, p in twin.named_parameters() if ".lora_" in n}
        for n in lora:
            if ".lora_A." in n:
                base = n.replace(".lora_A.default.weight", "")
                Pe[base + ".weight"] = P[base + ".weight"] + (alpha / rank) * lora[base + ".lora_B.default.weight"] @ lora[n]
    ref = unet_forward(Pe, UNetConfig(**UN.SMALL), sample.to(F64), t.to(F64), ehs.to(F64), {"text_embeds": te.to(F64), "time_ids": ti.to(F64)})
    ((ref - target.to(F64)) ** 2).mean().backward()
    if mode == "full":
        # the fp64 reference through the same state-dict -> working-layout map the weights take (bf16 storage there): carried as three bf16-exact parts
        parts, rest = [], {k: v.grad.clone() for k, v in P.items()}
        for _ in range(4):
            hi = {k: v.to(torch.bfloat16) for k, v in rest.items()}
            g = Cls(device="cpu", **UN.SMALL)
            g.load_diffusers_state({k: v.clone() for k, v in hi.items()})
            parts.append({s.name: layout(s, s.t).to(F64) for s in g._specs})
            rest = {k: rest[k] - hi[k].to(F64) for k in rest}
        g64 = {k: sum(p[k] for p in parts) for k in parts[0]}
    else:
        g64 = {n: v.grad for n, v in lora.items()}
    _finish(f"unet sdxl_small {mode}", g_gpu, g_emu, g64, ALG._unet_width("sdxl_small"), (out_g, out_e, ref.detach()))


# ------------------------------------------------------------------------------------------------
# Features, one case each on SD3 LoRA: the fused feature kernels on the device, their stand-ins (tests/*_ref.py) on the twin
# ------------------------------------------------------------------------------------------------
FEATURES = ("dora", "lokr", "internal_guidance", "nextlat", "layersync")
IG_BLOCK = NL_BLOCK = 1
REG_WEIGHT, LS_PAIR, LS_LAMBDA = 8.0, (0, 1), 8.0


def _feature_model(feature, device):
    from simpletuner_amd.sd3 import transformer as T
    from tests import dora_ref as DR
    from tests import internal_guidance_ref as IG
    from tests import lokr_ref as LR
    from tests import nextlat_ref as NL
    kw = {"internal_guidance": dict(internal_guidance_block_index=IG_BLOCK), "nextlat": dict(nextlat_block_index=-1)}.get(feature, {})
    m = T.SD3Transformer2DModel(device=device, **kw, **S3._arch(3))
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith(IG.PREFIX) or name.startswith(NL.PREFIX):
                continue
            p.copy_(0.05 * torch.randn(p.shape, generator=g) if name.endswith(".bias") else torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = m.config
        m.pos_embed.pos_embed.copy_(T.sincos_2d(m.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])
    if feature == "lokr":
        m.add_lokr_adapter(factors={"Attention": 2, "FeedForward": 2})
        m.prepare_for_training()
    else:
        m.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02, **(dict(targets="all", dora=True) if feature == "dora" else {}))
    m.train()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():                 # move the feature's own parameters off their initial values, so that their gradients are gradients of something
        for n, p in m.named_parameters():
            if n.endswith(DR.KEY):
                p.mul_((1.0 + 0.2 * (torch.rand(p.shape, generator=g) - 0.5)).to(p.device))
            elif n.endswith(LR.K2):
                p.copy_((0.02 * torch.randn(p.shape, generator=g)).to(p.device))
    if feature == "internal_guidance":
        IG.seed_head(m)
    if feature == "nextlat":
        m.set_nextlat(NL_BLOCK, "smooth_l1")
        assert m._nl_block == NL_BLOCK
        NL.seed_predictor(m)
    if feature == "layersync":
        m.set_layersync(*LS_PAIR)
    return m


def _feature_run(feature, model, d):
    res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=True)
    tgt = d["target"].float()
    loss = ((res.sample.float() - tgt) ** 2).mean()
    if feature == "internal_guidance":
        loss = loss + REG_WEIGHT * ((res.internal_guidance_prediction.float() - tgt) ** 2).mean()
    if feature == "nextlat":
        loss = loss + REG_WEIGHT * res.nextlat_state_loss
    if feature == "layersync":
        loss = loss - LS_LAMBDA * res.layersync_similarity
    loss.backward()
    return res.sample.detach().float().cpu(), ALG._engine_grads(model)


@pytest.mark.parametrize("feature", FEATURES)
def test_sd3_feature_device_gradients_slab_by_slab(monkeypatch, feature):
    from tests import dora_ref as DR
    from tests import lokr_ref as LR
    dev = _feature_model(feature, DEV)
    d = S3._inputs(2, 16, 24, 33)
    out_g, g_gpu = _feature_run(feature, dev, _to_dev(d))
    torch.cuda.synchronize()
    g_gpu = _cpu(g_gpu)
    LR.install(monkeypatch)                # the emulator and every feature stand-in on top of it
    twin = _feature_model(feature, "cpu")
    _copy_params(dev, twin)
    out_e, g_emu = _feature_run(feature, twin, d)
    kw = {"dora": dict(linear=lambda P: DR.dora_linear({k[:-len(DR.KEY)]: v for k, v in P.items() if k.endswith(DR.KEY)})),
          # the merged weight rounded to bf16 on the oracle side, as the rule defines the bf16 forward (tests/test_lokr_cpu.py)
          "lokr": dict(linear=lambda P: LR.lokr_linear({k[:-len(LR.K1)]: (P[k], P[k[:-len(LR.K1)] + LR.K2]) for k in P if k.endswith(LR.K1)}, 1.0, round_bf16=True)),
          "internal_guidance": dict(ig=(IG_BLOCK, REG_WEIGHT)), "nextlat": dict(nl=(NL_BLOCK, REG_WEIGHT)), "layersync": dict(ls=LS_PAIR + (LS_LAMBDA,))}[feature]
    o64, _, g64 = ALG._sd3_feature_oracle(monkeypatch, twin, ALG._wide(d), F64, **kw)
    assert set(g64) == set(g_emu)
    _finish(f"sd3 LoRA + {feature}", g_gpu, g_emu, g64, twin.D, (out_g, out_e, o64))

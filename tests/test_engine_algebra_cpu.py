"""The engines' hand-written backward, held SLAB BY SLAB to autograd on the fp64 oracle — in wide arithmetic (tests/wide_arith.py: fp32 storage through the same
host sequencing), where the few-percent bf16 noise of the model-level parity tests is gone and the same algebra is checked four orders of magnitude tighter,
on every tensor, with nothing skipped.  Rule and constants: tests/engine_parity.py.  The bf16 host-sequencing tests (tests/test_*_host_sequencing_cpu.py) stay
as they are: they pin the emulator's bf16 sequencing, bit identity under recomputation and the launch stream; the case tables and shapes here are theirs."""
import pathlib

import pytest
import torch

from oracle import flux as OF
from oracle import sd3 as OS
from oracle.pixart import PixArtConfig, controlnet_forward, pixart_forward
from oracle.unet import UNetConfig, unet_forward
from tests import engine_parity as EP
from tests import ops_emulator as EMU
from tests import parity_utils as PU
from tests import test_flux_host_sequencing_cpu as FX
from tests import test_pixart_host_sequencing_cpu as PX
from tests import test_sd3_host_sequencing_cpu as S3
from tests import test_unet_host_sequencing_cpu as UN
from tests import wide_arith as W

F32, F64 = torch.float32, torch.float64


def test_every_module_that_binds_the_storage_constant_is_listed():
    """a module under simpletuner_amd/ or a tests/*_ref.py that binds BF16 and is not in tests/wide_arith.py would keep bf16 storage in wide mode, silently"""
    found = W.modules_binding_the_constant(pathlib.Path(__file__).resolve().parent.parent)
    assert sorted(found) == sorted(W.MODULES), sorted(set(found) ^ set(W.MODULES))
    assert W._binds("from x import F32, BF16") and W._binds("F32, BF16 = a, b") and W._binds("BF16: object = a") and not W._binds("x = BF16") and not W._binds("    BF16 = a")


def test_wide_mode_rebinds_the_constant_and_monkeypatch_restores_it():
    from simpletuner_amd import engine
    mp = pytest.MonkeyPatch()
    W.install(mp)
    try:
        assert engine.BF16 is F32 and EMU.BF16 is F32
    finally:
        mp.undo()
    assert engine.BF16 is torch.bfloat16 and EMU.BF16 is torch.bfloat16


def _wide(d):
    """the bf16-representable inputs of the bf16 case tables, stored wide"""
    return {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.bfloat16 else v) for k, v in d.items()}


def _to(v, dt):
    return v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v


def _param_refs(model, P, lp):
    """{engine parameter name: oracle gradient}: base parameters by name, adapter factors through their module key"""
    ref = {}
    for name, p in model.named_parameters():
        if ".lora_" in name:
            key, which = name.split(".lora_")
            ref[name] = lp[key][0 if which.startswith("A") else 1].grad
        elif p.requires_grad:
            ref[name] = P[name].grad
    return {k: (torch.zeros_like(dict(model.named_parameters())[k], dtype=F64) if v is None else v) for k, v in ref.items()}


def _engine_grads(model):
    return {n: p.grad for n, p in model.named_parameters() if p.requires_grad}


def _tread_record(B, Si, seed, per_sample_seed=False):
    if per_sample_seed:
        perm = torch.stack([torch.randperm(Si, generator=torch.Generator().manual_seed(seed + b)) for b in range(B)])
    else:
        g = torch.Generator().manual_seed(seed)
        perm = torch.stack([torch.randperm(Si, generator=g) for _ in range(B)])
    K = Si - int(round(Si * 0.5))
    return {"mask": torch.ones(B, Si, dtype=torch.bool).scatter_(1, perm[:, :K], False), "ids_keep": perm[:, :K], "ids_mask": perm[:, K:], "ids_shuffle": perm,
            "ids_restore": torch.argsort(perm, dim=1)}


# ------------------------------------------------------------------------------------------------
# Flux
# ------------------------------------------------------------------------------------------------
def _flux_engine(model, d, mask=None):
    out = model(hidden_states=d["packed"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], img_ids=d["img_ids"], txt_ids=d["txt_ids"],
                guidance=d["guidance"] if model.config.guidance_embeds else None, attention_mask=mask, return_dict=False)[0]
    assert out.dtype == F32                                    # wide storage reached the prediction
    loss = ((out.float() - d["target"].float()) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), _engine_grads(model)


def _flux_oracle(model, d, dt, key_bias=None, tread=None):
    P, lora, scale = PU.oracle_state(model, dtype=dt)
    if model.full:
        P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()} or None
    f = lambda k: d[k].to(dt)
    out = OF.flux_forward(P, PU.oracle_cfg(model), f("packed"), f("prompt"), f("pooled"), f("t"), f("img_ids"), f("txt_ids"),
                          f("guidance") if model.config.guidance_embeds else None, lp, scale, key_bias=_to(key_bias, dt), tread=tread)
    assert out.dtype == dt
    loss = ((out - f("target")) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), _param_refs(model, P, lp)


def _flux_check(case, model, d, mask=None, key_bias=None, tread=None):
    out, loss, eng = _flux_engine(model, d, mask)
    o64, l64, g64 = _flux_oracle(model, d, F64, key_bias, tread)
    o32, l32, g32 = _flux_oracle(model, d, F32, key_bias, tread)
    rep = EP.check_wide(case, eng, g64, g32, model.D, {"prediction": (out, o64, o32), "loss": (loss, l64, l32)}).record().assert_ok()
    return rep, eng, g64, g32


def _flux_model(monkeypatch, layers, single, guidance=True):
    W.install(monkeypatch)
    return FX._model(monkeypatch, layers, single, guidance=guidance)


@pytest.mark.parametrize("which,layers,single,B,lat_h,lat_w,S_txt,rank", [
    ("all", 2, 2, 1, 16, 16, 64, 16), ("all", 2, 2, 2, 16, 8, 24, 16),
    ("all+ffs+embedder", 2, 2, 2, 16, 8, 24, 16), ("ai-toolkit", 2, 2, 2, 16, 8, 24, 16), ("all+ffs", 2, 2, 1, 8, 8, 40, 80), ("nano", 1, 9, 2, 8, 8, 24, 16),
    ("all+ffs+embedder", 0, 2, 2, 16, 8, 24, 16)])
def test_flux_adapter_gradients_slab_by_slab(monkeypatch, which, layers, single, B, lat_h, lat_w, S_txt, rank):
    """LoRA targets "all"; the widest sets (feed-forward, embedder, modulation: "ai-toolkit", single-layer: "nano"); rank 80 (64-column slabs in rank space); a model
    without double blocks"""
    model = _flux_model(monkeypatch, layers, single)
    model.add_lora_adapter(rank=rank, alpha=float(rank), targets=which, init_b_std=0.02)
    rep, *_ = _flux_check(f"flux LoRA {which} r{rank} L{layers}+{single} B{B}", model, _wide(FX._inputs(B, lat_h, lat_w, S_txt)))
    assert len(rep.rows) >= 2 * len(OF.lora_targets(PU.oracle_cfg(model), which)) + 2          # every factor; B factors of the [4D, r] feed-forward projections split


@pytest.mark.parametrize("B,lat_h,lat_w,S_txt,guidance", [(1, 16, 16, 64, True), (2, 16, 8, 24, True), (2, 8, 8, 40, False)])
def test_flux_full_rank_gradients_slab_by_slab(monkeypatch, B, lat_h, lat_w, S_txt, guidance):
    model = _flux_model(monkeypatch, 2, 2, guidance=guidance)
    model.enable_full_finetune()
    if B == 2 and guidance:
        model._tn_window_bytes = 2 * model.D * 1024            # the modulation matrix's input gradient in 8 row blocks, as in the bf16 table
    rep, *_ = _flux_check(f"flux full-rank B{B} guidance={guidance}", model, _wide(FX._inputs(B, lat_h, lat_w, S_txt)))
    assert len(rep.rows) > len(list(model.named_parameters())) + 2          # the [6D, D] / [3D, D] modulation matrices and fused projections really were split


@pytest.mark.parametrize("layers,single,B,lat_h,lat_w,S_txt", [(2, 2, 1, 16, 16, 64), (0, 2, 1, 16, 8, 24), (2, 2, 2, 16, 8, 24)])
def test_flux_tokenwise_timesteps_slab_by_slab(monkeypatch, layers, single, B, lat_h, lat_w, S_txt):
    model = _flux_model(monkeypatch, layers, single)
    model.add_lora_adapter(rank=16, alpha=16.0, targets="all", init_b_std=0.02)
    d = _wide(FX._inputs(B, lat_h, lat_w, S_txt))
    d["t"] = torch.rand(B, (lat_h // 2) * (lat_w // 2), generator=torch.Generator().manual_seed(8)) * 0.9 + 0.05
    _flux_check(f"flux tokenwise L{layers}+{single} B{B}", model, d)


def test_flux_masked_attention_training_slab_by_slab(monkeypatch):
    model = _flux_model(monkeypatch, 1, 2)
    model.add_lora_adapter(rank=8, alpha=8.0, targets="default", init_b_std=0.02)
    d = _wide(FX._inputs(2, 16, 16, 32))
    St, Si = 32, 64
    mask = torch.ones(2, St); mask[0, 20:] = 0; mask[1, 9:] = 0
    kb = torch.ones(2, St + Si); kb[:, :St] = (mask > 0).float()
    _flux_check("flux masked attention", model, d, mask=mask, key_bias=kb)


@pytest.mark.parametrize("masked", [False, True])
def test_flux_fused_projection_path_slab_by_slab(monkeypatch, masked):
    """Flux's default host path (fused QKV epilogue, attention backward with the RoPE / RMSNorm epilogues), as tests/test_flux_host_sequencing_cpu.py enables it"""
    from simpletuner_amd import ops
    from simpletuner_amd.flux import transformer as T
    model = _flux_model(monkeypatch, 2, 1)
    monkeypatch.setattr(T, "_FUSED_QKV", True)
    model.add_lora_adapter(rank=16, alpha=16.0, targets="default", init_b_std=0.02)
    calls, orig = [], EMU.attn_bwd_rope
    monkeypatch.setattr(ops, "attn_bwd_rope", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    d = _wide(FX._inputs(2, 32, 32, 256))
    mask = kb = None
    if masked:
        mask = torch.ones(2, 256); mask[0, 160:] = 0; mask[1, 72:] = 0
        kb = torch.ones(2, 512); kb[:, :256] = (mask > 0).float()
    _flux_check(f"flux fused projection masked={masked}", model, d, mask=mask, key_bias=kb)
    assert len(calls) == 3                                     # every block's backward went through the fused attention + RoPE / RMSNorm backward


@pytest.mark.parametrize("which,start,end", [("default", 1, -2), ("default", 3, 5), ("all+ffs", 1, 3)])
def test_flux_tread_routes_under_recomputation_slab_by_slab(monkeypatch, which, start, end):
    """TREAD x {none, per-block, segmented} recomputation: each against the oracle replaying the permutation, and the recomputed gradients equal to the kept-activation
    ones to the same allowance (bit identity stays with the bf16 tests)"""
    from simpletuner_amd.training.tread import ReplayRouter
    d = _wide(FX._inputs(2, 16, 16, 32))
    rec = _tread_record(2, 64, 17)
    routes = [{"selection_ratio": 0.5, "start_layer_idx": start, "end_layer_idx": end}]
    kept = None
    for plan in ("none", "per-block", "segmented"):
        model = _flux_model(monkeypatch, 3, 4)
        model.add_lora_adapter(rank=8, alpha=8.0, targets=which, init_b_std=0.02)
        model.set_router(ReplayRouter([rec]), routes)
        model.train()
        if plan != "none":
            model.enable_gradient_checkpointing()
            if plan == "segmented":
                model.set_gradient_checkpointing_interval(2)
        case = f"flux TREAD [{start},{end}] {which} recompute={plan}"
        _, eng, g64, g32 = _flux_check(case, model, d, tread={"routes": routes, "mask_infos": [rec]})
        if kept is None:
            kept = eng
        else:
            EP.check_equal_wide(case + " vs kept", eng, kept, g64, g32, model.D).assert_ok()


def test_flux_full_rank_recomputation_slab_by_slab(monkeypatch):
    d = _wide(FX._inputs(2, 16, 8, 24))
    kept = None
    for ckpt in (False, True):
        model = _flux_model(monkeypatch, 2, 3)
        model.enable_full_finetune()
        if ckpt:
            model.enable_gradient_checkpointing()
            model.set_gradient_checkpointing_interval(2)
        _, eng, g64, g32 = _flux_check(f"flux full-rank recompute={ckpt}", model, d)
        if kept is None:
            kept = eng
        else:
            EP.check_equal_wide("flux full-rank recomputed vs kept", eng, kept, g64, g32, model.D).assert_ok()


# ------------------------------------------------------------------------------------------------
# SD3 / SD3.5
# ------------------------------------------------------------------------------------------------
def _sd3_model(monkeypatch, layers, sd35=False):
    W.install(monkeypatch)
    return S3._model(monkeypatch, layers, sd35)


def _sd3_engine(model, d):
    out = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)[0]
    assert out.dtype == F32
    loss = ((out.float() - d["target"].float()) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), _engine_grads(model)


def _sd3_oracle(model, d, dt, tread=None):
    P, lora, scale = PU.oracle_state(model, dtype=dt)
    if model.full:
        P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().to(dt)
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()} or None
    out = OS.sd3_forward(P, S3._ocfg(model), d["lat"].to(dt), d["prompt"].to(dt), d["pooled"].to(dt), d["t"].to(dt), lora=lp, lora_scale=scale, tread=tread)
    assert out.dtype == dt
    loss = ((out - d["target"].to(dt)) ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach(), _param_refs(model, P, lp)


def _sd3_check(case, model, d, tread=None):
    out, loss, eng = _sd3_engine(model, d)
    o64, l64, g64 = _sd3_oracle(model, d, F64, tread)
    o32, l32, g32 = _sd3_oracle(model, d, F32, tread)
    rep = EP.check_wide(case, eng, g64, g32, model.D, {"prediction": (out, o64, o32), "loss": (loss, l64, l32)}).record().assert_ok()
    return rep, eng, g64, g32


@pytest.mark.parametrize("sd35,rank", [(False, 16), (True, 16), (False, 80)])
def test_sd3_adapter_gradients_slab_by_slab(monkeypatch, sd35, rank):
    model = _sd3_model(monkeypatch, 3, sd35)
    model.add_lora_adapter(rank=rank, alpha=float(rank), init_b_std=0.02)
    _sd3_check(f"sd3{'.5' if sd35 else ''} LoRA r{rank}", model, _wide(S3._inputs(2, 16, 24, 33)))


@pytest.mark.parametrize("layers,B,lat_h,lat_w,S_txt,sd35", [(2, 1, 16, 16, 40, False), (3, 2, 16, 24, 33, False), (3, 2, 16, 24, 33, True)])
def test_sd3_full_finetune_gradients_slab_by_slab(monkeypatch, layers, B, lat_h, lat_w, S_txt, sd35):
    """every parameter, the ones under the bf16 tests' "small stays small" rule included; SD3.5: dual attention + q/k RMSNorm weights"""
    model = _sd3_model(monkeypatch, layers, sd35)
    model.enable_full_finetune()
    rep, *_ = _sd3_check(f"sd3{'.5' if sd35 else ''} full fine-tune L{layers} B{B}", model, _wide(S3._inputs(B, lat_h, lat_w, S_txt)))
    assert len(rep.rows) > len(list(model.named_parameters())) + 2


def test_sd3_scale_entry_of_exactly_minus_one_slab_by_slab(monkeypatch):
    model = _sd3_model(monkeypatch, 2)
    model.enable_full_finetune()
    with torch.no_grad():
        blk, D = model.blocks[0], model.D
        model.mod_w[blk.mod_off + D + 5].zero_()
        model.mod_b[blk.mod_off + D + 5] = -1.0
    _sd3_check("sd3 scale == -1", model, _wide(S3._inputs(2, 16, 16, 24)))


@pytest.mark.parametrize("B,lat_h,lat_w", [(1, 16, 24), (2, 16, 24)])
def test_sd3_tokenwise_timesteps_slab_by_slab(monkeypatch, B, lat_h, lat_w):
    model = _sd3_model(monkeypatch, 3)
    model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    d = _wide(S3._inputs(B, lat_h, lat_w, 33))
    d["t"] = torch.rand(B, (lat_h // 2) * (lat_w // 2), generator=torch.Generator().manual_seed(8)) * 900.0 + 50.0
    _sd3_check(f"sd3 tokenwise B{B}", model, d)


@pytest.mark.parametrize("full", [False, True])
def test_sd3_tread_and_checkpoint_plans_slab_by_slab(monkeypatch, full):
    """TREAD x checkpoint plans: the routed run and the routed + per-block-recomputed run against the oracle replaying the permutation; the plain run and the segmented
    plan (interval 2 / stride 3) against the plain oracle; recomputed gradients equal to the kept ones to the same allowance"""
    from simpletuner_amd.training.tread import ReplayRouter
    d = _wide(S3._inputs(2, 16, 16, 24))
    rec = _tread_record(2, 64, 11)
    routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]

    def run(route, ckpt, interval=None, stride=None):
        model = _sd3_model(monkeypatch, 4)
        if full:
            model.enable_full_finetune()
        else:
            model.add_lora_adapter(rank=8, alpha=8.0, init_b_std=0.02)
        if route:
            model.set_router(ReplayRouter([rec]), routes)
        model.train()
        if ckpt:
            model.gradient_checkpointing = True
            model.gradient_checkpointing_interval, model.gradient_checkpointing_segment_stride = interval, stride
        case = f"sd3 {'full' if full else 'LoRA'} route={route} recompute={(interval, stride) if ckpt else None}"
        _, eng, g64, g32 = _sd3_check(case, model, d, tread={"routes": routes, "mask_infos": [rec]} if route else None)
        return model, eng, g64, g32

    _, kept, *_ = run(True, False)
    model, eng, g64, g32 = run(True, True)
    EP.check_equal_wide("sd3 routed, recomputed vs kept", eng, kept, g64, g32, model.D).assert_ok()
    _, kept, *_ = run(False, False)
    model, eng, g64, g32 = run(False, True, 2, 3)
    EP.check_equal_wide("sd3 segmented plan vs kept", eng, kept, g64, g32, model.D).assert_ok()


# ------------------------------------------------------------------------------------------------
# PixArt
# ------------------------------------------------------------------------------------------------
def _pixart_inputs():
    lat, cond, enc, mask, t = PX._inputs()
    return lat.float(), cond.float(), enc.float(), mask, t


@pytest.mark.parametrize("route", [False, True])
def test_pixart_trunk_adapter_gradients_slab_by_slab(monkeypatch, route):
    """trunk LoRA on both routes (plain, TREAD around blocks [1, -2]); adapters compared in their true (un-padded) shapes, the pad lanes exactly zero"""
    W.install(monkeypatch)
    from simpletuner_amd.pixart.transformer import HP, PixArtTransformer2DModel
    from simpletuner_amd.training.tread import ReplayRouter
    ARCH = PX.ARCH
    m = PixArtTransformer2DModel(device="cpu", **ARCH)
    m.init_synthetic(5)
    m.add_lora_adapter(rank=8, alpha=16.0, init_b_std=0.05)
    lat, cond, enc, mask, t = _pixart_inputs()
    B, S = lat.shape[0], (lat.shape[2] // 2) * (lat.shape[3] // 2)
    routes, rec = [], None
    if route:
        rec = _tread_record(B, S, 11)
        routes = [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": -2}]
        m.set_router(ReplayRouter([rec]), routes)
    m.train()
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))
    out = m(lat, encoder_hidden_states=enc, timestep=t, encoder_attention_mask=mask, return_dict=False)[0]
    assert out.dtype == F32
    loss = ((out.chunk(2, dim=1)[0].float() - target) ** 2).mean()
    loss.backward()
    H, hd = ARCH["num_attention_heads"], ARCH["attention_head_dim"]
    eng = {}
    for name, p in m.named_parameters():
        if ".lora_" not in name:
            continue
        which, g = name.split(".lora_")[1], p.grad
        if which.startswith("A") and g.shape[1] == H * HP:
            g3 = g.view(g.shape[0], H, HP)
            assert float(g3[:, :, hd:].abs().max()) == 0
            g = g3[:, :, :hd].reshape(g.shape[0], H * hd)
        if which.startswith("B") and g.shape[0] == H * HP:
            g3 = g.view(H, HP, g.shape[1])
            assert float(g3[:, hd:].abs().max()) == 0
            g = g3[:, :hd].reshape(H * hd, g.shape[1])
        eng[name] = g

    def oracle(dt):
        P = {k: v.detach().to(dt) for k, v in m.named_parameters() if ".lora_" not in k}
        lp = {k: tuple(x.detach().to(dt).requires_grad_(True) for x in ab) for k, ab in PX._true_lora(m).items()}
        res, ar = torch.tensor([[16.0, 16.0]], dtype=dt).expand(2, -1), torch.tensor([[1.0]], dtype=dt).expand(2, -1)
        ref = pixart_forward(P, PixArtConfig(**ARCH), lat.to(dt), enc.to(dt), mask, t.to(dt), res, ar, lora=lp, lora_scale=16.0 / 8,
                             tread={"routes": routes, "mask_infos": [rec]} if route else None)
        assert ref.dtype == dt
        lref = ((ref.chunk(2, dim=1)[0] - target.to(dt)) ** 2).mean()
        lref.backward()
        return ref.detach(), lref.detach(), {n: lp[n.split(".lora_")[0]][0 if n.split(".lora_")[1].startswith("A") else 1].grad for n in eng}

    o64, l64, g64 = oracle(F64)
    o32, l32, g32 = oracle(F32)
    EP.check_wide(f"pixart trunk LoRA route={route}", eng, g64, g32, H * hd, {"prediction": (out.detach(), o64, o32), "loss": (loss.detach(), l64, l32)}).record().assert_ok()


def test_pixart_controlnet_branch_gradients_slab_by_slab(monkeypatch):
    """every tensor of the trained branch — to_k.bias included, whose true gradient is zero (softmax-invariant) and which the bf16 test leaves out: the floors hold it"""
    W.install(monkeypatch)
    from simpletuner_amd.pixart.transformer import PixArtSigmaControlNetTransformerModel, PixArtTransformer2DModel
    ARCH = PX.ARCH
    m = PixArtTransformer2DModel(device="cpu", **ARCH)
    m.init_synthetic(5)
    cn = PixArtSigmaControlNetTransformerModel(m, num_layers=2)
    cn.init_adapter_synthetic(seed=9, std=0.05)
    with torch.no_grad():
        for blk, _ in cn.cblocks:
            for v in blk.P.values():
                v.add_(0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).float())
    lat, cond, enc, mask, t = _pixart_inputs()
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))
    out = cn(lat, encoder_hidden_states=enc, timestep=t, controlnet_cond=cond, encoder_attention_mask=mask, return_dict=False)[0]
    assert out.dtype == F32
    loss = ((out.chunk(2, dim=1)[0].float() - target) ** 2).mean()
    loss.backward()
    eng = {}
    for i, (blk, ex) in enumerate(cn.cblocks):
        eng.update({f"controlnet_blocks.{i}.transformer_block.{k}": g for k, g in blk.G.items()})
        eng.update({f"controlnet_blocks.{i}.{k}": g for k, g in ex.G.items()})

    def oracle(dt):
        P = {k: v.detach().to(dt) for k, v in m.named_parameters()}
        C = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in cn.adapter_state_dict().items()}
        ref = controlnet_forward(P, C, PixArtConfig(**ARCH), 2, lat.to(dt), cond.to(dt), enc.to(dt), mask, t.to(dt), torch.tensor([[16.0, 16.0]], dtype=dt).expand(2, -1),
                                 torch.tensor([[1.0]], dtype=dt).expand(2, -1))
        assert ref.dtype == dt
        lref = ((ref.chunk(2, dim=1)[0] - target.to(dt)) ** 2).mean()
        lref.backward()
        return ref.detach(), lref.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in C.items()}

    o64, l64, g64 = oracle(F64)
    o32, l32, g32 = oracle(F32)
    assert set(eng) == set(g64)
    D = ARCH["num_attention_heads"] * ARCH["attention_head_dim"]
    EP.check_wide("pixart ControlNet branch", eng, g64, g32, D, {"prediction": (out.detach(), o64, o32), "loss": (loss.detach(), l64, l32)}).record().assert_ok()


# ------------------------------------------------------------------------------------------------
# UNet
# ------------------------------------------------------------------------------------------------
def _unet_width(arch):
    widths = sorted(set(UN.ARCHS[arch]["block_out_channels"]), reverse=True)

    def width(name, t):
        """the channel width of the stream a tensor sits in: the largest block width that divides its leading dimension"""
        return next((w for w in widths if t.dim() and t.shape[0] % w == 0), 0)
    return width


def _unet_inputs(B, H, W_, seed):
    sample, t, ehs, te, ti = UN._inputs(B, H, W_, seed=seed)
    return sample.float(), t, ehs.float(), te.float(), ti.float()


@pytest.mark.parametrize("arch", list(UN.ARCHS))
def test_unet_full_finetune_gradients_slab_by_slab(monkeypatch, arch):
    W.install(monkeypatch)
    from simpletuner_amd.unet.unet import UNet2DConditionModel as Cls
    m = Cls(device="cpu", **UN.ARCHS[arch])
    m.init_synthetic(5)
    m.enable_full_finetune()
    sample, t, ehs, te, ti = _unet_inputs(2, 16, 16, 1)
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9))
    ack = {"text_embeds": te, "time_ids": ti} if arch == "sdxl_small" else None
    out = m(sample, t, ehs, None, added_cond_kwargs=ack, return_dict=False)[0]
    assert out.dtype == F32
    loss = ((out.float() - target) ** 2).mean()
    loss.backward()

    def layout(s, x):
        """the engine's working layout carries pad channels on conv_in / conv_out: compare what the reference model owns"""
        if s.name.startswith("conv_in.weight"):
            return x[:, :72].reshape(-1, 9, 8)[:, :, :4]
        return x[:4] if s.name.startswith("conv_out") else x

    eng = {s.name: layout(s, s.g) for s in m._specs}
    sd = m.diffusers_state_dict()

    def oracle(dt):
        P = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
        ref = unet_forward(P, UNetConfig(**UN.ARCHS[arch]), sample.to(dt), t.to(dt), ehs.to(dt), {"text_embeds": te.to(dt), "time_ids": ti.to(dt)})
        assert ref.dtype == dt
        lref = ((ref - target.to(dt)) ** 2).mean()
        lref.backward()
        return ref.detach(), lref.detach(), {k: v.grad for k, v in P.items()}

    o64, l64, G64 = oracle(F64)
    o32, l32, G32 = oracle(F32)

    def working(G, dt):
        """the reference gradients through the same state-dict -> working-layout map the weights take"""
        g = Cls(device="cpu", **UN.ARCHS[arch])
        g.load_diffusers_state({k: v.to(F32) for k, v in G.items()})
        return {s.name: layout(s, s.t) for s in g._specs}

    # the state-dict -> working-layout map stores fp32 in wide mode: carry the fp64 reference through it as (fp32 head) + (fp32 remainder)
    hi = {k: v.to(F32) for k, v in G64.items()}
    lo = {k: (v - hi[k].to(F64)).to(F32) for k, v in G64.items()}
    w_hi, w_lo = working(hi, F32), working(lo, F32)
    g64 = {k: w_hi[k].to(F64) + w_lo[k].to(F64) for k in w_hi}
    g32 = working(G32, F32)
    EP.check_wide(f"unet {arch} full fine-tune", eng, g64, g32, _unet_width(arch), {"prediction": (out.detach(), o64, o32), "loss": (loss.detach(), l64, l32)}).record().assert_ok()


def test_unet_adapter_gradients_slab_by_slab(monkeypatch):
    rank, alpha = 16, 16.0
    W.install(monkeypatch)
    from simpletuner_amd.unet.unet import UNet2DConditionModel as Cls
    m = Cls(device="cpu", **UN.SMALL)
    m.init_synthetic(6)
    m.add_lora_adapter(rank=rank, alpha=alpha, seed=3, init_b_std=0.05)
    sample, t, ehs, te, ti = _unet_inputs(2, 16, 16, 2)
    target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(8))
    out = m(sample, t, ehs, None, added_cond_kwargs={"text_embeds": te, "time_ids": ti}, return_dict=False)[0]
    assert out.dtype == F32
    loss = ((out.float() - target) ** 2).mean()
    loss.backward()
    eng = {n: p.grad for n, p in m.named_parameters() if ".lora_" in n}
    sd = m.diffusers_state_dict()

    def oracle(dt):
        P = {k: v.detach().to(dt) for k, v in sd.items()}
        lora = {n: p.detach().to(dt).clone().requires_grad_(True) for n, p in m.named_parameters() if ".lora_" in n}
        Pe = dict(P)
        for n in lora:
            if ".lora_A." in n:
                base = n.replace(".lora_A.default.weight", "")
                Pe[base + ".weight"] = P[base + ".weight"] + (alpha / rank) * lora[base + ".lora_B.default.weight"] @ lora[n]
        ref = unet_forward(Pe, UNetConfig(**UN.SMALL), sample.to(dt), t.to(dt), ehs.to(dt), {"text_embeds": te.to(dt), "time_ids": ti.to(dt)})
        assert ref.dtype == dt
        lref = ((ref - target.to(dt)) ** 2).mean()
        lref.backward()
        return ref.detach(), lref.detach(), {n: v.grad for n, v in lora.items()}

    o64, l64, g64 = oracle(F64)
    o32, l32, g32 = oracle(F32)
    EP.check_wide("unet sdxl_small LoRA", eng, g64, g32, _unet_width("sdxl_small"), {"prediction": (out.detach(), o64, o32), "loss": (loss.detach(), l64, l32)}).record().assert_ok()


# ------------------------------------------------------------------------------------------------
# Features (engine.py and the adapter sites), on SD3 — LayerSync on Flux too.  The engines come from the features' own bf16 tests; the oracle side is one function:
# autograd through oracle.sd3 with the feature's rule on top (a `linear` that restates the adapter, a regulariser on the recorded block outputs), in the dtype asked for.
# ------------------------------------------------------------------------------------------------
def _sd3_feature_oracle(monkeypatch, model, d, dt, linear=None, ig=None, nl=None, ls=None, tread=None):
    """linear: f(P) -> replacement of oracle.sd3.linear; ig = (block, weight); nl = (block, weight); ls = (student, teacher, lambda).
    Returns (prediction, total loss, {engine parameter name: gradient} for every trainable parameter)."""
    import torch.nn.functional as F

    from tests import internal_guidance_ref as IG
    from tests import layersync_ref as LS
    from tests import nextlat_ref as NL
    with monkeypatch.context() as m:
        outs = LS.record_sd3_blocks(m)
        leaves, P, A, Bm = {}, {}, {}, {}
        for k, v in model.named_parameters():
            t = v.detach().to(dt).clone()
            if v.requires_grad:
                leaves[k] = t.requires_grad_(True)
            if ".lora_A." in k:
                A[k.split(".lora_A.")[0]] = t
            elif ".lora_B." in k:
                Bm[k.split(".lora_B.")[0]] = t
            else:
                P[k] = t
        P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().to(dt)
        lp = {k: (A[k], Bm[k]) for k in A} or None
        scale = model.lora_groups[0].scale if model.lora_groups else 1.0
        if linear is not None:
            m.setattr(OS, "linear", linear(P))
        kw = {} if tread is None else dict(tread=tread)
        out = OS.sd3_forward(P, S3._ocfg(model), d["lat"].to(dt), d["prompt"].to(dt), d["pooled"].to(dt), d["t"].to(dt), lora=lp, lora_scale=scale, **kw)
        assert out.dtype == dt
        tgt = d["target"].to(dt)
        total = ((out - tgt) ** 2).mean()
        if ig is not None:
            igp = IG.head_autograd(outs[ig[0]], *(P[IG.PREFIX + nm] for nm in IG.NAMES), tgt.shape[1], tgt.shape[2], tgt.shape[3])
            total = total + ig[1] * ((igp - tgt) ** 2).mean()
        if nl is not None:               # nextlat_ref.state_autograd without its casts to fp32
            h = outs[nl[0]]
            ga, be, Wu, bu, Wd, bd = (P[NL.PREFIX + nm] for nm in NL.NAMES)
            pred = F.linear(F.gelu(F.linear(F.layer_norm(h[:, :-1], (h.shape[-1],), ga, be, NL.EPS), Wu, bu)), Wd, bd)
            total = total + nl[1] * F.smooth_l1_loss(pred, h[:, 1:].detach(), reduction="mean")
        if ls is not None:
            total = total - ls[2] * LS.autograd_similarity(outs[ls[0]], outs[ls[1]])
        total.backward()
    return out.detach(), total.detach(), {k: (torch.zeros_like(t) if t.grad is None else t.grad) for k, t in leaves.items()}


def _sd3_feature_check(case, monkeypatch, model, d, engine, **oracle_kw):
    out, loss = engine(model, d)
    eng = _engine_grads(model)
    o64, l64, g64 = _sd3_feature_oracle(monkeypatch, model, d, F64, **oracle_kw)
    o32, l32, g32 = _sd3_feature_oracle(monkeypatch, model, d, F32, **oracle_kw)
    rep = EP.check_wide(case, eng, g64, g32, model.D, {"prediction": (out, o64, o32), "loss": (loss, l64, l32)}).record().assert_ok()
    return rep, eng, g64, g32


def _plain_engine(model, d):
    out, loss, _ = _sd3_engine(model, d)
    return out, loss


@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_dora_gradients_slab_by_slab(monkeypatch, sd35):
    from tests import dora_ref as DR
    from tests import test_dora_cpu as TD
    W.install(monkeypatch)
    model = TD._model(monkeypatch, 3, sd35, targets="all")
    TD._perturb(model)
    hook = lambda P: DR.dora_linear({k[:-len(DR.KEY)]: v for k, v in P.items() if k.endswith(DR.KEY)})
    rep, *_ = _sd3_feature_check(f"sd3{'.5' if sd35 else ''} DoRA", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)), _plain_engine, linear=hook)
    assert any(EP.family(r.name) == "DoRA magnitude" and r.ref > 0 for r in rep.rows)


@pytest.mark.parametrize("ckpt", ["plain", "stride"])
@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_lokr_gradients_slab_by_slab(monkeypatch, sd35, ckpt):
    """the merged weight is NOT rounded on the oracle side here (the bf16 test rounds it to bf16, as the rule defines the bf16 forward): in wide arithmetic the fold's
    one fp32 rounding is within the allowance"""
    from tests import lokr_ref as LR
    from tests import test_lokr_cpu as TL
    W.install(monkeypatch)
    model = TL._model(monkeypatch, 4, sd35)
    TL._perturb(model)
    TL._plan(model, ckpt)
    hook = lambda P: LR.lokr_linear({k[:-len(LR.K1)]: (P[k], P[k[:-len(LR.K1)] + LR.K2]) for k in P if k.endswith(LR.K1)}, 1.0, round_bf16=False)
    rep, *_ = _sd3_feature_check(f"sd3{'.5' if sd35 else ''} LoKr {ckpt}", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)), _plain_engine, linear=hook)
    assert sum(EP.family(r.name) == "LoKr factor" and r.ref > 0 for r in rep.rows) > 20


@pytest.mark.parametrize("sd35", [False, True], ids=["plain-block", "dual-attention"])
def test_sd3_lora_dropout_gradients_slab_by_slab(monkeypatch, sd35):
    """p = 0.25 > 0; the mask is counter-based (seed, rank, call, stream, element), so the oracle's masked linear draws the identical mask"""
    from tests import lora_dropout_ref as LD
    from tests import test_lora_dropout_cpu as TD
    W.install(monkeypatch)
    model = TD._model(monkeypatch, 3, sd35, calls=4)
    d = _wide(S3._inputs(2, 16, 24, 33))

    def engine(model, d):
        out, loss = _plain_engine(model, d)
        assert model.lora_dropout.calls() == 5
        return out, loss

    hook = lambda P: LD.masked_linear(LD.stream_ids(model), LD.key_of(TD.SEED, TD.RANK), 5, model.lora_dropout.thr)
    _, eng, g64, _ = _sd3_feature_check(f"sd3{'.5' if sd35 else ''} LoRA dropout p={TD.P_DROP}", monkeypatch, model, d, engine, linear=hook)
    # ... and the mask is live: the same oracle without it is far from the engine
    _, _, plain = _sd3_feature_oracle(monkeypatch, model, d, F64)
    assert max(PU.rel_l2(eng[k], plain[k]) for k in eng) > 0.25


def _ig_engine(weight, lam=None):
    def engine(model, d):
        res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=True)
        out, igp = res.sample, res.internal_guidance_prediction
        assert igp.dtype == F32 and out.dtype == F32
        tgt = d["target"].float()
        loss = ((out.float() - tgt) ** 2).mean() + weight * ((igp.float() - tgt) ** 2).mean()
        if lam is not None:
            loss = loss - lam * res.layersync_similarity
        loss.backward()
        return out.detach(), loss.detach()
    return engine


@pytest.mark.parametrize("full,block,ckpt", [(False, 1, "plain"), (True, 0, "segmented"), (True, 2, "per-block")])
def test_sd3_internal_guidance_gradients_slab_by_slab(monkeypatch, full, block, ckpt):
    from tests import test_internal_guidance_cpu as TI
    W.install(monkeypatch)
    model = TI._sd3_model(monkeypatch, 3, block, full)
    TI._set_ckpt(model, ckpt)
    rep, *_ = _sd3_feature_check(f"sd3 Internal Guidance {'full' if full else 'LoRA'} block {block} {ckpt}", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)),
                                 _ig_engine(TI.WEIGHT), ig=(block, TI.WEIGHT))
    assert sum(r.name.startswith(TI.PRE) and r.ref > 0 for r in rep.rows) >= 4


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_internal_guidance_with_layersync_gradients_slab_by_slab(monkeypatch, full):
    from tests import test_internal_guidance_cpu as TI
    W.install(monkeypatch)
    model = TI._sd3_model(monkeypatch, 3, 1, full)
    model.set_layersync(0, 2)
    _sd3_feature_check(f"sd3 Internal Guidance + LayerSync {'full' if full else 'LoRA'}", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)),
                       _ig_engine(TI.WEIGHT, lam=8.0), ig=(1, TI.WEIGHT), ls=(0, 2, 8.0))


@pytest.mark.parametrize("full,block,ckpt", [(False, 1, "plain"), (True, 0, "per-block"), (True, 2, "segmented")])
def test_sd3_nextlat_gradients_slab_by_slab(monkeypatch, full, block, ckpt):
    from tests import nextlat_ref as NL
    from tests import test_nextlat_cpu as TN
    W.install(monkeypatch)
    model = TN.sd3_model(NL.install, monkeypatch, 3, block, full)
    TN._set_ckpt(model, ckpt)

    def engine(model, d):
        res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=True)
        loss = ((res.sample.float() - d["target"].float()) ** 2).mean() + TN.WEIGHT * res.nextlat_state_loss
        loss.backward()
        return res.sample.detach(), loss.detach()

    rep, *_ = _sd3_feature_check(f"sd3 NextLat {'full' if full else 'LoRA'} block {block} {ckpt}", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)), engine,
                                 nl=(block, TN.WEIGHT))
    assert sum(r.name.startswith(TN.PRE) and r.ref > 0 for r in rep.rows) >= 6


@pytest.mark.parametrize("full,student,teacher,ckpt", [(False, 0, 1, "plain"), (True, 1, 2, "segmented"), (True, 2, 2, "per-block")])
def test_sd3_layersync_gradients_slab_by_slab(monkeypatch, full, student, teacher, ckpt):
    from tests import test_layersync_cpu as TL
    W.install(monkeypatch)
    model = TL._sd3_model(monkeypatch, 3)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    TL._set_ckpt(model, ckpt)
    model.set_layersync(student, teacher)

    def engine(model, d):
        out, sim = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
        loss = ((out.float() - d["target"].float()) ** 2).mean() - TL.LAMBDA * sim
        loss.backward()
        return out.detach(), loss.detach()

    _sd3_feature_check(f"sd3 LayerSync {'full' if full else 'LoRA'} s{student} t{teacher} {ckpt}", monkeypatch, model, _wide(S3._inputs(2, 16, 24, 33)), engine,
                       ls=(student, teacher, TL.LAMBDA))


@pytest.mark.parametrize("full,student,teacher,ckpt", [(False, 0, 1, "plain"), (True, 1, 3, "segmented"), (False, 2, 4, "per-block"), (True, 3, 3, "plain")])
def test_flux_layersync_gradients_slab_by_slab(monkeypatch, full, student, teacher, ckpt):
    """2 double + 3 single blocks: both double; last double -> single; both single; teacher == student"""
    from tests import layersync_ref as LS
    from tests import test_layersync_cpu as TL
    W.install(monkeypatch)
    model = TL._flux_model(monkeypatch, 2, 3)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, targets="all", init_b_std=0.02)
    TL._set_ckpt(model, ckpt)
    model.set_layersync(student, teacher)
    d = _wide(FX._inputs(2, 16, 8, 24))
    out, sim = model(hidden_states=d["packed"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], img_ids=d["img_ids"], txt_ids=d["txt_ids"],
                     guidance=d["guidance"], return_dict=False)
    loss = ((out.float() - d["target"].float()) ** 2).mean() - TL.LAMBDA * sim
    loss.backward()
    eng = _engine_grads(model)

    def oracle(dt):
        with monkeypatch.context() as m:
            outs = LS.record_flux_blocks(m)
            P, lora, scale = PU.oracle_state(model, dtype=dt)
            if full:
                P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
            lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()} or None
            f = lambda k: d[k].to(dt)
            o = OF.flux_forward(P, PU.oracle_cfg(model), f("packed"), f("prompt"), f("pooled"), f("t"), f("img_ids"), f("txt_ids"), f("guidance"), lp, scale)
            Si = d["packed"].shape[1]
            total = ((o - f("target")) ** 2).mean() - TL.LAMBDA * LS.autograd_similarity(LS.image_tokens(outs[student], Si), LS.image_tokens(outs[teacher], Si))
            total.backward()
        return o.detach(), total.detach(), _param_refs(model, P, lp)

    o64, l64, g64 = oracle(F64)
    o32, l32, g32 = oracle(F32)
    EP.check_wide(f"flux LayerSync {'full' if full else 'LoRA'} s{student} t{teacher} {ckpt}", eng, g64, g32, model.D,
                  {"prediction": (out.detach(), o64, o32), "loss": (loss.detach(), l64, l32)}).record().assert_ok()


@pytest.mark.parametrize("loss_type,with_rollout,masked", [("l2", True, False), ("huber", True, True), ("smooth_l1", False, False)])
def test_reflexflow_loss_gradient_slab_by_slab(monkeypatch, loss_type, with_rollout, masked):
    """foundation._ReflexFlowLossFn (statistics pass + loss pass, gradient from the same pass) against autograd on the reference's expression
    (tests/reflexflow_ref.py::loss64, restated here in the dtype asked for and pinned to it at fp64): exposure weight, beta2, mask, ADR term"""
    from tests import reflexflow_ref as RR
    W.install(monkeypatch)
    RR.install(monkeypatch)
    from simpletuner_amd import foundation
    B, shape = 3, (3, 16, 8, 8)
    g = torch.Generator().manual_seed(7)
    bf = lambda t: t.to(torch.bfloat16).float()
    pred, target, noisy, latents, clean, biased = (bf(torch.randn(shape, generator=g)) for _ in range(6))
    if not with_rollout:
        clean = biased = None
    emask = torch.rand(B, 64, generator=g) if masked else None
    alpha, beta1, beta2, c = 1.0, 10.0, 0.7, 0.1
    p = pred.clone().requires_grad_(True)
    loss, adr, stats = foundation._ReflexFlowLossFn.apply(p, target, noisy, latents, clean, biased, loss_type, c, emask, alpha, beta1, beta2)
    loss.backward()

    def oracle(dt):
        fl = lambda t: None if t is None else t.to(dt).reshape(B, -1)
        q = fl(pred).clone().requires_grad_(True)
        dd = q - fl(target)
        if loss_type == "l2":
            l = dd * dd
        else:
            l = (2 * c if loss_type == "huber" else 2.0) * (torch.sqrt(dd * dd + c * c) - c)
        if clean is not None:
            e = fl(clean) - fl(biased)
            l = l * (1.0 + alpha * e / e.abs().sum(1, keepdim=True).clamp_min(RR.EPS))
        l = l * beta2
        if emask is not None:
            l = l * emask.to(dt).repeat(1, l.shape[1] // 64)
        tau = fl(noisy) - fl(latents)
        t_dir = tau / torch.norm(tau, dim=1, keepdim=True).clamp_min(RR.EPS)
        p_dir = q / torch.norm(q, dim=1, keepdim=True).clamp_min(RR.EPS)
        total = (l.mean(1) + beta1 * (p_dir - t_dir).pow(2).sum(1)).mean()
        total.backward()
        return total.detach(), q.grad.reshape(shape)

    l64, g64 = oracle(F64)
    l32, g32 = oracle(F32)
    fl64 = lambda t: None if t is None else t.double().reshape(B, -1)
    pinned = RR.loss64(fl64(pred), fl64(target), fl64(noisy), fl64(latents), fl64(clean), fl64(biased), loss_type, c, emask, alpha, beta1, beta2)[0]
    assert abs(pinned.item() - l64.item()) < 1e-12 * abs(l64.item())
    EP.check_wide(f"ReflexFlow loss {loss_type} rollout={with_rollout} mask={masked}", {"d loss / d prediction": p.grad}, {"d loss / d prediction": g64},
                  {"d loss / d prediction": g32}, 0, {"loss": (loss.detach(), l64, l32)}).record().assert_ok()

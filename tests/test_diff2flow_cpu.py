"""Diff2Flow (diff2flow_enabled + diff2flow_loss) on the CPU: the restatement against the records of the executed reference (tests/golden/diff2flow_vectors.pt,
tools/gen_diff2flow_golden.py: the bridge in fp64, fp32 and bf16), the stand-in of ops.diff2flow_loss inside the kernel's derived bounds (tests/diff2flow_bounds.py),
and the plugin's host code — prepare_batch, loss, the XM passes, the refusals — on the kernel-contract emulator with the flags set."""
import logging
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import diff2flow_bounds as DB
from tests import diff2flow_ref as DR
from tests import ops_emulator as EMU
from tests import test_unet_host_sequencing_cpu as UN

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLD = Path(__file__).resolve().parent / "golden" / "diff2flow_vectors.pt"
MASKS = (None, "mask", "segmentation")
U64 = 2.0 ** -53


@pytest.fixture(scope="module")
def G():
    return torch.load(GOLD, weights_only=False)


def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True)


def _mask64(cpv, kind, hw, dtype=F64):
    """common.py:6402-6424 restated in `dtype`: [B, H * W] or None"""
    if kind is None:
        return None
    c = cpv.to(dtype)
    m = c[:, 0].unsqueeze(1) if kind == "mask" else torch.sum(c, dim=1, keepdim=True) / 3
    m = torch.nn.functional.interpolate(m, size=hw, mode="area") / 2 + 0.5
    if kind == "segmentation":
        m = (m > 0).to(dtype)
    return m.reshape(m.shape[0], -1)


def _case_operands(G, pname):
    I = G["inputs"]
    tau = (I["noise"] - I["latents"])                                  # bf16 - bf16 in the weight dtype: one rounding (bridge.flow_target)
    assert tau.dtype == BF16
    return I["preds"][pname], I["noisy_latents"], tau, torch.tensor(G["timesteps"]), ("epsilon" if pname.startswith("epsilon") else "v_prediction")


def _restated(G, pname, kind, table_dtype=None):
    """autograd through the restatement (fp64) on the fixture's operands; table_dtype: round the fp32 tables to it first"""
    pred, noisy, tau, t, mode = _case_operands(G, pname)
    tables = DR.tables32(G["alphas_cumprod"])
    if table_dtype is not None:
        tables = {k: v.to(table_dtype) for k, v in tables.items()}
    table = DR.pair_table(tables, mode)
    B = pred.shape[0]
    m = _mask64(G["inputs"]["conditioning_pixel_values"], kind, pred.shape[2:])
    m = None if m is None else m.repeat(1, pred.shape[1])
    p = pred.to(F64).reshape(B, -1).clone().requires_grad_(True)
    loss, per = DR.loss64(p, noisy.to(F64).reshape(B, -1), tau.to(F64).reshape(B, -1), t, table, mode, m)
    loss.backward()
    return loss.detach(), per.detach(), p.grad.reshape(pred.shape), table


# ---- the tables and the maps ----
def test_device_tables_are_bit_equal_to_the_reference_bridge(G):
    from simpletuner_amd.diff2flow import Diff2FlowBridge
    br = Diff2FlowBridge(G["alphas_cumprod"], device="cpu")
    for k, v in G["tables"].items():
        got = getattr(br, k)
        assert got.dtype == F32 and torch.equal(got, v), k
    assert torch.equal(br.table("epsilon"), torch.stack([G["tables"]["sqrt_recip_alphas_cumprod"], G["tables"]["sqrt_recipm1_alphas_cumprod"]], 1))
    assert torch.equal(br.table("v_prediction"), torch.stack([G["tables"]["sqrt_alphas_cumprod"], G["tables"]["sqrt_one_minus_alphas_cumprod"]], 1))
    assert torch.equal(DR.scaled_linear_acp(), G["alphas_cumprod"])
    from simpletuner_amd.foundation import DDPMSchedule
    assert torch.equal(DDPMSchedule().alphas_cumprod, G["alphas_cumprod"])              # the training schedule the plugin builds the bridge over


def test_sigma_maps_match_the_record_exactly(G):
    from simpletuner_amd.diff2flow import Diff2FlowBridge
    br = Diff2FlowBridge(G["alphas_cumprod"], device="cpu")
    assert torch.equal(br.timesteps_to_sigma(torch.arange(1000)), G["timesteps_to_sigma"])
    assert br.timesteps_to_sigma(torch.arange(4), broadcast_shape=(4, 4, 8, 8)).shape == (4, 1, 1, 1)
    assert torch.equal(br.sigma_to_timesteps(G["sigma_grid"].clone()), G["sigma_to_timesteps"])
    assert torch.equal(br.sigma_to_timesteps(G["sigma_grid_2d"].clone()), G["sigma_to_timesteps_2d"])
    assert torch.equal(br.flow_target(G["inputs"]["latents"], G["inputs"]["noise"]), G["inputs"]["noise"] - G["inputs"]["latents"])


def test_prediction_to_flow_matches_the_record(G):
    from simpletuner_amd.diff2flow import Diff2FlowBridge
    br = Diff2FlowBridge(G["alphas_cumprod"], device="cpu")
    t = torch.tensor(G["timesteps"])
    for pname in ("epsilon", "v_prediction"):
        pred, noisy = G["inputs"]["preds"][pname], G["inputs"]["noisy_latents"]
        got = br.prediction_to_flow(pred.float(), noisy.float(), t, prediction_type=pname)
        assert got.dtype == F32 and torch.equal(got, G["prediction_to_flow"][("fp32", pname)])          # the same fp32 operations in the same order
        table = DR.pair_table(DR.tables32(G["alphas_cumprod"]), pname)
        c0, c1 = DR._coeffs(table, t, 4)
        want = DR.flow64(pred.to(F64).reshape(4, -1), noisy.to(F64).reshape(4, -1), c0, c1, pname).reshape(pred.shape)
        ref = G["prediction_to_flow"][("fp64", pname)]
        assert ref.dtype == F64 and float((want - ref).abs().max()) <= 8 * U64 * float(ref.abs().max())
    with pytest.raises(ValueError, match="Unsupported prediction_type"):
        br.prediction_to_flow(pred.float(), noisy.float(), t, prediction_type="sample")


# ---- the restatement against the three runs of the reference ----
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("pname", ["epsilon", "v_prediction", "epsilon.perfect"])
def test_restatement_equals_the_fp64_bridge_record(G, pname, kind):
    loss, per, grad, _ = _restated(G, pname, kind)
    c = G["cases"][("fp64", pname, kind)]
    assert c["loss"].dtype == F64 and c["grad"].dtype == F64
    # fp64 rounding: a sum of N = 256 terms in two different orders, the terms themselves a dozen operations deep
    N = grad[0].numel()
    assert abs(float(loss - c["loss"])) <= (N + 32) * U64 * float(c["loss"].abs())
    assert float((per - c["per_sample"]).abs().max()) <= (N + 32) * U64 * float(c["per_sample"].abs().max())
    tol = 64 * U64 * grad.abs() + 64 * U64 * float(grad.abs().max()) * 1e-6
    # the gradient of one element is k_t (f - tau) scaled: f - tau cancels, so its fp64 error is relative to the cancelling terms, at most ~16x the result here
    scale = (G["inputs"]["noisy_latents"].to(F64).abs() * 16 + 4) * float(grad.abs().max())
    assert bool(((grad - c["grad"]).abs() <= tol + 64 * U64 * scale).all())


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("pname", ["epsilon", "v_prediction", "epsilon.perfect"])
def test_fp32_bridge_record_lies_inside_the_derived_bound(G, pname, kind):
    pred, noisy, tau, t, mode = _case_operands(G, pname)
    table = DR.pair_table(DR.tables32(G["alphas_cumprod"]), mode, F32)
    # the reference forms its mask in fp32 (loss.dtype): the bound is taken around the restatement ON THAT MASK, like every other operand
    m32 = _mask64(G["inputs"]["conditioning_pixel_values"], kind, pred.shape[2:], F32)
    ref = DB.loss_ref(pred, noisy, tau, t, table, mode, emask=m32, rounds=DB.AUTOGRAD_ROUNDINGS, out_bf16=False)
    c = G["cases"][("fp32", pname, kind)]
    assert c["loss"].dtype == F32
    for name, got in (("loss", c["loss"]), ("per_sample", c["per_sample"]), ("dpred", c["grad"])):
        ok, worst = DB.inside(got, *ref[name])
        print(f"[diff2flow fp32 record] {pname} mask={kind} {name}: worst |err| / bound = {worst:.3f}")
        assert ok, (name, worst)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("pname", ["epsilon", "v_prediction"])
def test_bf16_rounded_tables_reproduce_the_bf16_bridge_record(G, pname, kind):
    """the deviation is exactly the table rounding: the restatement with its tables rounded to bf16 is the reference's bf16 run (fp32 arithmetic on promoted operands)"""
    pred, noisy, tau, t, mode = _case_operands(G, pname)
    tables = {k: v.to(BF16).to(F32) for k, v in DR.tables32(G["alphas_cumprod"]).items()}
    table = DR.pair_table(tables, mode, F32)
    m32 = _mask64(G["inputs"]["conditioning_pixel_values"], kind, pred.shape[2:], F32)
    ref = DB.loss_ref(pred, noisy, tau, t, table, mode, emask=m32, rounds=DB.AUTOGRAD_ROUNDINGS, out_bf16=False)
    c = G["cases"][("bf16", pname, kind)]
    for name, got in (("loss", c["loss"]), ("per_sample", c["per_sample"]), ("dpred", c["grad"])):
        ok, worst = DB.inside(got, *ref[name])
        assert ok, (name, worst)
    # and it is NOT the fp32-table run: the two records lie further apart than two bounds, so no value is inside both
    c32 = G["cases"][("fp32", pname, kind)]
    assert abs(float(c["loss"] - c32["loss"])) > 2 * float(ref["loss"][1])


def test_perfect_prediction_floor_at_the_last_timestep(G):
    """a perfect epsilon prediction at t = 999: the bf16-table run keeps a loss above 1e-4 (bf16(sqrt(1/a)) sqrt(a) != 1), fp32 tables leave less than 1e-9"""
    fl = G["floor"]
    I = fl["inputs"]
    B = I["noise"].shape[0]
    flat = lambda x: x.to(F64).reshape(B, -1)
    tau = I["noise"] - I["latents"]
    for name, dt in (("fp32", None), ("bf16", BF16)):
        tables = DR.tables32(G["alphas_cumprod"])
        if dt is not None:
            tables = {k: v.to(dt) for k, v in tables.items()}
        table = DR.pair_table(tables, "epsilon")
        loss, per = DR.loss64(flat(I["noise"]), flat(I["noisy_latents"]), flat(tau), I["timesteps"], table, "epsilon")
        rec = float(fl[name]["loss"])
        print(f"[diff2flow floor] {name} tables: restated {float(loss):.3e}, recorded {rec:.3e}")
        if name == "bf16":
            assert float(loss) > 1e-4 and rec > 1e-4
            # fp32 arithmetic on promoted operands against fp64: |f - tau| ~ 3e-2 from terms of size ~ 15 |x|: relative error ~ 2^-24 * 15 * 4 / 3e-2
            assert abs(float(loss) - rec) <= 1e-3 * rec
        else:
            assert float(loss) < 1e-9 and rec < 1e-9


def test_closed_form_gradient_equals_autograd(G):
    for pname in ("epsilon", "v_prediction"):
        for kind in MASKS:
            loss, per, grad, table = _restated(G, pname, kind)
            pred, noisy, tau, t, mode = _case_operands(G, pname)
            m = _mask64(G["inputs"]["conditioning_pixel_values"], kind, pred.shape[2:])
            r = DR.closed64(pred, noisy, tau, t, table, mode, emask=m)
            assert float((r["dpred"] - grad).abs().max()) <= 64 * U64 * float(grad.abs().max())
            assert abs(float(r["loss"] - loss)) <= 512 * U64 * float(loss) and float((r["per_sample"] - per).abs().max()) <= 512 * U64 * float(per.max())


# ---- the stand-in inside the kernel's bounds ----
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("shape", list(DR.SHAPES))
def test_stand_in_lies_inside_the_bounds(shape, mode, kind, with_weight, want_grad):
    o = DR.operands(shape, seed=3, mask_kind=kind, with_weight=with_weight)
    pred = DR.pred_of(o, mode)
    assert pred.is_contiguous() != o.strided
    table = DR.pair_table(o.tables, mode, F32)
    loss, per, dpred = DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, mode, weight=o.weight, want_grad=want_grad, grad_scale=1.0, emask=o.emask)
    ref = DB.loss_ref(pred, o.noisy, o.tau, o.timesteps, table, mode, emask=o.emask, weight=o.weight)
    assert loss.dtype == F32 and loss.shape == (1,) and per.shape == (o.B,) and (dpred is None) == (not want_grad)
    assert DB.inside(loss, *ref["loss"])[0] and DB.inside(per, *ref["per_sample"])[0]
    if want_grad:
        assert dpred.dtype == BF16 and dpred.shape == pred.shape and dpred.is_contiguous() and DB.inside(dpred, *ref["dpred"])[0]


def test_stand_in_clamps_the_timestep_and_checks_its_operands():
    o = DR.operands("small", seed=4, timesteps=[1000, -3])
    table = DR.pair_table(o.tables, "epsilon", F32)
    pred = DR.pred_of(o, "epsilon")
    a = DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, "epsilon")
    b = DR.diff2flow_loss(pred, o.noisy, o.tau, torch.tensor([999, 0]), table, "epsilon")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(Exception):
        DR.diff2flow_loss(pred.float(), o.noisy, o.tau, o.timesteps, table, "epsilon")
    with pytest.raises(Exception):
        DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps.int(), table, "epsilon")
    with pytest.raises(Exception):
        DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, "sample")


# ---- the plugin on the emulator ----
def _sdxl_batch(B=2, hw=(16, 16), seed=2, timesteps=(500, 999)):
    g = torch.Generator().manual_seed(seed)
    return {"latent_batch": torch.randn(B, 4, *hw, generator=g).to(BF16), "prompt_embeds": torch.randn(B, 9, 128, generator=g).to(BF16),
            "add_text_embeds": torch.randn(B, 64, generator=g).to(BF16), "batch_time_ids": torch.tensor([[64.0, 48.0, 0.0, 0.0, 64.0, 48.0]] * B).to(BF16),
            "timesteps": torch.tensor(list(timesteps)), "noise": torch.randn(B, 4, *hw, generator=g).to(BF16)}


def _plugin(monkeypatch, family, **over):
    DR.install(monkeypatch)
    from simpletuner_amd.training.trainer import default_config
    cfg = default_config(model_family=family, model_type="lora", lora_rank=16, lora_alpha=16.0, lora_init_b_std=0.05, train_batch_size=2, **over)
    if family == "sdxl":
        from simpletuner_amd.sdxl.model import SDXL as Cls
        arch = UN.SMALL
    else:
        from simpletuner_amd.sd1x.model import StableDiffusion1, StableDiffusion2
        Cls = StableDiffusion2 if family == "sd2x" else StableDiffusion1
        arch = UN.SD15_WIDE
    pl = Cls(cfg, _acc())
    pl.load_model(**arch)
    pl.add_lora_adapter()
    return pl, arch


def _unet_oracle_grads(pl, arch, prepared, loss_of, sdxl):
    """autograd through the oracle UNet (fp64, adapters merged into effective weights) and `loss_of(prediction [B, N] fp64)`"""
    from oracle.unet import UNetConfig, unet_forward
    m = pl.model
    rank, alpha = 16, 16.0
    P = {k: v.detach().to(F64) for k, v in m.diffusers_state_dict().items()}
    lora = {n: p.detach().to(F64).clone().requires_grad_(True) for n, p in m.named_parameters() if ".lora_" in n}
    Pe = dict(P)
    for n in lora:
        if ".lora_A." in n:
            base = n.replace(".lora_A.default.weight", "")
            Pe[base + ".weight"] = P[base + ".weight"] + (alpha / rank) * lora[base + ".lora_B.default.weight"] @ lora[n]
    ack = prepared["added_cond_kwargs"]
    ack = {"text_embeds": ack["text_embeds"].to(F64), "time_ids": ack["time_ids"].to(F64)} if sdxl else None
    ref = unet_forward(Pe, UNetConfig(**arch), prepared["noisy_latents"].to(F64), prepared["timesteps"].to(F64), prepared["encoder_hidden_states"].to(F64), ack)
    B = ref.shape[0]
    loss = loss_of(ref.reshape(B, -1))
    loss.backward()
    return ref.detach(), loss.detach(), {n: v.grad for n, v in lora.items()}


@pytest.mark.parametrize("family", ["sdxl", "sd2x"])
def test_tiny_lora_step_trains_the_flow_objective(monkeypatch, family):
    """FAILS WITHOUT THE FEATURE (the flags were never read: the step trained the plain epsilon / v MSE).  A tiny SDXL (epsilon) and a tiny SD 2.x (v-prediction)
    LoRA step on the kernel-contract emulator with both flags set: the loss is the restatement on the engine's own prediction, far from the plain MSE of that
    prediction, and every adapter gradient matches autograd through the oracle UNet plus the restated loss at the UNet LoRA tolerances (2e-2 / 6e-2)."""
    pl, arch = _plugin(monkeypatch, family, diff2flow_enabled=True, diff2flow_loss=True)
    mode = "epsilon" if family == "sdxl" else "v_prediction"
    assert pl.PREDICTION_TYPE.value == mode
    batch = _sdxl_batch()
    if family != "sdxl":
        batch.pop("add_text_embeds"); batch.pop("batch_time_ids")
    prepared = pl.prepare_batch(dict(batch), {"global_step": 0})
    tau = prepared["flow_target"]
    assert tau.dtype == BF16 and torch.equal(tau, (batch["noise"] - batch["latent_batch"]))                 # bf16, one rounding
    out = pl.model_predict(prepared)
    pred = out["model_prediction"]
    loss = pl.loss(prepared, out)
    loss.backward()
    table = pl.diff2flow_value().table(mode)
    p16 = pred.detach().to(BF16)
    ref = DB.loss_ref(p16, prepared["noisy_latents"], tau, prepared["timesteps"], table, mode)
    ok, worst = DB.inside(loss.detach().reshape(1), ref["loss"][0].reshape(1), ref["loss"][1].reshape(1))
    assert ok, worst
    target = pl.get_prediction_target(prepared)
    plain = float(((p16.double() - target.double()) ** 2).mean())
    print(f"[diff2flow {family}] loss {loss.item():.6f} (restated {float(ref['loss'][0]):.6f}, bound {float(ref['loss'][1]):.2e}), plain MSE of the same prediction {plain:.6f}")
    assert abs(plain - float(ref["loss"][0])) > 100 * float(ref["loss"][1])
    B = pred.shape[0]
    flat = lambda x: x.to(F64).reshape(B, -1)
    loss_of = lambda p: DR.loss64(p, flat(prepared["noisy_latents"]), flat(tau), prepared["timesteps"], table, mode)[0]
    o_pred, o_loss, grads = _unet_oracle_grads(pl, arch, prepared, loss_of, family == "sdxl")
    assert UN._rel(pred.detach(), o_pred) < 2e-2
    worst = (0.0, "")
    for n, p in pl.model.named_parameters():
        if ".lora_" in n:
            r = UN._rel(p.grad, grads[n])
            worst = max(worst, (r, n))
            assert r < 6e-2, (n, r)
    print(f"[diff2flow {family}] oracle loss {float(o_loss):.6f}; worst adapter gradient rel_l2 {worst[0]:.3e} at {worst[1]}")


def test_sd1x_with_a_configured_prediction_type(monkeypatch):
    pl, _ = _plugin(monkeypatch, "sd1x", diff2flow_enabled=True, diff2flow_loss=True, prediction_type="v_prediction")
    assert pl.PREDICTION_TYPE.value == "v_prediction"
    o = DR.operands("small", seed=5)
    pb = {"noisy_latents": o.noisy, "flow_target": o.tau, "timesteps": o.timesteps, "velocity_target": o.tau}
    pred = DR.pred_of(o, "v_prediction")
    loss = pl.loss(pb, {"model_prediction": pred})
    ref = DB.loss_ref(pred, o.noisy, o.tau, o.timesteps, DR.pair_table(o.tables, "v_prediction", F32), "v_prediction")
    assert DB.inside(loss.reshape(1), ref["loss"][0].reshape(1), ref["loss"][1].reshape(1))[0]


@pytest.mark.parametrize("branch", ["trunk_lora", "controlnet"])
def test_pixart_step_through_the_plugin_trains_the_flow_objective(monkeypatch, branch):
    """FAILS WITHOUT THE FEATURE.  PixArt-Sigma through the plugin — prepare_batch, model_predict (the trunk with LoRA) or controlnet_predict (the ControlNet
    branch), loss — with both flags set.  The prediction is the leading half of the 8-channel output (`.chunk(2, dim=1)[0]`): the loss reads it in place and autograd
    carries the compact gradient back through the chunk.  The loss is the restatement on the engine's own prediction, far from the plain epsilon MSE; every trained
    tensor's gradient matches autograd on the oracle plus the restated loss at the PixArt tolerances (2e-2 prediction, 6e-2 / 8e-2 gradients)."""
    DR.install(monkeypatch)
    from oracle.pixart import PixArtConfig, controlnet_forward, pixart_forward
    from simpletuner_amd.pixart.model import PixartSigma
    from simpletuner_amd.pixart.transformer import HP
    from simpletuner_amd.training.trainer import default_config
    from tests import test_pixart_host_sequencing_cpu as PX
    cn = branch == "controlnet"
    cfg = default_config(model_family="pixart_sigma", model_type="full" if cn else "lora", lora_rank=8, lora_alpha=16.0, lora_init_b_std=0.05, train_batch_size=2,
                         diff2flow_enabled=True, diff2flow_loss=True, controlnet=cn)
    pl = PixartSigma(cfg, _acc())
    pl.load_model(**PX.ARCH)
    m = pl.model
    if cn:
        ctl = pl.controlnet_init(num_layers=2, synthetic_adapter=True)
    else:
        pl.add_lora_adapter()
    pl.get_trained_component().train()
    lat, cond, enc, mask, t = PX._inputs()
    noise = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4)).to(BF16)
    batch = {"latent_batch": lat, "prompt_embeds": enc, "encoder_attention_mask": mask, "timesteps": t.long(), "noise": noise}
    if cn:
        batch["conditioning_latents"] = cond
    prepared = pl.prepare_batch(dict(batch), {"global_step": 0})
    tau = prepared["flow_target"]
    assert torch.equal(tau, noise - lat)
    out = pl.model_predict(prepared)
    pred = out["model_prediction"]
    assert pred.shape == lat.shape and not pred.is_contiguous()                                    # the channel half of the wider output, in place
    loss = pl.loss(prepared, out)
    loss.backward()
    noisy, tt = prepared["noisy_latents"], prepared["timesteps"]
    table = pl.diff2flow_value().table("epsilon")
    p16 = pred.detach().to(BF16)
    ref = DB.loss_ref(p16, noisy, tau, tt, table, "epsilon")
    assert DB.inside(loss.detach().reshape(1), ref["loss"][0].reshape(1), ref["loss"][1].reshape(1))[0]
    plain = float(((p16.double() - noise.double()) ** 2).mean())
    assert abs(plain - float(ref["loss"][0])) > 100 * float(ref["loss"][1])
    res, ar = torch.tensor([[16.0, 16.0]]).expand(2, -1), torch.tensor([[1.0]]).expand(2, -1)
    flat = lambda x: x.to(F64).reshape(2, -1)
    restated = lambda o: DR.loss64(flat(o.chunk(2, dim=1)[0]), flat(noisy), flat(tau), tt, table, "epsilon")[0]
    if cn:
        P = {k: v.detach().float() for k, v in m.named_parameters()}
        C = {k: v.float().clone().requires_grad_(True) for k, v in ctl.adapter_state_dict().items()}
        o = controlnet_forward(P, C, PixArtConfig(**PX.ARCH), 2, noisy.float(), cond.float(), enc.float(), mask, tt.float(), res, ar)
        restated(o).backward()
        assert PX._rel(pred.detach(), o.chunk(2, dim=1)[0].detach()) < 2e-2
        got = {}
        for i, (blk, ex) in enumerate(ctl.cblocks):
            got.update({f"controlnet_blocks.{i}.transformer_block.{k}": g for k, g in blk.G.items()})
            got.update({f"controlnet_blocks.{i}.{k}": g for k, g in ex.G.items()})
        assert set(got) == set(C)
        for k, g in got.items():
            if k.endswith("to_k.bias"):          # softmax-invariant: the true gradient is zero, both sides hold rounding noise
                continue
            r = PX._rel(g, C[k].grad)
            assert r < (8e-2 if (k.endswith(".bias") or k.endswith("scale_shift_table")) else 6e-2), (k, r)
        return
    P = {k: v.detach().float() for k, v in m.named_parameters() if ".lora_" not in k}
    lp = PX._true_lora(m)
    o = pixart_forward(P, PixArtConfig(**PX.ARCH), noisy.float(), enc.float(), mask, tt.float(), res, ar, lora=lp, lora_scale=16.0 / 8)
    restated(o).backward()
    assert PX._rel(pred.detach(), o.chunk(2, dim=1)[0].detach()) < 2e-2
    H, hd = PX.ARCH["num_attention_heads"], PX.ARCH["attention_head_dim"]
    for name, p in m.named_parameters():
        if ".lora_" not in name:
            continue
        mod, which = name.split(".lora_")
        gr = p.grad
        if which.startswith("A") and gr.shape[1] == H * HP:
            gr = gr.view(gr.shape[0], H, HP)[:, :, :hd].reshape(gr.shape[0], H * hd)
        if which.startswith("B") and gr.shape[0] == H * HP:
            gr = gr.view(H, HP, gr.shape[1])[:, :hd].reshape(H * hd, gr.shape[1])
        r = PX._rel(gr, lp[mod][0 if which.startswith("A") else 1].grad)
        assert r < 6e-2, (name, r)


def _loss_only_plugin(monkeypatch, **over):
    DR.install(monkeypatch)
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import default_config
    pl = SDXL(default_config(model_family="sdxl", model_type="lora", **over), _acc())
    pl.setup_training_noise_schedule()
    return pl


def _loss_batch(o, mode="epsilon"):
    return {"noisy_latents": o.noisy, "flow_target": o.tau, "timesteps": o.timesteps, "noise": o.tau}, DR.pred_of(o, mode)


def test_loss_type_and_snr_gamma_change_nothing_under_the_flags(monkeypatch, caplog):
    o = DR.operands("small", seed=6)
    vals = []
    with caplog.at_level(logging.INFO, logger="simpletuner_amd.diff2flow"):
        for over in (dict(), dict(loss_type="huber"), dict(snr_gamma=5.0), dict(loss_type="smooth_l1", snr_gamma=5.0, snr_weight=0.5)):
            pl = _loss_only_plugin(monkeypatch, diff2flow_enabled=True, diff2flow_loss=True, **over)
            pb, pred = _loss_batch(o)
            p = pred.clone().requires_grad_(True)
            loss = pl.loss(pb, {"model_prediction": p})
            loss.backward()
            pl.loss(pb, {"model_prediction": p})
            vals.append((loss.detach().clone(), p.grad.clone()))
    assert all(torch.equal(v[0], vals[0][0]) and torch.equal(v[1], vals[0][1]) for v in vals)
    said = [r for r in caplog.records if "loss_type" in r.getMessage() and "snr_gamma" in r.getMessage() and "snr_weight" in r.getMessage()]
    assert len(said) == 4 and all(r.levelno == logging.INFO for r in said)                     # once per bridge, not once per call
    # and the flag that does nothing alone: diff2flow_loss without diff2flow_enabled is the plain epsilon MSE
    pl = _loss_only_plugin(monkeypatch, diff2flow_loss=True)
    pb, pred = _loss_batch(o)
    plain = pl.loss(pb, {"model_prediction": pred})
    assert pl.diff2flow_value() is None and float(plain) == pytest.approx(float(((pred.double() - o.tau.double()) ** 2).mean()), rel=1e-5)


def test_conditioning_mask_reaches_the_flow_loss(monkeypatch):
    o = DR.operands("small", seed=7)
    pl = _loss_only_plugin(monkeypatch, diff2flow_enabled=True, diff2flow_loss=True)
    pb, pred = _loss_batch(o)
    cpv = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)) * 2 - 1
    for kind in ("mask", "segmentation"):
        pbm = dict(pb, loss_mask_type=kind, conditioning_pixel_values=cpv)
        m = _mask64(cpv, kind, (8, 8), F32)
        ref = DB.loss_ref(pred, o.noisy, o.tau, o.timesteps, DR.pair_table(o.tables, "epsilon", F32), "epsilon", emask=m)
        assert DB.inside(pl.loss(pbm, {"model_prediction": pred}).reshape(1), ref["loss"][0].reshape(1), ref["loss"][1].reshape(1))[0]
        unmasked = pl.loss(pbm, {"model_prediction": pred}, apply_conditioning_mask=False)
        assert torch.equal(unmasked, pl.loss(pb, {"model_prediction": pred}))


def test_xm_per_sample_losses_are_the_plain_calls_per_sample(monkeypatch):
    o = DR.operands("small", seed=8, shape=(4, 4, 8, 8), timesteps=[100, 200, 100, 200])
    pl = _loss_only_plugin(monkeypatch, diff2flow_enabled=True, diff2flow_loss=True, snr_gamma=5.0, xm_enabled=True, xm_candidate_count=2)
    pb, pred = _loss_batch(o)
    table = DR.pair_table(o.tables, "epsilon", F32)
    _, want, _ = DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, "epsilon")
    per, base_w = pl.loss(pb, {"model_prediction": pred}, _per_sample_only=True)
    assert base_w is None and torch.equal(per, want)                                       # no min-SNR factor on this branch
    w = torch.tensor([0.0, 2.0, 2.0, 0.0])
    p = pred.clone().requires_grad_(True)
    loss = pl.loss(pb, {"model_prediction": p}, _row_weight=w)
    loss.backward()
    l2, _, d2 = DR.diff2flow_loss(pred, o.noisy, o.tau, o.timesteps, table, "epsilon", weight=w)
    assert torch.equal(loss.reshape(1), l2) and torch.equal(p.grad, d2) and float(p.grad[0].abs().max()) == 0.0
    # the whole XM pass: winners by the flow loss
    pb.update(latents=o.tau, metadata=[{"id": i % 2} for i in range(4)], xm_candidate_count=2, xm_original_batch_size=2)
    out = {"model_prediction": pred.clone().requires_grad_(True), "xm_candidate_count": 2}
    loss, logs = pl.loss_with_logs(pb, out)
    cand = want.reshape(2, 2)
    assert out["xm_winner_indices"].tolist() == cand.argmin(0).tolist() and logs["xm_loss"] == pytest.approx(float(loss.detach()))


@pytest.mark.parametrize("family", ["flux", "sd3"])
def test_flags_on_a_flow_matching_family_leave_the_launch_stream_unchanged(monkeypatch, family):
    import sys
    calls = []

    def run(**over):
        ops = DR.install(monkeypatch)
        from simpletuner_amd.training.trainer import default_config
        calls.clear()
        for name in EMU._EMULATED:
            fn = getattr(ops, name)
            monkeypatch.setattr(ops, name, (lambda n, f: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(name, fn))
        if family == "flux":
            from simpletuner_amd.flux.model import Flux as Cls
        else:
            from simpletuner_amd.sd3.model import SD3 as Cls
        pl = Cls(default_config(model_family=family, **over), _acc())
        assert pl.diff2flow_value() is None
        g = torch.Generator().manual_seed(3)
        lat, noise = torch.randn(2, 16, 8, 8, generator=g).to(BF16), torch.randn(2, 16, 8, 8, generator=g).to(BF16)
        pl.sample_flow_sigmas = lambda batch, state: (torch.tensor([0.3, 0.7]), torch.tensor([300.0, 700.0]))
        prepared = pl.prepare_batch({"latent_batch": lat, "noise": noise}, {"global_step": 0})
        pred = torch.randn(2, 16, 8, 8, generator=g).to(BF16)
        loss = pl.loss(prepared, {"model_prediction": pred})
        return list(calls), loss, prepared["flow_target"]

    sys.modules.pop("simpletuner_amd.diff2flow", None)
    c0, l0, t0 = run()
    c1, l1, t1 = run(diff2flow_enabled=True, diff2flow_loss=True)
    assert c0 == c1 and len(c0) > 0 and torch.equal(l0, l1) and torch.equal(t0, t1)
    assert "simpletuner_amd.diff2flow" not in sys.modules                                    # never imported on a flow-matching family


def test_flags_absent_import_nothing_and_launch_the_parents_stream(monkeypatch):
    import sys
    sys.modules.pop("simpletuner_amd.diff2flow", None)
    pl = _loss_only_plugin(monkeypatch)
    called = []
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "diff2flow_loss", lambda *a, **k: called.append(1))
    prepared = pl.prepare_batch(_sdxl_batch(), {"global_step": 0})
    assert "flow_target" not in prepared
    pl.loss(prepared, {"model_prediction": prepared["noise"]})
    assert not called and "simpletuner_amd.diff2flow" not in sys.modules and not hasattr(pl, "_diff2flow")


def test_zero_terminal_snr_with_epsilon_is_refused_by_name(monkeypatch):
    DR.install(monkeypatch)
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.sd1x.model import StableDiffusion2
    from simpletuner_amd.training.trainer import default_config
    pl = SDXL(default_config(model_family="sdxl", diff2flow_enabled=True, diff2flow_loss=True, rescale_betas_zero_snr=True), _acc())
    with pytest.raises(NotImplementedError) as e:
        pl.setup_training_noise_schedule()
    msg = str(e.value)
    assert "diff2flow_loss" in msg and "diff2flow_enabled" in msg and "rescale_betas_zero_snr" in msg
    # v-prediction carries a zero terminal SNR: sqrt(a) = 0, sqrt(1 - a) = 1, nothing infinite
    pv = StableDiffusion2(default_config(model_family="sd2x", diff2flow_enabled=True, diff2flow_loss=True, rescale_betas_zero_snr=True), _acc())
    pv.setup_training_noise_schedule()
    assert bool(torch.isfinite(pv.diff2flow_value().table("v_prediction")).all())
    # and the flag alone (no loss) builds the target without the tables being used: not refused
    pe = SDXL(default_config(model_family="sdxl", diff2flow_enabled=True, rescale_betas_zero_snr=True), _acc())
    pe.setup_training_noise_schedule()


def test_enabled_alone_only_adds_the_flow_target(monkeypatch):
    pl = _loss_only_plugin(monkeypatch, diff2flow_enabled=True, input_perturbation=0.1)
    base2 = _loss_only_plugin(monkeypatch, input_perturbation=0.1)
    b = _sdxl_batch()
    torch.manual_seed(0)
    prepared0 = base2.prepare_batch(dict(b), {"global_step": 0})
    torch.manual_seed(0)
    prepared1 = pl.prepare_batch(dict(b), {"global_step": 0})
    assert torch.equal(prepared1["flow_target"], b["noise"] - b["latent_batch"])            # the UN-perturbed noise
    assert not torch.equal(prepared1["input_noise"], prepared1["noise"])
    assert set(prepared1) - set(prepared0) == {"flow_target"} and set(prepared0) <= set(prepared1)
    assert all(torch.equal(prepared0[k], prepared1[k]) for k in prepared0 if torch.is_tensor(prepared0[k]))
    pred = prepared1["noise"] * 0.5
    assert torch.equal(pl.loss(prepared1, {"model_prediction": pred}), base2.loss(prepared0, {"model_prediction": pred}))      # the plain epsilon MSE

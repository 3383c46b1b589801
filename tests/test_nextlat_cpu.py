"""NextLat (helpers/training/nextlat.py) on the CPU: the fp64 restatement against the executed reference's golden file, the stand-ins against the derived bounds,
the index rule, the plugin / trainer / file surface, and the SD3 engine's host sequencing — where the state loss leaves the network's autograd node and where its
gradient enters the hand-written dX chain, under every checkpoint mode — against autograd through the oracle (tests/ops_emulator.py + the stand-ins of
tests/nextlat_ref.py)."""
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import internal_guidance_bounds as IB
from tests import layersync_ref as LS
from tests import nextlat_bounds as NB
from tests import nextlat_ref as NL
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GOLDEN = Path(__file__).resolve().parent / "golden" / "nextlat_vectors.pt"
# the weight of the engine cases: large enough that the regulariser's share of the trunk gradient is well above the gradient tolerances (every case asserts the
# measured share >= 0.1) — a dropped or misplaced injection then misses them by a wide margin
WEIGHT = 8.0
PRE = NL.PREFIX


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=True)


def _params(golden):
    return tuple(golden["params"][nm] for nm in NL.NAMES)


# ------------------------------------------------------------------------------------------------
# (a) the restatement against the executed reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["smooth_l1", "mse", "constant_row"])
def test_restatement_equals_the_executed_reference(golden, case):
    """prediction, loss, logs, the hidden-state gradient and the six parameter gradients of NextLatRegularizer.compute_loss, to the project's oracle-pinning
    tolerance: 1e-5 of each tensor's largest entry (1e-5 max(1, |value|) for the scalars), the constant-row case included."""
    g = golden[case]
    h = g["hidden"]
    B, S, D = h.shape
    assert (B, S, D) == tuple(golden["shape"]) == (2, 35, 64)
    loss, logs, pred, dh, grads = NL.loss64(h, _params(golden), g["weight"], g["state_loss"])
    x = h[:, :-1].double().reshape(-1, D)
    tol = 1e-5
    ref = g["prediction"].double().reshape(-1, D)
    assert ((pred.reshape(-1, D) - ref).abs() <= tol * ref.abs().max()).all()
    assert abs(loss.item() - g["loss"].item()) <= tol * max(1.0, g["loss"].item())
    for k in ("nextlat_loss", "nextlat_state_loss"):
        assert abs(logs[k] - g["logs"][k]) <= tol * max(1.0, g["logs"][k]), k
    assert set(g["logs"]) == {"nextlat_loss", "nextlat_state_loss"} and abs(g["logs"]["nextlat_loss"] - g["weight"] * g["logs"]["nextlat_state_loss"]) < 1e-6
    rh = g["grad_hidden"].double()
    assert rh.abs().max() > 0 and ((dh - rh).abs() <= tol * rh.abs().max()).all()
    assert (rh[:, -1] == 0).all() and (dh[:, -1] == 0).all()                  # row S - 1 of every sample: only the detached target reads it
    for nm in NL.NAMES:
        r = g["grads"][nm].double()
        assert r.abs().max() > 0 and ((grads[nm] - r).abs() <= tol * r.abs().max()).all(), nm
    if case == "constant_row":
        b0, r0 = g["row"]
        xh, rs = NL.rows64(x)
        i = b0 * (S - 1) + r0
        assert xh[i].abs().max() == 0 and abs(rs[i].item() - 1000.0) < 1e-6
    if case == "smooth_l1":
        assert 0.1 <= g["linear_share"] <= 0.9                                # both regimes of smooth-L1 are exercised
        d = (pred - h[:, 1:].double()).abs()
        assert abs((d >= 1).double().mean().item() - g["linear_share"]) < 1e-3


def test_index_rule_init_and_state_dict_keys_equal_the_executed_reference(golden):
    from simpletuner_amd.engine import NEXTLAT_NAMES, nextlat_index, nextlat_shapes
    table = {"None": None, "0": 0, "-1": -1, "2": 2, "1": 1}
    assert golden["index_table"] == {"None": 2, "0": 2, "-1": 2, "2": 2, "1": 1}          # a configured 0 also means the last block
    for key, want in golden["index_table"].items():
        assert nextlat_index(table[key], 3) == want, key
    with pytest.raises(ValueError) as ei:
        nextlat_index(3, 3)
    assert str(ei.value) == golden["errors"]["index_high"] == "nextlat_block_index must be within [-1, 2], got 3."
    sk = golden["state_keys"]
    assert sk["module_name"] + "." == NL.PREFIX and sk["keys"] == ["block_index", *NEXTLAT_NAMES] and NEXTLAT_NAMES == NL.NAMES
    assert sk["block_index_dtype"] == "torch.int64" and sk["block_index_shape"] == ()
    assert [sk["shapes"][nm] for nm in NEXTLAT_NAMES] == list(nextlat_shapes(64))
    init = golden["init"]
    assert init["down_zero"] and init["norm_weight_one"] and init["norm_bias_zero"] and init["eps"] == NL.EPS and init["up_abs_max"] <= init["up_bound"] == 0.125


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins (the kernels' contracts in plain torch) against the derived bounds
# ------------------------------------------------------------------------------------------------
def check_kernels(fns, dev, B, S, D, lead, bf16_params, mode, seed=0):
    """Shared with tests/test_nextlat_gpu.py: run every NextLat entry of `fns` (the ops wrappers or the stand-ins) on seeded operands — the row views with `lead`
    foreign rows ahead of each sample's S token rows — and hold EVERY output element to tests/nextlat_bounds.py, each kernel against the fp64 value of its own
    stored operands.  Returns the outputs (for bit-equality of a second call)."""
    g = torch.Generator().manual_seed(seed + D + lead)
    rows, M, N = S - 1, B * (S - 1), 2 * D
    pdt = BF16 if bf16_params else F32
    rn = lambda *s: torch.randn(*s, generator=g)
    joint = rn(B, lead + S, D).to(BF16)
    if rows > 4:
        joint[0, lead + 3] = 2.0 ** -7                                        # constant row: xhat = 0, rstd = 1000
    params = [(1.0 + 0.25 * rn(D)).to(pdt), (0.1 * rn(D)).to(pdt), (rn(N, D) / D ** 0.5).to(pdt), (0.05 * rn(N)).to(pdt), (rn(D, N) / N ** 0.5).to(pdt), (0.05 * rn(D)).to(pdt)]
    U_ = (1.5 * rn(M, N)).to(BF16); U_[0, :8] = torch.tensor([-9.0, -6.0, -5.0, -0.0, 0.0, 5.0, 6.0, 9.0]).to(BF16)          # the erf tails and both zeros
    dA = rn(M, N).to(BF16)
    pred = (joint[:, lead + 1:].float().reshape(M, D) + 1.2 * rn(M, D)).to(BF16)          # |pred - t| on both sides of 1
    gg = rn(M, D).to(BF16)
    dxj = rn(B, lead + S, D).to(BF16)
    P1, db1, P2, db2 = rn(N, D).to(BF16), rn(N), rn(D, N).to(BF16), rn(D)
    scale = torch.tensor([0.37 / (M * D)], dtype=F32)
    to = lambda t: t.to(dev)
    joint, U_, dA, pred, gg, dxj, P1, db1, P2, db2, scale = map(to, (joint, U_, dA, pred, gg, dxj, P1, db1, P2, db2, scale))
    params = [to(p) for p in params]
    view, tview, dxv = joint[:, lead:lead + rows], joint[:, lead + 1:], dxj[:, lead:lead + rows]
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)
    cpu = lambda t: t.detach().cpu()
    worst = {}

    def hold(name, got, ref, tol):
        err = (cpu(got).double().reshape(ref.shape) - ref).abs()
        assert torch.isfinite(cpu(got).float()).all(), name
        tol = tol.expand_as(ref) if torch.is_tensor(tol) and tol.dim() else torch.full_like(ref, float(tol))
        worst[name] = (err / tol.clamp_min(1e-300)).max().item()
        assert not (err > tol).any(), f"{name} D={D} lead={lead}: {int((err > tol).sum())} elements over the bound, worst err/tol {worst[name]:.3f}"

    # fold
    W1f, W1fT, c1, Wd, WdT, bd = z(N, D), z(D, N), z(N), z(D, N), z(N, D), z(D)
    fns["nextlat_fold"](*params, W1f, W1fT, c1, Wd, WdT, bd)
    fb = NB.fold_bounds(*(cpu(p) for p in params))
    for nm, got in (("W1f", W1f), ("c1", c1), ("Wd", Wd), ("bd", bd)):
        hold(nm, got, *fb[nm])
    assert torch.equal(cpu(W1fT), cpu(W1f).t()) and torch.equal(cpu(WdT), cpu(Wd).t())
    # row pass (st355_ig_head_fwd as it is, on the view h[:, :S-1])
    xhat, rstd = z(M, D), z(M, dt=F32)
    fns["nextlat_rows"](view, xhat, rstd)
    xh64, tx, rs64, trs = IB.fwd_bounds(cpu(view).reshape(M, D))
    hold("xhat", xhat, xh64, tx); hold("rstd", rstd, rs64, trs)
    # GELU
    A, dU = z(M, N), z(M, N)
    fns["gelu_erf"](U_, A)
    hold("A", A, *NB.gelu_fwd_bounds(cpu(U_)))
    fns["gelu_erf_bwd"](U_, dA, dU)
    hold("dU", dU, *NB.gelu_bwd_bounds(cpu(U_), cpu(dA)))
    inpl = dA.clone()
    fns["gelu_erf_bwd"](U_, inpl, inpl)
    assert torch.equal(cpu(inpl), cpu(dU))                                    # dU may be dA
    # loss (pred overwritten with psi)
    psi, loss = pred.clone(), z(1, dt=F32)
    fns["nextlat_loss"](psi, tview, mode, loss)
    l64, tl, p64, tp = NB.loss_bounds(cpu(pred), cpu(tview).reshape(M, D), mode)
    hold("loss", loss, l64.reshape(1), tl); hold("psi", psi, p64, tp)
    lin = ((cpu(pred).double() - cpu(tview).double().reshape(M, D)).abs() >= 1).double().mean().item()
    assert 0.1 <= lin <= 0.9, lin
    # LayerNorm backward added into the dX view
    dx0 = dxj.clone()
    fns["nextlat_ln_bwd_add"](gg, xhat, rstd, scale * (M * D), dxv)
    o64, to_ = NB.ln_bwd_add_bounds(cpu(gg), cpu(xhat), cpu(rstd), cpu(scale * (M * D)).item(), cpu(dx0)[:, lead:lead + rows].reshape(M, D))
    hold("dx", dxv.reshape(M, D), o64, to_)
    assert torch.equal(cpu(dxj)[:, :lead], cpu(dx0)[:, :lead]) and torch.equal(cpu(dxj)[:, lead + rows:], cpu(dx0)[:, lead + rows:])      # the lead rows and row S - 1: bit-equal
    assert (cpu(dxj)[:, lead:lead + rows] != cpu(dx0)[:, lead:lead + rows]).any()
    # weight gradients
    gU = [z(D, dt=pdt), z(D, dt=pdt), z(N, D, dt=pdt), z(N, dt=pdt)]
    fns["nextlat_wgrad_up"](P1, db1, params[0], params[1], params[2], scale, *gU)
    wb = NB.wgrad_up_bounds(cpu(P1), cpu(db1), cpu(params[0]), cpu(params[1]), cpu(params[2]), cpu(scale).item(), bf16_params)
    for nm, got in zip(("g_gamma", "g_beta", "g_W", "g_b"), gU):
        hold("up." + nm, got, *wb[nm])
    gD = [z(D, N, dt=pdt), z(D, dt=pdt)]
    fns["nextlat_wgrad_down"](P2, db2, scale, *gD)
    wd = NB.wgrad_down_bounds(cpu(P2), cpu(db2), cpu(scale).item(), bf16_params)
    for nm, got in zip(("g_W", "g_b"), gD):
        hold("down." + nm, got, *wd[nm])
    # accumulate adds to what the gradient tensors hold: fp32(held) + the new value, one more rounding in the gradients' dtype (exact doubling would hide a dropped
    # read of what is held; the bound is the kernel's own: held value + fp64 reference, the reference's error plus one fp32 addition, then the store's rounding)
    held = [cpu(t).double() for t in gU + gD]
    twice = [t.clone() for t in gU + gD]
    fns["nextlat_wgrad_up"](P1, db1, params[0], params[1], params[2], scale, *twice[:4], accumulate=True)
    fns["nextlat_wgrad_down"](P2, db2, scale, *twice[4:], accumulate=True)
    raw_u = NB.wgrad_up_bounds(cpu(P1), cpu(db1), cpu(params[0]), cpu(params[1]), cpu(params[2]), cpu(scale).item(), False)
    raw_d = NB.wgrad_down_bounds(cpu(P2), cpu(db2), cpu(scale).item(), False)
    raws = [raw_u[nm] for nm in ("g_gamma", "g_beta", "g_W", "g_b")] + [raw_d[nm] for nm in ("g_W", "g_b")]
    for nm, h0, t, (ref, e) in zip(("up.g_gamma", "up.g_beta", "up.g_W", "up.g_b", "down.g_W", "down.g_b"), held, twice, raws):
        want = h0.reshape(ref.shape) + ref
        e_acc = e + NB.U * want.abs()
        hold("acc." + nm, t, want, NB._rounded(want, e_acc) if bf16_params else e_acc)
        assert (cpu(t).double().reshape(ref.shape) != h0.reshape(ref.shape)).any(), nm
    print(f"[nextlat] D={D} lead={lead} {mode} {'bf16' if bf16_params else 'fp32'} params: worst err/bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    return [cpu(t) for t in (W1f, W1fT, c1, Wd, WdT, bd, xhat, rstd, A, dU, psi, loss, dxj, *gU, *gD)]


@pytest.mark.parametrize("mode", NL.MODES)
@pytest.mark.parametrize("bf16_params", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,lead", [(64, 0), (64, 8), (1536, 8)])
def test_stand_ins_stay_inside_the_derived_bounds(D, lead, bf16_params, mode):
    check_kernels(NL.STAND_INS, "cpu", 2, 36, D, lead, bf16_params, mode)


def test_stand_ins_single_partial_tile():
    check_kernels(NL.STAND_INS, "cpu", 1, 3, 64, 8, False, "smooth_l1")


def _standin_chain(h, params, weight, mode):
    """the engine's chain on the stand-ins (engine.NextLatTap with plain tensors): (state, dx [B, S, D] bf16, the six gradients)"""
    from simpletuner_amd.engine import NextLatHead, NextLatTap
    grads = [torch.zeros_like(p) for p in params]
    head = NextLatHead(1, h.shape[-1], list(params), grads, 0, sum(p.numel() for p in params), "cpu")
    tap = NextLatTap(head, mode)
    tap.tap(1, h)
    state = tap.state().clone()
    dx = torch.zeros_like(h)
    tap.backward(torch.tensor(weight), dx)
    return state, dx, grads


@pytest.mark.parametrize("mode", NL.MODES)
def test_stand_ins_reproduce_the_executed_reference_end_to_end(monkeypatch, golden, mode):
    """unchained: the bf16 chain from the fixture's fp32 inputs against the executed reference — the state loss within 1 %, the hidden-state gradient and the six
    parameter gradients within 3 % rel-L2 (bf16 xhat, folded weights, U, A, pred, psi, dA, dU, g, P1, P2: eleven roundings of 2^-9 along the longest path)"""
    NL.install(monkeypatch)
    g = golden[mode]
    params = [p.clone() for p in _params(golden)]
    state, dx, grads = _standin_chain(g["hidden"].to(BF16), params, g["weight"], mode)
    assert abs(state.item() - g["logs"]["nextlat_state_loss"]) < 1e-2 * g["logs"]["nextlat_state_loss"]
    assert PU.rel_l2(dx, g["grad_hidden"]) < 3e-2 and (dx[:, -1] == 0).all()
    for nm, t in zip(NL.NAMES, grads):
        assert PU.rel_l2(t, g["grads"][nm]) < 3e-2, nm


# ------------------------------------------------------------------------------------------------
# (c) plugin / trainer surface
# ------------------------------------------------------------------------------------------------
def _acc():
    return SimpleNamespace(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
                           backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _plugin(monkeypatch, family="sd3", layers=3, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    NL.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=2, single=2))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(layers))
    return plugin


def _setup(plugin):
    """the trainer's order: the trainable arena first, then post_model_load_setup"""
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    return plugin


def test_post_model_load_setup_accepts_nextlat_for_sd3(monkeypatch, golden):
    """the configuration path (on the parent commit `nextlat_enabled` raises NotImplementedError here)"""
    plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    assert comp._nl_block == 2 == golden["index_table"]["None"] and plugin.nextlat.weight == 0.3 and plugin.nextlat.block_index == 2 and plugin.nextlat.state_loss == "smooth_l1"
    own = dict(comp.named_parameters())
    D = comp.D
    assert [tuple(own[PRE + nm].shape) for nm in NL.NAMES] == [(D,), (D,), (2 * D, D), (2 * D,), (D, 2 * D), (D,)]
    # the reference's initial values: LayerNorm affine (1, 0), `up` inside nn.Linear's default bound and not zero, `down` zero
    assert (own[PRE + "norm.weight"] == 1).all() and (own[PRE + "norm.bias"] == 0).all() and (own[PRE + "down.weight"] == 0).all() and (own[PRE + "down.bias"] == 0).all()
    for nm in ("up.weight", "up.bias"):
        assert 0 < own[PRE + nm].abs().max() <= 1 / D ** 0.5 and own[PRE + nm].std() > 0.4 / D ** 0.5
    assert all(own[PRE + nm].requires_grad and own[PRE + nm].dtype == F32 for nm in NL.NAMES)          # LoRA: fp32 masters
    w = own[PRE + "up.weight"].detach()
    assert (w != w.to(BF16).float()).any()                                    # ... drawn in fp32 (not copies of the base arena's bf16 values)
    plugin.freeze_components()
    assert all(own[PRE + nm].requires_grad for nm in NL.NAMES)
    # the reference's index rule through the configuration, and the second loss form
    for configured, want in ((0, 2), (-1, 2), (2, 2), (1, 1)):
        plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.25, nextlat_block_index=configured, nextlat_state_loss="mse")
        plugin.add_lora_adapter(); plugin.post_model_load_setup()
        assert plugin.get_trained_component()._nl_block == want == golden["index_table"][repr(configured)] and plugin.get_trained_component()._nl_mode == "mse"
    e = golden["errors"]
    for kw, text in ((dict(nextlat_weight=-0.5), e["bad_weight"]), (dict(nextlat_weight=0), e["zero_weight"]), (dict(), e["zero_weight"]),
                     (dict(nextlat_weight=0.3, nextlat_state_loss="l1"), e["bad_state_loss"]), (dict(nextlat_weight=0.3, nextlat_kl_weight=-1.0), e["bad_kl"]),
                     (dict(nextlat_weight=0.3, nextlat_kl_weight=0.5), e["kl_no_head"])):
        with pytest.raises(ValueError) as ei:
            _setup(_plugin(monkeypatch, nextlat_enabled=True, **kw))
        assert str(ei.value) == text
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, nextlat_block_index=3)
    assert str(ei.value) == e["index_high"]
    # the reference's order: the weight is checked before the index, the index before the loss form
    ok = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3)
    ok.add_lora_adapter()
    ok.config.nextlat_block_index, ok.config.nextlat_state_loss = 3, "l1"
    with pytest.raises(ValueError) as ei:
        ok.post_model_load_setup()
    assert str(ei.value) == e["index_high"]
    ok.config.nextlat_weight = 0
    with pytest.raises(ValueError) as ei:
        ok.post_model_load_setup()
    assert str(ei.value) == e["zero_weight"]
    # (the text below is common.py:5203-5206's, typed out: that module does not load on its own, so the fixture cannot record it)
    with pytest.raises(ValueError) as ei:
        _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, lora_type="lycoris").post_model_load_setup()
    assert str(ei.value) == "NextLat requires standard PEFT LoRA or full-model training so its predictor is optimized and saved."
    # off: nothing is laid out, the forward returns one output, auxiliary_loss passes the loss through
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter(); plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    assert plugin.nextlat is None and comp._nl_block is None and comp._nl is None and not any(n.startswith(PRE) for n, _ in comp.named_parameters())
    loss = torch.tensor(1.5)
    assert plugin.auxiliary_loss({"model_prediction": None}, {}, loss) == (loss, None)


def test_refusals_by_name(monkeypatch, golden):
    from simpletuner_amd.sdxl.model import SDXL
    from simpletuner_amd.training.trainer import Trainer
    from tests import test_unet_host_sequencing_cpu as UH
    with pytest.raises(NotImplementedError, match="nextlat_enabled.*built: SD3"):          # Flux: the follow-up
        _plugin(monkeypatch, "flux", nextlat_enabled=True, nextlat_weight=0.3).post_model_load_setup()
    from simpletuner_amd.pixart.model import PixartSigma
    from simpletuner_amd.pixart.transformer import PixArtTransformer2DModel
    from tests import test_pixart_host_sequencing_cpu as PH
    pix = PixartSigma.__new__(PixartSigma)
    pix.config, pix.accelerator, pix.model, pix.controlnet = SimpleNamespace(nextlat_enabled=True, nextlat_weight=0.3), _acc(), PixArtTransformer2DModel(device="cpu", **PH.ARCH), None
    with pytest.raises(NotImplementedError, match="nextlat_enabled.*built: SD3"):
        pix.post_model_load_setup()
    unet, _ = UH._unet(monkeypatch, "sdxl_small", 3)
    plug = SDXL.__new__(SDXL)
    plug.config, plug.accelerator, plug.model, plug.controlnet = SimpleNamespace(nextlat_enabled=True, nextlat_weight=0.3), _acc(), unet, None
    with pytest.raises(ValueError) as ei:
        plug.post_model_load_setup()
    assert str(ei.value) == "NextLat is only supported for transformer model families."          # common.py:5201-5202
    for flag in ("crepa_enabled", "irepa_enabled", "urepa_enabled"):
        with pytest.raises(NotImplementedError, match=flag):
            _plugin(monkeypatch, **{flag: True}).post_model_load_setup()
    with pytest.raises(NotImplementedError, match="Internal Guidance together with NextLat"):
        _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, internal_guidance_enabled=True).post_model_load_setup()
    # an ordering requirement of this path: set-up follows the lay-out of the arena that trains
    with pytest.raises(NotImplementedError, match="nextlat_enabled: post_model_load_setup while the component has no trainable arena"):
        _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3).post_model_load_setup()
    routes = {"routes": [{"selection_ratio": 0.5, "start_layer_idx": 1, "end_layer_idx": 2}]}
    with pytest.raises(NotImplementedError, match="nextlat_enabled with TREAD routing"):
        _setup(_plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, tread_config=routes))
    plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3)
    plugin.xm_config = SimpleNamespace(enabled=True)
    plugin.add_lora_adapter()
    with pytest.raises(NotImplementedError, match="nextlat_enabled with XM noise candidates"):
        plugin.post_model_load_setup()
    plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3)
    plugin.add_lora_adapter(); plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    comp.set_router(object(), routes["routes"])          # a router handed to the component directly: refused by the engine at the training forward
    d = SH._inputs(2, 16, 24, 33)
    with pytest.raises(NotImplementedError, match="NextLat under TREAD routing"):
        comp(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"])
    for kw, text in ((dict(hip_graph=True), "hip_graph: NextLat"), (dict(optimizer="muon"), "optimizer 'muon' with nextlat_enabled.*st355-adamw"),
                     (dict(optimizer="soap"), "optimizer 'soap' with nextlat_enabled.*optimi-lion")):
        plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.3, **kw)
        plugin.SUPPORTS_MUON_CLIP = True
        plugin.add_lora_adapter()
        with pytest.raises(NotImplementedError, match=text):
            Trainer(plugin.config, plugin, plugin.accelerator)
    # a predictor cannot join arenas that are already laid out; the two heads exclude each other at the component too
    plugin = _plugin(monkeypatch)
    plugin.add_lora_adapter()
    with pytest.raises(RuntimeError, match="before add_lora_adapter"):
        plugin.get_trained_component().set_nextlat(1)
    from simpletuner_amd.sd3 import transformer as T
    with pytest.raises(NotImplementedError, match="Internal Guidance together with NextLat"):
        T.SD3Transformer2DModel(device="cpu", internal_guidance_block_index=1, nextlat_block_index=1, **SH._arch(3))
    with pytest.raises(ValueError) as ei:
        T.SD3Transformer2DModel(device="cpu", **SH._arch(3)).set_nextlat(1, "l1")
    assert str(ei.value) == golden["errors"]["bad_state_loss"]


# ------------------------------------------------------------------------------------------------
# (d) host sequencing: loss and every trainable gradient against autograd through the oracle
# ------------------------------------------------------------------------------------------------
def _set_ckpt(model, mode):
    if mode != "plain":
        model.enable_gradient_checkpointing()
    if mode == "segmented":
        model.set_gradient_checkpointing_interval(2)


def sd3_model(install, monkeypatch, layers, block, full, dev="cpu", arch=SH._arch, mode="smooth_l1", seed=11):
    """tests/test_sd3_host_sequencing_cpu.py::_model with the predictor laid out (its values seeded: the reference's zero `down` would hide the injection).  `block` is
    the tap's block itself: the reference's index rule cannot name block 0 (a configured 0 means the last block), so the tap is moved there by hand."""
    if install is not None:
        install(monkeypatch)
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device=dev, nextlat_block_index=-1, **arch(layers))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith(PRE):
                continue
            if name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
        c = model.config
        model.pos_embed.pos_embed.copy_(T.sincos_2d(model.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None])
    assert model._nl_block == layers - 1
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    model.set_nextlat(block if block else None, mode)
    if block == 0:
        model._nl_block = model._nl.block = 0
    assert model._nl_block == block == model._nl.block
    NL.seed_predictor(model)
    return model


def hip_side(model, d, weight, lam=None):
    res = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=True)
    out, state = res.sample, res.nextlat_state_loss
    assert state.dim() == 0 and state.dtype == F32 and state.requires_grad
    loss = ((out.float() - d["target"].float()) ** 2).mean() + weight * state
    if lam is not None:
        loss = loss - lam * res.layersync_similarity
    loss.backward()
    return out.detach(), loss.detach(), state.detach()


def head_rel(model, head):
    """worst rel-L2 / cosine of the six predictor gradients against the oracle's"""
    own = dict(model.named_parameters())
    worst_r, worst_c = 0.0, 1.0
    for nm in NL.NAMES:
        p, ref = own[PRE + nm], head[PRE + nm].grad
        assert p.grad is not None and ref.norm() > 0, nm
        worst_r, worst_c = max(worst_r, PU.rel_l2(p.grad, ref)), min(worst_c, PU.cos_sim(p.grad, ref))
    return worst_r, worst_c


def _check(model, out, loss, state, oracle, full):
    o_out, o_loss, o_state, P, lp, share, head = oracle
    assert PU.rel_l2(out, o_out) < 2e-2 and abs(loss.item() - o_loss.item()) < 2e-3 * max(1.0, abs(o_loss.item()))
    assert abs(state.item() - o_state.item()) < 1e-2 * abs(o_state.item())
    assert share >= 0.1, share          # dropping the injection would miss the gradient tolerances by a wide margin
    if full:
        LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",))          # (walks the predictor's six tensors too)
    else:
        LS.check_lora_grads(model, lp, 5e-2)
    rg, cg = head_rel(model, head)
    assert rg < 6e-2 and cg > 0.998, f"predictor gradients: rel={rg:.3e} cos={cg:.5f}"          # the form of layersync_ref.check_full_grads
    return share, rg


@pytest.mark.parametrize("ckpt", ["plain", "per-block", "segmented"])
@pytest.mark.parametrize("block", [0, 1, 2])          # 3 joint blocks (the last is context_pre_only)
@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_with_nextlat_matches_autograd_through_the_oracle(monkeypatch, full, block, ckpt):
    model = sd3_model(NL.install, monkeypatch, 3, block, full)
    _set_ckpt(model, ckpt)
    d = SH._inputs(2, 16, 24, 33)
    out, loss, state = hip_side(model, d, WEIGHT)
    _, lora, scale = PU.oracle_state(model)
    oracle = NL.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, block, WEIGHT, full, None if full else lora, scale)
    share, rg = _check(model, out, loss, state, oracle, full)
    print(f"[emu] sd3 nextlat {'full' if full else 'lora'} block {block} {ckpt}: regulariser share of the trunk gradient={share:.3e}, predictor gradients rel-L2={rg:.3e}")


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_at_the_gpu_test_shapes_measures_the_predictor_gradient_error(monkeypatch, full):
    """The figure tests/test_nextlat_gpu.py doubles for its tolerance: the worst rel-L2 of the six predictor gradients, stand-ins against the oracle, at that test's
    model, inputs, block, weight and loss forms (P1 and P2 are bf16 here, where Internal Guidance's P is fp32).  Measured: LoRA 4.02e-3 (smooth-L1) / 3.96e-3 (MSE),
    full fine-tune 3.96e-3 / 3.95e-3; HEAD_REL_CPU is their worst, rounded up."""
    for mode in NL.MODES:
        model = sd3_model(NL.install, monkeypatch, 3, 1, full, mode=mode)
        d = SH._inputs(2, 16, 24, 33)
        out, loss, state = hip_side(model, d, WEIGHT)
        _, lora, scale = PU.oracle_state(model)
        oracle = NL.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, 1, WEIGHT, full, None if full else lora, scale, mode=mode)
        rg, cg = head_rel(model, oracle[-1])
        print(f"[emu] sd3 nextlat {'full' if full else 'lora'} {mode}: predictor gradients worst rel-L2={rg:.3e} cos={cg:.6f}")
        assert rg <= HEAD_REL_CPU


HEAD_REL_CPU = 4.1e-3


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_engine_with_nextlat_and_layersync_together(monkeypatch, full):
    """outputs in the order (out, sim, nextlat_state); both gradients enter the dX chain at their blocks"""
    model = sd3_model(NL.install, monkeypatch, 3, 1, full)
    model.set_layersync(0, 2)
    d = SH._inputs(2, 16, 24, 33)
    tup = model(hidden_states=d["lat"], encoder_hidden_states=d["prompt"], pooled_projections=d["pooled"], timestep=d["t"], return_dict=False)
    assert len(tup) == 3 and tup[1].dim() == 0 and tup[2].dim() == 0
    out, loss, state = hip_side(model, d, WEIGHT, lam=8.0)
    assert not torch.equal(tup[1].detach(), tup[2].detach())
    _, lora, scale = PU.oracle_state(model)
    oracle = NL.sd3_oracle(monkeypatch, model, SH._ocfg(model), d, 1, WEIGHT, full, None if full else lora, scale, layersync=(0, 2, 8.0))
    _check(model, out, loss, state, oracle, full)


def test_gradient_accumulation_adds_the_predictor_gradients(monkeypatch):
    """LoRA, two micro-steps with accumulate_lora_grads: the predictor's gradient views hold the sum, like the adapters'"""
    model = sd3_model(NL.install, monkeypatch, 3, 1, False)
    d1, d2 = SH._inputs(2, 16, 24, 33, seed=5), SH._inputs(2, 16, 24, 33, seed=6)
    own = dict(model.named_parameters())
    singles = []
    for d in (d1, d2):
        hip_side(model, d, WEIGHT)
        singles.append([own[PRE + nm].grad.clone() for nm in NL.NAMES])
        for p in model.parameters():
            p.grad = None
    hip_side(model, d1, WEIGHT)
    model.accumulate_lora_grads = True
    for p in model.parameters():
        p.grad = None                            # the engine's flat gradient arena keeps the first micro-step's values
    hip_side(model, d2, WEIGHT)
    for nm, a, b in zip(NL.NAMES, *singles):
        assert torch.allclose(own[PRE + nm].grad, a + b, rtol=1e-5, atol=1e-7 * (a + b).abs().max().item()), nm


def test_tap_below_the_first_trained_block_fills_only_the_predictor_gradients(monkeypatch, golden):
    """backward(d_state, None): no dX accumulation, the predictor's gradients as with it; d_state None: zeros unless accumulating; fewer than two tokens refused"""
    from simpletuner_amd.engine import NextLatHead, NextLatTap
    NL.install(monkeypatch)
    g = torch.Generator().manual_seed(2)
    B, S, D = 2, 35, 64
    params = [p.clone() for p in _params(golden)]
    joint = torch.randn(B, S + 8, D, generator=g).to(BF16)
    outs = []
    for with_dx in (True, False):
        grads = [torch.zeros_like(p) for p in params]
        ready = []
        head = NextLatHead(1, D, params, grads, 128, 128 + sum(p.numel() for p in params), "cpu")
        tap = NextLatTap(head)
        tap.tap(0, joint[:, 8:])
        assert tap.state_loss is None                      # only at its block
        with pytest.raises(RuntimeError, match="never reached"):
            tap.state()
        tap.tap(1, joint[:, 8:])
        assert tap.state().dim() == 0 and tap.state().item() > 0
        dx = torch.zeros(B, S, D, dtype=BF16)
        tap.backward(torch.tensor(0.3), dx if with_dx else None, False, SimpleNamespace(ready=lambda lo, hi: ready.append((lo, hi))))
        assert ready == [(head.flat_lo, head.flat_hi)] and (dx[:, :-1].abs().max() > 0) == with_dx and (dx[:, -1] == 0).all() and all(t.abs().max() > 0 for t in grads)
        outs.append(grads)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    grads = outs[-1]
    tap = NextLatTap(head)
    tap.tap(1, joint[:, 8:])
    keep = [t.clone() for t in grads]
    tap.backward(None, None, True)
    assert all(torch.equal(a, b) for a, b in zip(keep, head.grads))
    tap.tap(1, joint[:, 8:])
    tap.backward(None, None, False)
    assert all((t == 0).all() for t in head.grads)
    with pytest.raises(ValueError) as ei:
        NextLatTap(head).tap(1, joint[:, 8:9])
    assert str(ei.value) == golden["errors"]["one_token"]


# ------------------------------------------------------------------------------------------------
# (e) arena invariants: one run for the optimizer, EMA, clipping
# ------------------------------------------------------------------------------------------------
def _trainer(monkeypatch, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, nextlat_enabled=True, nextlat_weight=0.5, nextlat_block_index=1, lora_rank=8, lora_init_b_std=0.02, **cfg_kw)
    if plugin.config.model_type == "lora":
        plugin.add_lora_adapter()
    else:
        plugin.freeze_components()
    plugin.post_model_load_setup()
    NL.seed_predictor(plugin.get_trained_component())
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    return plugin, trainer, batch


@pytest.mark.parametrize("model_type", ["lora", "full"])
def test_trainable_parameters_and_gradients_stay_one_run_with_the_predictor(monkeypatch, model_type):
    from simpletuner_amd.training.optimizer import flat_view
    plugin, trainer, batch = _trainer(monkeypatch, model_type=model_type)
    comp = plugin.get_trained_component()
    params = comp.trainable_parameters()
    own = dict(comp.named_parameters())
    head = [own[PRE + nm] for nm in NL.NAMES]
    assert all(any(p is h for p in params) for h in head)
    assert all(h.data_ptr() % 16 == 0 for h in head)                          # the kernels move 8 elements per lane
    flat = flat_view([p.data for p in params])
    assert flat is not None and flat.numel() >= sum(p.numel() for p in params)
    assert flat.dtype == (F32 if model_type == "lora" else BF16) and head[0].dtype == flat.dtype
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    total, logs = plugin.auxiliary_loss(pred, prepared, trainer.model.loss_with_logs(prepared, pred)[0])
    total.backward()
    gflat = flat_view([p.grad for p in params])
    assert gflat is not None and all(h.grad is not None and h.grad.abs().max() > 0 for h in head)


def test_train_step_adds_the_regulariser_keeps_its_logs_and_moves_the_predictor(monkeypatch, golden):
    """Trainer.train_step (st355-adamw): loss = mse + weight * state, the logs as floats in `last_aux_logs`, merged with LayerSync's when both are on — NextLat's
    entries before LayerSync's, the reference's order"""
    plugin, trainer, batch = _trainer(monkeypatch, learning_rate=1e-3, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=3,
                                      use_ema=True, ema_decay=0.9, max_grad_norm=0.05)
    comp = plugin.get_trained_component()
    own = dict(comp.named_parameters())
    before = [own[PRE + nm].detach().clone() for nm in NL.NAMES]
    prepared = plugin.prepare_batch(dict(batch), {"global_step": 0})
    pred = plugin.model_predict(prepared)
    mse, _ = plugin.loss_with_logs(prepared, pred)
    total, logs = plugin.auxiliary_loss(pred, prepared, mse)
    assert list(logs) == ["nextlat_loss", "nextlat_state_loss", "layersync_loss", "layersync_similarity"] and all(isinstance(v, float) for v in logs.values())
    state = pred["nextlat_state_loss"]
    assert logs["nextlat_state_loss"] == state.item() and abs(logs["nextlat_loss"] - 0.5 * state.item()) < 1e-7
    assert abs(total.item() - (mse.item() + 0.5 * state.item() + logs["layersync_loss"])) < 1e-5
    total.backward()
    params = comp.trainable_parameters()
    sq = lambda ps: sum(p.grad.double().pow(2).sum().item() for p in ps) ** 0.5
    norm_all, norm_adapters = sq(params), sq([p for n, p in comp.named_parameters() if ".lora_" in n])
    assert norm_all > 1.01 * norm_adapters                                                              # the predictor's share is visible in the norm
    for p in params:
        p.grad = None
    loss = trainer.train_step(dict(batch))
    assert abs(loss.item() - total.item()) < 1e-5 and trainer.last_aux_logs == logs
    assert all(not torch.equal(own[PRE + nm].detach(), b) for nm, b in zip(NL.NAMES, before))          # AdamW moved all six
    assert float(trainer.last_grad_norm) > 0.05 and abs(float(trainer.last_grad_norm) - norm_all) <= 1e-4 * norm_all          # the on-device norm covers the predictor's range
    sh = getattr(trainer.ema_model, "shadow_flat", None)
    assert sh is not None                         # the trainables are still ONE run: the EMA keeps its flat shadow, which covers the predictor's range and lags it
    lo, hi = comp._nl.flat_lo, comp._nl.flat_hi
    cur = comp.lora_flat[lo:hi]
    assert sh.numel() >= hi and 0 < (sh[lo:hi].float() - cur).abs().max().item() < (torch.cat([b.reshape(-1) for b in before]) - cur).abs().max().item()
    with torch.no_grad():          # a prediction outside training carries no state loss: the regulariser cannot be evaluated on it
        with pytest.raises(ValueError) as ei:
            plugin.auxiliary_loss(plugin.model_predict(prepared), prepared, mse)
        assert str(ei.value) == golden["errors"]["no_buffer"]


@pytest.mark.parametrize("opt", ["adamw_bf16", "optimi-lion"])
@pytest.mark.parametrize("model_type", ["lora", "full"])
def test_the_other_one_launch_optimizers_move_the_predictor(monkeypatch, model_type, opt):
    from tests import lion_bounds as LB
    # (full fine-tune under Lion: every step moves a bf16 parameter by lr exactly, Kahan-compensated — 1e-2 so that two steps pass the bf16 ulp of gamma ~ 1, 2^-7)
    lr = 1e-3 if model_type == "lora" else (1e-2 if opt == "optimi-lion" else 1e-4)
    plugin, trainer, batch = _trainer(monkeypatch, model_type=model_type, optimizer=opt, learning_rate=lr)
    LB.install(monkeypatch)                       # (the emulated ops.lion_step)
    own = dict(plugin.get_trained_component().named_parameters())
    before = [own[PRE + nm].detach().clone() for nm in NL.NAMES]
    for _ in range(2):
        trainer.train_step(dict(batch))
    moved = [not torch.equal(own[PRE + nm].detach(), b) for nm, b in zip(NL.NAMES, before)]
    assert all(moved), dict(zip(NL.NAMES, moved))


# ------------------------------------------------------------------------------------------------
# (f) files
# ------------------------------------------------------------------------------------------------
def test_lora_file_round_trip_carries_the_predictor(monkeypatch, golden, tmp_path):
    from safetensors.torch import load_file
    plugin, _, _ = _trainer(monkeypatch)
    comp = plugin.get_trained_component()
    vals = {n: p.detach().clone() for n, p in comp.named_parameters() if n.startswith(PRE)}
    path = plugin.save_lora_weights(str(tmp_path))
    flat = load_file(path)
    keys = sorted(k for k in flat if "nextlat_predictor" in k)
    # the module's own state-dict keys under `transformer.nextlat_predictor.` (seven entries; the layout is not pinned against peft's modules_to_save)
    assert keys == sorted("transformer." + PRE + s for s in golden["state_keys"]["keys"]) and len(keys) == 7
    bi = flat["transformer." + PRE + "block_index"]
    assert bi.dtype == torch.int64 and bi.dim() == 0 and bi.item() == 1
    adapter_dtype = next(v.dtype for k, v in flat.items() if ".lora_A." in k)
    assert all(flat["transformer." + PRE + nm].dtype == adapter_dtype for nm in NL.NAMES)
    with torch.no_grad():
        for n, p in comp.named_parameters():
            if n.startswith(PRE) or ".lora_" in n:
                p.add_(0.5)
    plugin.load_lora_weights(input_dir=str(tmp_path))
    for n, p in comp.named_parameters():
        if n.startswith(PRE):
            assert torch.equal(p.detach(), vals[n]), n
    # strict: a file with a predictor, none configured
    plain = _plugin(monkeypatch, lora_rank=8)
    plain.add_lora_adapter(); plain.post_model_load_setup()
    with pytest.raises(ValueError, match="carries a NextLat predictor"):
        plain.load_lora_weights(input_dir=str(tmp_path))
    # ... a ComfyUI-dialect file into a component with a predictor: refused (that dialect cannot carry it; it would silently keep its initial values)
    plugin.config.lora_format = "comfyui"
    plugin.save_lora_weights(str(tmp_path / "comfy_in"))
    with pytest.raises(ValueError, match="ComfyUI-format LoRA file cannot carry the NextLat predictor"):
        plugin.load_lora_weights(input_dir=str(tmp_path / "comfy_in"))
    plugin.config.lora_format = None
    # ... a predictor configured, a file without one; a file from another block
    plain.save_lora_weights(str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="block index"):
        plugin.load_lora_weights(input_dir=str(tmp_path / "plain"))
    comp.set_nextlat(2)
    with pytest.raises(ValueError, match="NextLat predictor was trained on block 1"):
        plugin.load_lora_weights(input_dir=str(tmp_path))
    comp.set_nextlat(1)
    # the ComfyUI export drops the predictor
    plugin.config.lora_format = "comfyui"
    assert not any("nextlat" in k for k in load_file(plugin.save_lora_weights(str(tmp_path / "comfy"))))


def test_full_checkpoint_carries_the_predictor_through_the_parameter_names(monkeypatch):
    model = sd3_model(NL.install, monkeypatch, 2, 1, True)
    sd = model.diffusers_state_dict()
    assert all(PRE + nm in sd and sd[PRE + nm].dtype == BF16 for nm in NL.NAMES)
    other = sd3_model(NL.install, monkeypatch, 2, 1, True, seed=12)
    with torch.no_grad():
        for nm in NL.NAMES:
            dict(other.named_parameters())[PRE + nm].zero_()
    other.load_flat_state(sd)
    assert all(torch.equal(dict(other.named_parameters())[PRE + nm], sd[PRE + nm]) for nm in NL.NAMES)
    # optional in a file: a checkpoint without the predictor loads, and the predictor keeps what it holds
    keep = {nm: dict(other.named_parameters())[PRE + nm].detach().clone() for nm in NL.NAMES}
    other.load_flat_state({k: v for k, v in sd.items() if not k.startswith(PRE)})
    assert all(torch.equal(dict(other.named_parameters())[PRE + nm], keep[nm]) for nm in NL.NAMES)


def test_set_nextlat_before_the_adapters_lays_the_predictor_out_with_the_reference_initial_values(monkeypatch):
    """a component constructed without `nextlat_block_index`: set_nextlat before add_lora_adapter puts the fp32 masters behind the adapters (NextLatHead.init_reference)"""
    NL.install(monkeypatch)
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device="cpu", **SH._arch(3))
    model.set_nextlat(1, "mse")
    model.add_lora_adapter(rank=8)
    own, D = dict(model.named_parameters()), model.D
    assert model._nl.block == 1 and model._nl_mode == "mse" and model._nl.flat_lo % 8 == 0 and model._nl.flat_hi <= model.lora_flat.numel()
    assert (own[PRE + "norm.weight"] == 1).all() and (own[PRE + "norm.bias"] == 0).all() and (own[PRE + "down.weight"] == 0).all() and (own[PRE + "down.bias"] == 0).all()
    for nm in ("up.weight", "up.bias"):
        assert 0 < own[PRE + nm].abs().max() <= 1 / D ** 0.5 and own[PRE + nm].std() > 0.4 / D ** 0.5
    assert all(own[PRE + nm].data_ptr() % 16 == 0 and own[PRE + nm].dtype == F32 for nm in NL.NAMES)


def test_a_predictor_that_came_with_the_loaded_weights_starts_the_lora_masters(monkeypatch):
    """load_flat_state with `nextlat_predictor.*` in the file, then add_lora_adapter: the fp32 masters start from the file's values, not from a fresh draw"""
    src = sd3_model(NL.install, monkeypatch, 2, 1, True)
    sd = src.diffusers_state_dict()
    from simpletuner_amd.sd3 import transformer as T
    model = T.SD3Transformer2DModel(device="cpu", nextlat_block_index=1, **SH._arch(2))
    model.load_flat_state(sd)
    model.add_lora_adapter(rank=8)
    own = dict(model.named_parameters())
    assert all(own[PRE + nm].dtype == F32 and torch.equal(own[PRE + nm].detach(), sd[PRE + nm].float()) for nm in NL.NAMES)
    fresh = T.SD3Transformer2DModel(device="cpu", nextlat_block_index=1, **SH._arch(2))
    fresh.load_flat_state({k: v for k, v in sd.items() if not k.startswith(PRE)})
    fresh.add_lora_adapter(rank=8)
    assert (dict(fresh.named_parameters())[PRE + "down.weight"] == 0).all()          # no predictor in the file: the reference's initial values

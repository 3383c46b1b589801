"""Flow-DPO (`distillation_method=flow_dpo`) on the CPU: the fp64 restatement (tests/flow_dpo_ref.py) held to the EXECUTED reference distiller
(tests/golden/flow_dpo_vectors.pt, tools/gen_flow_dpo_golden.py) within bounds derived from fp32 summation, the closed forms held to autograd, the stand-ins
inside the kernels' bounds (tests/flow_dpo_bounds.py), why the margin is accumulated element by element, the host logic of simpletuner_amd/flow_dpo.py (config,
batch contract, refusals, dropout override), adapters off, and the tiny Flux / SD3 engines and the Trainer on the emulator against the oracle."""
import importlib.util
import logging
import os
from types import SimpleNamespace

import pytest
import torch

from oracle import flux as OF
from oracle import sd3 as OS
from tests import flow_dpo_bounds as FB
from tests import flow_dpo_ref as FR
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_scheduled_sampling_cpu import _acc, _capture_grads, _compare_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
U = FB.U


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(ROOT, "tests", "golden", "flow_dpo_vectors.pt"), weights_only=False)


# ------------------------------------------------------------------------------------------------
# (a) the restatement against the executed reference
# ------------------------------------------------------------------------------------------------
def _restate_case(case, shape):
    """the fp64 restatement over the calls of one recorded case (the EMA carried from call to call), with the bounds that hold the reference's fp32 values to it:
    every per-sample error is an fp32 sum of n terms of at most 4 roundings each — gamma(n + 4) E — and everything downstream is Lipschitz in the margins"""
    B, C, H, W = shape
    n = C * H * W
    cfg = {**FR_DEFAULTS, **{k: v for k, v in case["config"].items() if k != "mask"}}
    gam = FB.gamma(n + 4)
    ema, e_ema, out = None, 0.0, []
    for rec in case["calls"]:
        fl = lambda t, rows=B: t.to(F64).reshape(rows, -1)
        pol = torch.cat([fl(rec["policy_win"]), fl(rec["policy_lose"])]).requires_grad_(True)
        ref = torch.cat([fl(rec["ref_win"]), fl(rec["ref_lose"])])
        tw, tl = fl(rec["target_win"]), fl(rec["target_lose"])
        mask = None if rec["mask"] is None else fl(rec["mask"]).repeat(1, C)
        orig = rec["original_loss"].to(F64).clone().requires_grad_(True)
        m1 = torch.ones_like(tw) if mask is None else mask
        nu = FR.nu_of(cfg["norm_type"], n, None if mask is None else mask.sum(1)) * torch.ones(B, dtype=F64)
        errs = [nu * (m1 * (a - b) ** 2).sum(1) for a, b in ((pol[:B], tw), (pol[B:], tl), (ref[:B], tw), (ref[B:], tl))]
        e_m = ((gam + 3 * U) * sum(e.detach() for e in errs))
        _, margin = FR.loss64(pol, ref, tw, tl, mask, cfg["norm_type"])
        beta, e_beta = float(cfg["beta"]), 0.0
        target_gf = float(cfg["auto_beta_target_gf"] or 0.0)
        if cfg["auto_beta"] and target_gf > 0:
            am, e_am = float(margin.detach().abs().mean()), float(e_m.mean()) + 2 * U * float(margin.detach().abs().mean())
            d = float(cfg["auto_beta_decay"])
            ema, e_ema = (am, e_am) if ema is None else (d * ema + (1 - d) * am, d * e_ema + (1 - d) * e_am)
            eps = float(cfg["auto_beta_eps"])
            raw = FR.auto_num(target_gf, eps) / max(ema, eps)
            beta = raw
            if cfg["auto_beta_min"] is not None:
                beta = max(float(cfg["auto_beta_min"]), beta)
            if cfg["auto_beta_max"] is not None:
                beta = min(float(cfg["auto_beta_max"]), beta)
            e_beta = raw * (e_ema / max(ema, eps) + 8 * U)          # (the clamps are 1-Lipschitz; torch.logit of an fp32 tensor: a few u)
        loss, margin = FR.loss64(pol, ref, tw, tl, mask, cfg["norm_type"], beta, float(cfg["loss_weight"]), float(cfg["anchor_alpha"]), float(cfg["sft_loss_weight"]), orig)
        g_pol, = torch.autograd.grad(loss, [pol], retain_graph=True)
        mg = margin.detach()
        e_logit = 0.5 * (beta * e_m + mg.abs() * e_beta) + 2 * U * (0.5 * beta * mg).abs()
        lw, aa, sw = abs(float(cfg["loss_weight"])), float(cfg["anchor_alpha"]), float(cfg["sft_loss_weight"])
        anchor = 0.5 * aa * (((pol[:B] - ref[:B]) ** 2).mean() + ((pol[B:] - ref[B:]) ** 2).mean()).detach()
        e_dpo = float(e_logit.mean()) + 8 * U * float(torch.nn.functional.softplus(-0.5 * beta * mg).mean())
        e_loss = lw * e_dpo + float(FB.gamma(2 * n + 8) * anchor.abs()) + 4 * U * abs(sw * float(orig.detach())) + 4 * U * float(loss.detach().abs())
        # the gradient: coefficient c = lw beta sigma(-logit) / (2 B) per pair (|d sigma| <= e_logit / 4), times 2 nu m (p - t); anchor and element-wise roundings 8 u
        sn = torch.sigmoid(-0.5 * beta * mg)
        rel_c = (e_logit / 4) / sn + (e_beta / beta if beta else 0.0) + 8 * U
        g_anchor = aa / (B * n) * (pol - ref).detach()
        e_g = (g_pol - g_anchor).abs() * torch.cat([rel_c, rel_c]).reshape(2 * B, 1) + 8 * U * g_anchor.abs() + 1e-30
        out.append(dict(loss=loss.detach(), e_loss=e_loss, g_pol=g_pol, e_g=e_g, margin=mg, e_m=e_m, beta=beta, e_beta=e_beta, errs=[e.detach() for e in errs],
                        e_logit=e_logit, sn=sn, anchor=anchor, ema=ema, e_ema=e_ema, e_dpo=e_dpo, gam=gam, logit=0.5 * beta * mg,
                        g_orig=torch.autograd.grad(loss, [orig], allow_unused=True)[0]))
    return out


FR_DEFAULTS = {"beta": 1.0, "loss_weight": 1.0, "sft_loss_weight": 0.0, "anchor_alpha": 0.0, "norm_type": "sum", "mask_dilate": 0, "auto_beta": True,
               "auto_beta_target_gf": 0.2, "auto_beta_decay": 0.99, "auto_beta_min": 1e-3, "auto_beta_max": 1.0, "auto_beta_eps": 1e-6}


def test_defaults_and_method_config_equal_the_executed_reference(G):
    from simpletuner_amd import flow_dpo as FD
    assert FD.DEFAULTS == G["defaults"]
    assert {k: v for k, v in G["defaults"].items() if k != "distillation_type"} == FR_DEFAULTS
    for cfg, want in G["method_config"]:
        assert FD.method_config(cfg) == want, cfg
        assert FD.method_config(SimpleNamespace(**cfg)) == want
    merged = FD.merged_config({"distillation_config": {"flow_dpo": {"beta": 4.0}}})
    assert merged["beta"] == 4.0 and merged["norm_type"] == "sum" and merged["auto_beta_target_gf"] == 0.2


def test_restatement_equals_the_executed_reference_within_the_fp32_summation_bound(G):
    """loss, the twelve logs (+ the anchor's) and d loss / d prediction of both halves for every recorded case and call; zero undecided margins"""
    worst = 0.0
    for ci, case in enumerate(G["cases"]):
        res = _restate_case(case, G["shape"])
        B = G["shape"][0]
        for k, (rec, r) in enumerate(zip(case["calls"], res)):
            tag = (ci, k, case["config"])
            assert bool((r["margin"].abs() > r["e_m"]).all()), tag          # the input condition
            chk = lambda got, want, tol, name: _close(got, want, tol, tag + (name,))
            worst = max(worst, chk(rec["loss"], r["loss"], r["e_loss"], "loss"))
            g_ref = torch.cat([rec["grad_win"].reshape(B, -1), rec["grad_lose"].reshape(B, -1)]).to(F64)
            worst = max(worst, chk(g_ref, r["g_pol"], r["e_g"], "grad"))
            if r["g_orig"] is not None:
                assert abs(float(rec["grad_original"]) - float(r["g_orig"])) <= 2 * U * abs(float(r["g_orig"]))
            else:
                assert rec["grad_original"] is None
            L = rec["logs"]
            pw, pl, rw, rl = r["errs"]
            e_err = lambda e: float((r["gam"] + 2 * U) * e.mean()) + 1e-30
            chk(L["flow_dpo_loss"], -torch.nn.functional.logsigmoid(r["logit"]).mean(), r["e_dpo"], "dpo")
            chk(L["flow_dpo_beta"], r["beta"], r["e_beta"] + U * abs(r["beta"]), "beta")
            chk(L["flow_dpo_margin"], r["margin"].mean(), float(r["e_m"].mean()), "margin")
            chk(L["flow_dpo_win_adv"], (rw - pw).mean(), e_err(rw + pw), "win_adv")
            chk(L["flow_dpo_lose_adv"], (pl - rl).mean(), e_err(pl + rl), "lose_adv")
            for name, e in (("policy_win", pw), ("policy_lose", pl), ("ref_win", rw), ("ref_lose", rl)):
                chk(L[f"flow_dpo_{name}_err"], e.mean(), e_err(e), name)
            assert L["flow_dpo_negative_margin_pct"] == float((r["margin"] < 0).double().mean() * 100.0), tag
            chk(L["flow_dpo_gradient_factor"], r["sn"].mean(), float(r["e_logit"].mean()) / 4 + 4 * U, "gf")
            chk(L["total"], r["loss"], r["e_loss"], "total")
            assert ("flow_dpo_anchor_loss" in L) == (float(case["config"]["anchor_alpha"]) != 0.0)
            if "flow_dpo_anchor_loss" in L:
                chk(L["flow_dpo_anchor_loss"], r["anchor"], float(FB.gamma(2 * r["g_pol"].shape[1] + 8) * r["anchor"].abs()), "anchor")
            if rec["margin_ema"] is not None:
                chk(rec["margin_ema"], r["ema"], r["e_ema"], "ema")
    print(f"[golden] worst |restatement - reference| / bound over loss and gradients = {worst:.3f}")


def _close(got, want, tol, tag):
    got = torch.as_tensor(got, dtype=F64).reshape(-1)
    want = torch.as_tensor(want, dtype=F64).reshape(-1)
    tol = torch.as_tensor(tol, dtype=F64).reshape(-1) + 1e-300
    r = ((got - want).abs() / tol).max().item()
    assert r <= 1.0, (tag, r, got[:3], want[:3])
    return r


def test_mask_and_error_texts_equal_the_executed_reference(G):
    from simpletuner_amd import flow_dpo as FD
    for case in G["cases"]:
        for rec in case["calls"]:
            got = FD.mask_for_loss(rec["batch"], rec["policy_win"].float(), case["config"]["mask_dilate"])
            assert (got is None) == (rec["mask"] is None)
            if got is not None:
                assert got.dtype == F32 and torch.equal(got, rec["mask"]) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    E = G["errors"]
    B, C, H, W = G["shape"]
    good = dict(G["cases"][0]["calls"][0]["batch"])

    def err(edit, fn):
        b = dict(good)
        edit(b)
        with pytest.raises(ValueError) as ei:
            fn(b)
        return str(ei.value)

    def whole(b):
        FD.validate_batch(b)
        lose = FD.conditioning_latents(b)
        if lose.shape != b["latents"].shape:
            raise ValueError(f"Flow-DPO rejected latents must match preferred latents. Got {lose.shape} vs {b['latents'].shape}.")
    assert err(lambda b: b.update(conditioning_type="mask"), whole) == E["conditioning_type"]
    assert err(lambda b: b.update(conditioning_latents=None), whole) == E["conditioning_latents"]
    assert err(lambda b: (b.pop("sigmas"), b.pop("input_noise")), whole) == E["missing"]
    assert err(lambda b: b.update(conditioning_latents=[b["latents"], b["latents"]], conditioning_latents_type=["a", "b"]), whole) == E["list"]
    assert err(lambda b: b.update(conditioning_latents=["x"]), whole) == E["tensor"]
    b = dict(good, conditioning_latents=[good["latents"], good["conditioning_latents"]], conditioning_latents_type=["other", "reference_strict"])
    assert FD.conditioning_latents(b) is good["conditioning_latents"]
    # the shape text through the distiller itself
    model = _stub_model()
    d = FD.FlowDPODistiller(model)
    with pytest.raises(ValueError) as ei:
        d.prepare_batch(dict(good, conditioning_latents=good["latents"][:, :2]))
    assert str(ei.value) == E["shape"]
    # the constructor's texts
    for key, kw in (("norm_type", dict(norm_type="l2")), ("target_gf", dict(auto_beta_target_gf=0.5))):
        with pytest.raises(ValueError) as ei:
            FD.FlowDPODistiller(_stub_model(distillation_config=kw))
        assert str(ei.value) == E[key]
    with pytest.raises(ValueError) as ei:
        FD.FlowDPODistiller(_stub_model(model_type="full"))
    assert str(ei.value) == E["model_type"]
    from simpletuner_amd.foundation import PredictionTypes
    for pt in (PredictionTypes.EPSILON, PredictionTypes.V_PREDICTION):          # PixArt / SDXL / SD 1.5
        with pytest.raises(ValueError) as ei:
            FD.FlowDPODistiller(_stub_model(prediction=pt, hip_graph=True))          # the reference's ValueError fires before any refusal
        assert str(ei.value) == E["flow_matching"]


def _stub_model(prediction=None, **cfg):
    from simpletuner_amd.foundation import PredictionTypes
    base = dict(distillation_method="flow_dpo", model_type="lora", lora_type="standard")
    base.update(cfg)
    return SimpleNamespace(config=SimpleNamespace(**base), PREDICTION_TYPE=prediction or PredictionTypes.FLOW_MATCHING, ROLLOUT_BATCH_KEYS=("encoder_hidden_states",),
                           NAME="stub", accelerator=SimpleNamespace(num_processes=1), xm_config=None)


# ------------------------------------------------------------------------------------------------
# (b) the closed forms, the stand-ins, the margin
# ------------------------------------------------------------------------------------------------
VARIANTS = [dict(norm_type=nt, anchor_alpha=aa, mask=mk) for nt in FR.NORMS for aa in (0.0, 0.5) for mk in (False, True)]


@pytest.mark.parametrize("B,N,period", [(1, 8, None), (3, 1024, 64), (2, 2056, None)])
def test_closed_form_gradient_equals_autograd_and_the_stand_ins_stay_inside_the_bounds(B, N, period):
    for vi, v in enumerate(VARIANTS):
        if v["mask"] and period is None:
            continue
        d = FR.operands(B, N, seed=10 * B + vi, period=period if v["mask"] else None)
        kw = dict(norm_type=v["norm_type"], has_mask=d.emask is not None, beta=FR.f32(0.03 if v["norm_type"] == "sum" else 4.0), loss_weight=FR.f32(0.7),
                  anchor_alpha=FR.f32(v["anchor_alpha"]))
        # closed form (fp64) against autograd on the reference's expression (fp64)
        st = FR.stats64(d.policy, d.ref, d.tw, d.tl, d.emask)
        h = FR.head64(st, N, **kw)
        g = FR.grad64(d.policy, d.ref, d.tw, d.tl, h["pair"], d.emask, kw["anchor_alpha"], 0.5)
        pol = d.policy.double().requires_grad_(True)
        mfull = None if d.emask is None else d.emask.double().repeat(1, N // period)
        loss, margin = FR.loss64(pol, d.ref.double(), d.tw.double(), d.tl.double(), mfull, v["norm_type"], kw["beta"], kw["loss_weight"], kw["anchor_alpha"])
        loss.backward()
        assert torch.allclose(h["loss"], loss.detach(), rtol=1e-12, atol=1e-14) and torch.allclose(h["pair"][:, 0], margin.detach(), rtol=1e-9, atol=1e-12)
        assert torch.allclose(g, 0.5 * pol.grad, rtol=1e-10, atol=1e-16)
        # the stand-ins, op by op inside the kernels' bounds, and every margin decided
        s32 = FR.flow_dpo_stats(d.policy, d.ref, d.tw, d.tl, d.emask)
        ref_s, tol_s = FB.stats_ref(d.policy, d.ref, d.tw, d.tl, d.emask)
        assert FB.inside(s32, ref_s, tol_s)[0]
        assert FB.check_margins(s32, N, v["norm_type"], d.emask is not None)[0]
        loss32, pair32, logs32 = FR.flow_dpo_head(s32, N, **kw)
        hr = FB.head_ref(s32, N, **kw)
        assert FB.inside(loss32, *hr["loss"])[0] and FB.inside(pair32, *hr["pair"])[0] and FB.inside(logs32, *hr["logs"])[0]
        up = torch.tensor([0.25])
        g16 = FR.flow_dpo_grad(d.policy, d.ref, d.tw, d.tl, pair32, d.emask, kw["anchor_alpha"], 2.0, up)
        assert FB.inside(g16, *FB.grad_ref(d.policy, d.ref, d.tw, d.tl, pair32, d.emask, kw["anchor_alpha"], 0.5))[0]
        assert g16.dtype == torch.bfloat16 and g16.shape == d.policy.shape


def test_the_element_wise_margin_holds_where_the_four_sum_form_cancels():
    """policy = reference + 1e-3 (LoRA initialisation): the margin is the small difference of four sums of order n.  The margin accumulated element by element in
    fp32 stays inside its derived bound against fp64; the same fp32 arithmetic on the four sums is OUTSIDE it — the reason st355_flow_dpo_stats is shaped as it is."""
    B, N = 3, 65536
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(2 * B, N, generator=g)
    tw, tl = torch.randn(B, N, generator=g), torch.randn(B, N, generator=g)
    pol = ref + 1e-3
    adv32, four32 = FB.margin_forms(pol, ref, tw, tl)
    st = FR.stats64(pol.to(F32), ref.to(F32), tw.to(F32), tl.to(F32))
    want = st[:, 7] + st[:, 8]
    _, tol = FB.stats_ref(pol.to(F32), ref.to(F32), tw.to(F32), tl.to(F32), depth=16)          # log2(N) levels of margin_forms' tree
    bound = tol[:, 7] + tol[:, 8] + U * want.abs()
    e_adv, e_four = (adv32.double() - want).abs(), (four32.double() - want).abs()
    assert bool((e_adv <= bound).all()), (e_adv, bound)
    assert bool((e_four > bound).all()), (e_four, bound)
    print(f"[margin] |margin| {want.abs().tolist()}, bound {bound.tolist()}, element-wise error {e_adv.tolist()}, four-sum error {e_four.tolist()}")


def test_ema_over_three_calls_and_the_device_resident_state():
    d = FR.operands(3, 1024, seed=3)
    state = torch.zeros(2)
    kw = dict(norm_type="mean", auto_num=FR.auto_num(0.2, 1e-6), decay=0.5, beta_min=1e-3, beta_max=50.0)
    emas, betas = [], []
    for k in range(3):
        dk = FR.operands(3, 1024, seed=3 + k, delta=0.1 * (k + 1))
        st = FR.flow_dpo_stats(dk.policy, dk.ref, dk.tw, dk.tl)
        _, pair, logs = FR.flow_dpo_head(st, 1024, ema_state=state, **kw)
        emas.append(float(state[0])); betas.append(float(logs[1]))
        assert float(state[1]) == 1.0 and abs(float(logs[14]) - emas[-1]) < 1e-7
    am = [float(x) for x in emas]
    assert am[0] != am[1] != am[2] and all(abs(b - min(max(kw["auto_num"] / e, 1e-3), 50.0)) < 1e-4 * b for b, e in zip(betas, emas))


# ------------------------------------------------------------------------------------------------
# (c) refusals and the dropout override
# ------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(hip_graph=True), "distillation_method=flow_dpo with hip_graph: the step reads its logs on the host every step and cannot be captured"),
    (dict(tread_config={"routes": [{"start_layer_idx": 0}]}), "distillation_method=flow_dpo with TREAD routing: the reference's four forwards would each route their own token subset; not built on the st355 path"),
    (dict(xm_noise_candidates_enabled=True), "distillation_method=flow_dpo with XM noise candidates is not built on the st355 path"),
    (dict(scheduled_sampling_max_step_offset=2), "distillation_method=flow_dpo with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow): the rollout would re-time the preferred sample only; not built on the st355 path"),
    (dict(scheduled_sampling_reflexflow=True), "distillation_method=flow_dpo with scheduled sampling / ReflexFlow (scheduled_sampling_max_step_offset, scheduled_sampling_reflexflow): the rollout would re-time the preferred sample only; not built on the st355 path"),
    (dict(layersync_enabled=True), "distillation_method=flow_dpo with layersync_enabled: LayerSync's taps would see the 2B rows of the doubled batch; not built on the st355 path"),
    (dict(internal_guidance_enabled=True), "distillation_method=flow_dpo with internal_guidance_enabled: Internal Guidance's taps would see the 2B rows of the doubled batch; not built on the st355 path"),
    (dict(nextlat_enabled=True), "distillation_method=flow_dpo with nextlat_enabled: NextLat's taps would see the 2B rows of the doubled batch; not built on the st355 path"),
    (dict(use_dora=True), "distillation_method=flow_dpo with use_dora: the adapters-off forward through the DoRA fold is not built on the st355 path; set --use_dora=false"),
    (dict(lora_type="lycoris"), "distillation_method=flow_dpo with lora_type=lycoris: the adapters-off forward through the LoKr fold is not built on the st355 path; set --lora_type=standard"),
    (dict(controlnet=True), "distillation_method=flow_dpo with controlnet is not built on the st355 path"),
]


@pytest.mark.parametrize("cfg,text", REFUSALS)
def test_every_configuration_that_is_not_built_is_refused_by_name(cfg, text):
    from simpletuner_amd import flow_dpo as FD
    with pytest.raises(NotImplementedError) as ei:
        FD.FlowDPODistiller(_stub_model(**cfg))
    assert str(ei.value) == text


def test_other_methods_tokenwise_timesteps_and_an_absent_flag():
    from simpletuner_amd import flow_dpo as FD
    with pytest.raises(NotImplementedError) as ei:
        FD.create_distiller(_stub_model(distillation_method="dmd"))
    assert str(ei.value) == "distillation_method=dmd: not built on the st355 path (built: flow_dpo)"
    for off in (None, "", "none", "None", "false", "0"):
        assert FD.create_distiller(_stub_model(distillation_method=off)) is None
    d = FD.FlowDPODistiller(_stub_model())
    lat = torch.zeros(2, 16, 8, 8, dtype=torch.bfloat16)
    batch = dict(conditioning_type="reference_strict", conditioning_latents=lat, latents=lat, noise=lat, input_noise=lat, sigmas=torch.zeros(2, 1, 1, 1),
                 noisy_latents=lat, timesteps=torch.zeros(2, 64))
    with pytest.raises(NotImplementedError) as ei:
        d.prepare_batch(batch)
    assert str(ei.value) == "distillation_method=flow_dpo with tokenwise timesteps (2, 64): the margin is per sample; not built on the st355 path"


def test_lora_dropout_is_overridden_with_the_reference_warning_and_the_force_switch_is_refused(monkeypatch, caplog):
    from simpletuner_amd import flow_dpo as FD
    monkeypatch.delenv(FD.DROPOUT_FORCE_ENV, raising=False)
    cfg = SimpleNamespace(distillation_method="flow_dpo", lora_dropout=0.1)
    with caplog.at_level(logging.WARNING, logger="simpletuner_amd.flow_dpo"):
        assert FD.adapter_dropout_override(cfg) == 0.0
    assert cfg.lora_dropout == 0.0
    assert caplog.messages == ["flow_dpo distillation reference implementations train adapters with lora_dropout=0.0; overriding --lora_dropout=0.1. Set "
                               "SIMPLETUNER_LORA_DROPOUT_FORCE_ENABLED=1 to keep the configured value. Adapter dropout also injects amplified noise into "
                               "finite-difference distillation targets."]
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="simpletuner_amd.flow_dpo"):
        assert FD.adapter_dropout_override(SimpleNamespace(distillation_method="flow_dpo", lora_dropout=0.0)) == 0.0
    assert not caplog.messages
    monkeypatch.setenv(FD.DROPOUT_FORCE_ENV, "1")
    with pytest.raises(NotImplementedError) as ei:
        FD.adapter_dropout_override(SimpleNamespace(distillation_method="flow_dpo", lora_dropout=0.1))
    assert str(ei.value).startswith("SIMPLETUNER_LORA_DROPOUT_FORCE_ENABLED with lora_dropout=0.1 under distillation_method=flow_dpo:")
    # through the plugin: SD3 (which builds dropout) ends at 0.0 under the method, and keeps its value without it
    monkeypatch.delenv(FD.DROPOUT_FORCE_ENV, raising=False)
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import default_config
    p = SD3(default_config(model_family="sd3", lora_dropout=0.1, distillation_method="flow_dpo"), _acc())
    assert p.lora_dropout_value() == 0.0 and p.config.lora_dropout == 0.0
    p = SD3(default_config(model_family="sd3", lora_dropout=0.1), _acc())
    assert p.lora_dropout_value() == 0.1


# ------------------------------------------------------------------------------------------------
# (d) adapters off; the engines and the Trainer on the emulator against the oracle
# ------------------------------------------------------------------------------------------------
B_STD = 0.5


def _plugin(monkeypatch, family, block_abi=False, with_adapters=True, **cfg_kw):
    from simpletuner_amd.training.trainer import default_config
    FR.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=B_STD, learning_rate=1e-3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", block_abi)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3 import transformer as T
        from simpletuner_amd.sd3.model import SD3
        monkeypatch.setattr(T, "_BLOCK_ABI", block_abi)
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(2))
    if with_adapters:
        plugin.add_lora_adapter()
        plugin.post_model_load_setup()
    return plugin


def _pairs(B, seed=3):
    cpu, devt = PU.make_inputs(B, 8, 8, 24, 128, 64, "cpu", seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    # the rejected latents are drawn independently of the preferred ones: the adapter gradient is the DIFFERENCE of the two halves' contributions, and a rejected
    # sample close to the preferred one would make the test measure the cancellation of two nearly equal gradients instead of the step
    lose = torch.randn(devt["latents"].shape, generator=g).to(torch.bfloat16)
    cpu["lose"] = lose.float()
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"],
             "conditioning_latents": lose, "conditioning_type": "reference_strict"}
    return cpu, devt, batch


def _trainer(monkeypatch, family, B=2, seed=3, block_abi=False, **cfg_kw):
    from simpletuner_amd.training.trainer import Trainer
    plugin = _plugin(monkeypatch, family, block_abi, **cfg_kw)
    trainer = Trainer(plugin.config, plugin, plugin.accelerator)
    cpu, devt, batch = _pairs(B, seed)
    plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"][:batch["latent_batch"].shape[0]], devt["sigmas"][:batch["latent_batch"].shape[0]] * 1000.0)
    return plugin, trainer, batch, cpu


def _head_on(pred, ref, cpu, dcfg, loss_orig=None):
    """(loss, bound): tests/flow_dpo_ref's fp64 head on the given bf16 predictions [2B, ...] and the bounds of tests/flow_dpo_bounds.py for the three ops' chain —
    the stats' bound carried through the head (|d loss / d margin_b| <= loss_weight beta / (2 B)), the head's own, and the plugin's fp32 mean for the SFT term"""
    B = pred.shape[0] // 2
    r16 = lambda t: t.to(torch.bfloat16)
    tw, tl = r16(cpu["noise"] - cpu["latents"]), r16(cpu["noise"] - cpu["lose"])
    n = tw.numel() // B
    st, tol_s = FB.stats_ref(pred, ref, tw, tl)
    orig = float(((pred[:B].double() - tw.double()) ** 2).reshape(B, -1).mean(1).mean())
    kw = dict(norm_type=dcfg["norm_type"], beta=dcfg.get("beta", 1.0), loss_weight=dcfg.get("loss_weight", 1.0), anchor_alpha=dcfg.get("anchor_alpha", 0.0))
    if dcfg.get("auto_beta", True):
        kw.update(ema_state=(0.0, 0.0), auto_num=FR.auto_num(dcfg.get("auto_beta_target_gf", 0.2), 1e-6), decay=dcfg.get("auto_beta_decay", 0.99), beta_min=1e-3, beta_max=dcfg.get("auto_beta_max", 1.0))
    hr = FB.head_ref(st.to(F32), n, **kw)
    (loss, tol), pair = hr["loss"], hr["pair"][0]
    nu, beta = pair[:, 3], float(hr["logs"][0][1])
    lw, aa, sw = abs(kw["loss_weight"]), abs(kw["anchor_alpha"]), dcfg.get("sft_loss_weight", 0.0)
    e_stats = lw * float((0.5 * beta * nu * (tol_s[:, 7] + tol_s[:, 8])).mean()) * (2.0 if "ema_state" in kw else 1.0) + 0.5 * aa * float((tol_s[:, 4] + tol_s[:, 5]).sum()) / (B * n)
    e_cast = 2 * U * float(st.abs().max()) * lw * beta * float(nu.max())          # the stats reach the head as fp32 numbers
    total = float(loss) + sw * orig
    # beta = num / mean |margin|: the stats' bound and the cast, relative to the EMA, on top of the head's own bound
    e_beta = float(hr["logs"][1][1]) + (beta * (float((nu * (tol_s[:, 7] + tol_s[:, 8])).mean()) + 2 * U * float((nu * st[:, 7:9].abs().sum(1)).mean()))
                                       / float(hr["logs"][0][13]) if "ema_state" in kw else 0.0) + U * beta
    return total, float(tol) + e_stats + e_cast + abs(sw) * orig * (FB.gamma(n + B + 8) + 4 * U) + 4 * U * abs(total), beta, e_beta


def oracle_snapshot(comp):
    """the component's weights as the oracle takes them, copied: the optimizer step that follows must not move them"""
    P, lora, scale = PU.oracle_state(comp)
    return {k: v.clone() for k, v in P.items()}, {k: (a.clone(), b.clone()) for k, (a, b) in lora.items()}, scale


def oracle_dpo_step(family, comp, cpu, dcfg, ema=None, beta_given=None, state=None):
    """the same step in plain torch: ONE oracle forward (fp32) at batch 2B with the adapters (autograd) and one without, the predictions rounded to bf16 where the
    engine holds bf16 tensors (straight-through), the loss by tests/flow_dpo_ref.loss64 (fp64).  beta_given: the (detached) beta to use instead of the oracle's own
    auto-beta — beta = num / mean |margin| carries the margin's bf16 noise at full strength, so the engine's value is held to the fp64 head on the engine's own
    predictions (_head_on) and handed to the oracle, whose job is the gradient.  Returns (loss, 2B prediction, {target: (dA, dB)}, margin, beta)"""
    r16 = lambda t: t.to(torch.bfloat16).float()
    P, lora, scale = state or oracle_snapshot(comp)
    B = cpu["latents"].shape[0]
    idx = torch.cat([torch.arange(B), torch.arange(B)])
    if family == "sd3":
        P["pos_embed.pos_embed"] = comp.pos_embed.pos_embed.detach().float().cpu()
        ocfg = SH._ocfg(comp)
        fwd = lambda lp, x, t: OS.sd3_forward(P, ocfg, x, cpu["prompt"][idx], cpu["pooled"][idx], t, lora=lp, lora_scale=scale)
    else:
        ocfg = PU.oracle_cfg(comp)
        fwd = lambda lp, x, t: OF.flux_model_predict(P, ocfg, x, cpu["prompt"][idx], cpu["pooled"][idx], t, 1.0, lora=lp, lora_scale=scale)
    x, lose, n, sig = cpu["latents"], cpu["lose"], cpu["noise"], cpu["sigmas"]
    s4 = sig.view(B, 1, 1, 1)
    noisy = torch.cat([r16((1 - s4) * x + s4 * n), r16((1 - s4) * lose + s4 * n)])
    tw, tl, t = r16(n - x), r16(n - lose), torch.cat([sig, sig]) * 1000.0
    lp = {k: (a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for k, (a, b) in lora.items()}
    pol = fwd(lp, noisy, t)
    with torch.no_grad():
        ref = r16(fwd(None, noisy, t))
    pol16 = pol + (r16(pol) - pol).detach()
    fl = lambda v, rows: v.double().reshape(rows, -1)
    _, margin = FR.loss64(fl(pol16, 2 * B), fl(ref, 2 * B), fl(tw, B), fl(tl, B), None, dcfg["norm_type"])
    beta = float(dcfg.get("beta", 1.0))
    if dcfg.get("auto_beta", True):
        am = float(margin.detach().abs().mean())
        ema = am if ema is None else dcfg.get("auto_beta_decay", 0.99) * ema + (1 - dcfg.get("auto_beta_decay", 0.99)) * am
        beta = min(max(FR.auto_num(dcfg.get("auto_beta_target_gf", 0.2), 1e-6) / max(ema, 1e-6), 1e-3), dcfg.get("auto_beta_max", 1.0))
    if beta_given is not None:
        beta = beta_given
    orig = ((pol16[:B].double() - tw.double()) ** 2).reshape(B, -1).mean(1).mean()
    loss, margin = FR.loss64(fl(pol16, 2 * B), fl(ref, 2 * B), fl(tw, B), fl(tl, B), None, dcfg["norm_type"], beta, dcfg.get("loss_weight", 1.0),
                             dcfg.get("anchor_alpha", 0.0), dcfg.get("sft_loss_weight", 0.0), orig)
    loss.backward()
    return loss.detach(), pol.detach(), {k: (a.grad, b.grad) for k, (a, b) in lp.items()}, margin.detach(), beta, ema, orig.detach()


DCFGS = [dict(norm_type="sum", auto_beta=False, beta=0.02, anchor_alpha=0.0, sft_loss_weight=0.0),
         # (auto-beta: the target gradient factor 0.4 puts |logit| near 0.4.  The coefficient sigma(-logit) turns a relative error eps of the margin — the engines'
         # bf16 noise, which the margin amplifies — into |logit| sigma(logit) eps ~ 0.25 eps; at the default 0.2 (|logit| ~ 1.4) that factor is ~ 1.1)
         dict(norm_type="mean", auto_beta=True, auto_beta_target_gf=0.4, auto_beta_max=1000.0, anchor_alpha=0.5, sft_loss_weight=0.3, loss_weight=0.8)]


@pytest.mark.parametrize("dcfg", DCFGS, ids=["sum-fixed", "mean-auto-anchor-sft"])
@pytest.mark.parametrize("block_abi", [False, True], ids=["host", "block-abi"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_train_step_matches_the_oracle(monkeypatch, family, block_abi, dcfg):
    """B = 2 pairs through Trainer.train_step on the emulator + the stand-ins.  The tolerances are those of the families' LoRA host-sequencing tests: prediction
    rel-L2 2e-2, loss 2e-3 * max(1, loss), adapter gradients rel-L2 5e-2.  FAILS WITHOUT THE FEATURE: the flag is unknown there and the step returns the plain loss."""
    plugin, trainer, batch, cpu = _trainer(monkeypatch, family, block_abi=block_abi, distillation_method="flow_dpo", distillation_config={"flow_dpo": dcfg})
    comp = plugin.get_trained_component()
    snap = oracle_snapshot(comp)
    seen = []
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: (seen.append(predict(pb)), seen[-1])[1]
    grads = _capture_grads(trainer)
    loss = trainer.train_step(dict(batch))
    logs = trainer.last_aux_logs
    o_loss, o_pred, o_grads, o_margin, o_beta, _, o_orig = oracle_dpo_step(family, comp, cpu, dcfg, state=snap,
                                                                           beta_given=logs["flow_dpo_beta"] if dcfg["auto_beta"] else None)
    assert len(seen) == 2                                                     # two forwards, not four
    pred, ref = seen[0]["model_prediction"].detach(), seen[1]["model_prediction"].detach()
    assert pred.shape[0] == 4 and ref.shape[0] == 4 and not ref.requires_grad and PU.rel_l2(pred, o_pred) < 2e-2
    # the loss and beta: the fp64 head on the engine's OWN two predictions, inside the kernels' derived bounds (the margin amplifies the engines' bf16 noise, so
    # the oracle's loss is no yardstick for it; the oracle holds the adapter gradients below)
    e_loss, e_tol, e_beta, e_beta_tol = _head_on(pred, ref, cpu, dcfg, loss_orig=None)
    assert abs(loss.item() - e_loss) <= e_tol, (loss.item(), e_loss, e_tol)
    assert abs(logs["flow_dpo_beta"] - e_beta) <= e_beta_tol, (logs["flow_dpo_beta"], e_beta, e_beta_tol)
    worst = _compare_grads(grads, o_grads)
    keys = ["flow_dpo_loss", "flow_dpo_beta", "flow_dpo_margin", "flow_dpo_win_adv", "flow_dpo_lose_adv", "flow_dpo_policy_win_err", "flow_dpo_policy_lose_err",
            "flow_dpo_ref_win_err", "flow_dpo_ref_lose_err", "flow_dpo_negative_margin_pct", "flow_dpo_gradient_factor", "total"]
    assert list(logs)[:12] == keys and ("flow_dpo_anchor_loss" in logs) == (dcfg["anchor_alpha"] != 0.0) and all(isinstance(v, float) for v in logs.values())
    assert abs(logs["total"] - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    # a step that ignores the flag returns the plain loss on the preferred rows: far outside the tolerance
    assert abs(loss.item() - o_orig.item()) > 10 * 2e-3 * max(1.0, o_loss.item())
    assert comp.lora_groups and getattr(comp, "_lora_off", None) is None          # the adapters are back on
    print(f"[emu] {family} block_abi={block_abi} {dcfg['norm_type']}: loss {loss.item():.5f} vs oracle {o_loss.item():.5f}, margin {logs['flow_dpo_margin']:.4f} vs "
          f"{o_margin.mean().item():.4f}, beta {logs['flow_dpo_beta']:.4f} vs {o_beta:.4f}, worst adapter gradient rel-L2 {worst:.3e}")


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_gradient_accumulation_of_two_equals_one_step_of_the_concatenated_pairs(monkeypatch, family):
    """two micro-steps of 1 pair each against one step of the 2 pairs, fixed beta (the EMA would see the pairs in a different grouping): the same adapter
    gradients within the host-sequencing tolerance, and the loss changes against the flag-off step"""
    dcfg = dict(norm_type="sum", auto_beta=False, beta=0.02)
    kw = dict(distillation_method="flow_dpo", distillation_config=dcfg)
    plugin, trainer, batch, cpu = _trainer(monkeypatch, family, **kw)
    g_one = _capture_grads(trainer)
    loss_one = trainer.train_step(dict(batch)).item()
    plugin2, trainer2, batch2, _ = _trainer(monkeypatch, family, gradient_accumulation_steps=2, **kw)
    sig = PU.make_inputs(2, 8, 8, 24, 128, 64, "cpu", seed=3)[1]["sigmas"]
    g_two = _capture_grads(trainer2)
    halves = []
    for i in range(2):
        plugin2.sample_flow_sigmas = lambda batch, state, i=i: (sig[i:i + 1], sig[i:i + 1] * 1000.0)
        halves.append(trainer2.train_step({k: (v[i:i + 1] if torch.is_tensor(v) else v) for k, v in batch2.items()}).item())
    assert g_one and g_one.keys() == g_two.keys()
    worst = max(PU.rel_l2(g_two[k], g_one[k]) for k in g_one)
    assert worst < 5e-2, worst
    assert abs(sum(halves) - loss_one) < 2e-3 * max(1.0, abs(loss_one))
    plugin3, trainer3, batch3, _ = _trainer(monkeypatch, family)
    batch3 = {k: v for k, v in batch3.items() if not k.startswith("conditioning")}
    assert trainer3.distiller is None and abs(trainer3.train_step(batch3).item() - loss_one) > 1e-2


def _load_launch_trace():
    spec = importlib.util.spec_from_file_location("launch_trace_tool", os.path.join(ROOT, "tools", "launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("block_abi", [False, True], ids=["host", "block-abi"])
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_the_adapters_off_forward_launches_the_base_models_sequence_and_moves_no_counter(monkeypatch, family, block_abi):
    """tools/launch_trace.py's records of the disabled forward equal those of the same component built without adapters, the predictions are equal bit for bit,
    and neither the noise counters nor the adapter arena move"""
    LT = _load_launch_trace()
    from tests import ops_emulator as EMU
    lines = []
    tracer = SimpleNamespace(f=SimpleNamespace(write=lines.append))
    plugin = _plugin(monkeypatch, family, block_abi)
    bare = _plugin(monkeypatch, family, block_abi, with_adapters=False)
    from simpletuner_amd import ops
    for name in EMU._EMULATED:
        monkeypatch.setattr(ops, name, LT.LaunchTrace.wrap(tracer, name, getattr(ops, name)))
    cpu, devt, _ = _pairs(2)
    pb = lambda: {"latents": devt["latents"], "noisy_latents": devt["latents"], "timesteps": devt["sigmas"] * 1000.0, "prompt_embeds": devt["prompt"],
                  "encoder_hidden_states": devt["prompt"], "add_text_embeds": devt["pooled"]}
    comp = plugin.get_trained_component()
    before = (plugin._noise_step, plugin._noise_offset, comp.lora_flat.clone())
    with torch.no_grad():
        on = plugin.model_predict(pb())["model_prediction"]
        lines.clear()
        with comp.lora_disabled():
            assert not comp.lora_groups
            off = plugin.model_predict(pb())["model_prediction"]
        t_off = list(lines)
        lines.clear()
        base = bare.model_predict(pb())["model_prediction"]
        t_base = list(lines)
    assert t_off and t_off == t_base
    assert torch.equal(off, base) and not torch.equal(on, off)
    assert comp.lora_groups and (plugin._noise_step, plugin._noise_offset) == before[:2] and torch.equal(comp.lora_flat, before[2])
    comp.disable_lora(); comp.disable_lora(); comp.enable_lora()
    assert comp.lora_groups
    with torch.no_grad():
        assert torch.equal(plugin.model_predict(pb())["model_prediction"], on)


def test_flux_does_not_route_the_rejected_sample_into_reference_image_tokens(monkeypatch):
    plugin, trainer, batch, cpu = _trainer(monkeypatch, "flux", distillation_method="flow_dpo", distillation_config=dict(auto_beta=False, beta=0.02))
    seen = []
    predict = plugin.model_predict
    plugin.model_predict = lambda pb: (seen.append(dict(pb)), predict(pb))[1]
    batch["conditioning_packed_latents"] = torch.zeros(2, 4, 64, dtype=torch.bfloat16)
    batch["conditioning_ids"] = torch.zeros(2, 4, 3)
    trainer.train_step(dict(batch))
    assert len(seen) == 2 and all("conditioning_packed_latents" not in pb and "conditioning_ids" not in pb and pb["noisy_latents"].shape[0] == 4 for pb in seen)

"""LayerSync on the MI355X: the two kernels of simpletuner_amd/csrc/layersync.hip against the fp64 restatement (tests/layersync_ref.py) of the same bf16 inputs,
element-wise, inside the derived bounds of tests/layersync_bounds.py; their in-place and determinism contracts; the emulator's stand-ins against them; and the
engines on the HIP path — Flux and SD3, LoRA and full-rank, the regulariser's gradient entering the hand-written dX chain — against autograd through the oracle."""
import functools

import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.engine import rows_of
from tests import layersync_bounds as LB
from tests import layersync_ref as LS
from tests import parity_utils as PU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
B, ROWS, ST = 2, 37, 5          # 74 rows: the last 4-row block is half empty; the strided form is the image rows of a [2 * (5 + 37), D] joint buffer
S = ST + ROWS
ZERO_T = (1, 7)                  # an all-zero teacher row


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(D: int):
    """host inputs (joint [B * S, D] bf16 buffers whose image rows are the operands) and the fp64 reference, computed once per D and never modified"""
    g = torch.Generator().manual_seed(100 + D)
    js = torch.randn(B * S, D, generator=g).to(BF16)
    jt = (0.6 * js.float() + 0.8 * torch.randn(B * S, D, generator=g)).to(BF16)
    jt.view(B, S, D)[ZERO_T[0], ST + ZERO_T[1]] = 0
    s, t = rows_of(js, ST, ROWS, B, S), rows_of(jt, ST, ROWS, B, S)
    c64, sim64, G64, sn = LS.reference64(s, t)
    assert torch.isfinite(G64).all() and torch.isfinite(c64).all() and G64.abs().max() > 0 and c64[ZERO_T[0] * ROWS + ZERO_T[1]] == 0
    return js, jt, c64, sim64, G64, sn


def _operands(D: int, strided: bool):
    js, jt = (x.clone().to(DEV) for x in _case(D)[:2])
    s, t = rows_of(js, ST, ROWS, B, S), rows_of(jt, ST, ROWS, B, S)
    if not strided:
        s, t = s.contiguous(), t.contiguous()
    return js, jt, s, t


def _outputs(D: int):
    return torch.empty(B * ROWS, D, dtype=BF16, device=DEV), torch.empty(B * ROWS, dtype=F32, device=DEV), torch.empty((), dtype=F32, device=DEV)


def _inside(c, sim, G, D):
    """100 % of the elements inside the derived bounds; returns the worst ratios"""
    _, _, c64, sim64, G64, sn = _case(D)
    n = B * ROWS
    rc = ((c.double().cpu() - c64).abs() / LB.cos_bound(D)).max().item()
    rs = abs(sim.double().item() - sim64.item()) / LB.sim_bound(D, n)
    rg = ((G.double().cpu() - G64).abs() / LB.grad_bound(G64, sn, D)).max().item()
    assert rc <= 1.0 and rs <= 1.0 and rg <= 1.0, (rc, rs, rg)
    return rc, rs, rg


@pytest.mark.parametrize("strided", [False, True], ids=["compact", "strided"])
@pytest.mark.parametrize("D", [64, 1536, 3072])
def test_forward_kernel_is_inside_the_derived_bounds(D, strided):
    js, jt, s, t = _operands(D, strided)
    js0, jt0 = js.clone(), jt.clone()
    G, c, sim = _outputs(D)
    ops.layersync_fwd(s, t, G, c, sim)
    rc, rs, rg = _inside(c, sim, G, D)
    print(f"[layersync] D={D} {'strided' if strided else 'compact'}: worst error / bound: cos {rc:.3f}, sim {rs:.3f}, G {rg:.3f}")
    assert torch.equal(js, js0) and torch.equal(jt, jt0)                       # the inputs (text rows of the joint buffers included) are read only
    zr = ZERO_T[0] * ROWS + ZERO_T[1]
    assert c[zr].item() == 0 and G[zr].abs().max().item() == 0                  # the all-zero teacher row: cosine 0, gradient 0, as the executed reference records


@pytest.mark.parametrize("D", [64, 1536, 3072])
def test_in_place_call_and_repeated_calls_give_the_same_bits(D):
    _, _, s, t = _operands(D, False)
    G, c, sim = _outputs(D)
    ops.layersync_fwd(s, t, G, c, sim)
    G2, c2, sim2 = _outputs(D)
    ops.layersync_fwd(s, t, G2, c2, sim2)
    assert torch.equal(G, G2) and torch.equal(c, c2) and torch.equal(sim, sim2)          # determinism: fixed-order reductions, no atomics
    buf = s.clone()                                                                      # G aliases the (compact) student: each lane writes only what it has read
    c3, sim3 = torch.empty_like(c), torch.empty_like(sim)
    ops.layersync_fwd(buf, t, buf.view(B * ROWS, D), c3, sim3)
    assert torch.equal(buf.view(B * ROWS, D), G) and torch.equal(c3, c) and torch.equal(sim3, sim)


@pytest.mark.parametrize("D", [64, 1536, 3072])
def test_inject_adds_the_scaled_gradient_to_the_image_rows_only(D):
    g = torch.Generator().manual_seed(7 + D)
    joint = torch.randn(B * S, D, generator=g).to(BF16)
    G = (torch.randn(B * ROWS, D, generator=g) * 0.05).to(BF16)
    scale = torch.tensor(-0.2 / 3.0, dtype=F32)                                           # -lambda / accumulation steps, as autograd hands it over: a 0-dim fp32 tensor
    want = joint.clone()
    rows_of(want, ST, ROWS, B, S).copy_((rows_of(joint, ST, ROWS, B, S).float() + scale * G.view(B, ROWS, D).float()).to(BF16))          # two fp32 roundings, then RNE to bf16
    dj = joint.clone().to(DEV)
    ops.layersync_inject(rows_of(dj, ST, ROWS, B, S), G.to(DEV), scale.to(DEV))
    assert torch.equal(dj.cpu(), want)                                                    # bit for bit, the text rows untouched
    assert not torch.equal(want, joint)
    cj = joint.clone()                                                                    # the emulator's stand-in is the same function
    LS.layersync_inject(rows_of(cj, ST, ROWS, B, S), G, scale)
    assert torch.equal(cj, want)


@pytest.mark.parametrize("D", [64, 1536, 3072])
def test_emulator_stand_in_agrees_with_the_kernel_inside_the_same_bounds(D):
    js, jt, c64, sim64, G64, sn = _case(D)
    s, t = rows_of(js, ST, ROWS, B, S), rows_of(jt, ST, ROWS, B, S)
    Ge, ce, sime = torch.empty(B * ROWS, D, dtype=BF16), torch.empty(B * ROWS, dtype=F32), torch.empty((), dtype=F32)
    LS.layersync_fwd(s, t, Ge, ce, sime)
    _inside(ce, sime, Ge, D)                                                              # the stand-in against fp64
    _, _, sd, td = _operands(D, True)
    G, c, sim = _outputs(D)
    ops.layersync_fwd(sd, td, G, c, sim)
    n = B * ROWS
    assert ((c.cpu() - ce).abs().double() <= LB.cos_bound(D)).all() and abs(sim.item() - sime.item()) <= LB.sim_bound(D, n)
    assert ((G.cpu().double() - Ge.double()).abs() <= LB.grad_bound(G64, sn, D)).all()


def test_wrappers_refuse_what_the_kernels_cannot_take():
    _, _, s, t = _operands(64, True)
    G, c, sim = _outputs(64)
    from simpletuner_amd.lib import St355Error
    with pytest.raises(St355Error):
        ops.layersync_fwd(s, t[:, :, :32], G, c, sim)                                     # shapes disagree
    with pytest.raises(St355Error):
        ops.layersync_fwd(s, t, G[:, :32], c, sim)                                        # G must be compact
    with pytest.raises(St355Error):
        ops.layersync_inject(s, G, torch.tensor(1.0))                                     # the scale lives on the device


# ------------------------------------------------------------------------------------------------
# engines on the HIP path
# ------------------------------------------------------------------------------------------------
LAMBDA = 8.0          # as in tests/test_layersync_cpu.py: makes the regulariser comparable to the MSE term in these tiny models' gradients (share asserted)


def _flux_inputs(Bq, lat_h, lat_w, S_txt, seed=5):
    from oracle import flux as OF
    g = torch.Generator().manual_seed(seed)
    bf = lambda x: x.to(BF16)
    lat = bf(torch.randn(Bq, 16, lat_h, lat_w, generator=g))
    packed = OF.pack_latents(lat.float())
    return dict(packed=bf(packed), prompt=bf(torch.randn(Bq, S_txt, 128, generator=g)), pooled=bf(torch.randn(Bq, 64, generator=g)),
                t=torch.rand(Bq, generator=g) * 0.8 + 0.1, target=bf(torch.randn(packed.shape, generator=g)),
                img_ids=OF.prepare_latent_image_ids(lat_h, lat_w), txt_ids=torch.zeros(S_txt, 3), guidance=torch.full((Bq,), 3.5))


def _flux_model(layers, single, full):
    from simpletuner_amd.flux.transformer import FluxTransformer2DModel
    model = FluxTransformer2DModel(device=DEV, **PU.small_flux_cfg(layers=layers, single=single))
    model.init_synthetic(11)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, targets="default", init_b_std=0.02)
    return model


def _flux_hip(model, d, lam):
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, sim = model(hidden_states=dd["packed"], encoder_hidden_states=dd["prompt"], pooled_projections=dd["pooled"], timestep=dd["t"], img_ids=dd["img_ids"],
                     txt_ids=dd["txt_ids"], guidance=dd["guidance"], return_dict=False)
    loss = ((out.float() - dd["target"].float()) ** 2).mean() - lam * sim
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), loss.detach().cpu(), sim.detach().cpu()


# student in the double stack, teacher in the single stack; the last case has tile-aligned streams (256 + 256 rows: the block-level C entry points run) and the student
# in the single stack above block 0 — the place where a stale pre-gated copy of dx would drop the regulariser from the proj_out branch
@pytest.mark.parametrize("full,layers,single,student,teacher,shape", [(False, 2, 2, 1, 3, (2, 16, 16, 32)), (True, 2, 2, 0, 2, (2, 16, 16, 32)), (False, 1, 3, 2, 3, (2, 32, 32, 256))],
                         ids=["lora", "full", "lora-aligned-single-student"])
def test_flux_step_with_layersync_matches_the_oracle(monkeypatch, full, layers, single, student, teacher, shape):
    model = _flux_model(layers, single, full)
    model.set_layersync(student, teacher)
    d = _flux_inputs(*shape)
    out, loss, sim = _flux_hip(model, d, LAMBDA)
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_sim, P, lp, share = LS.flux_oracle(monkeypatch, model, d, student, teacher, LAMBDA, full, None if full else lora, scale)
    r, c = PU.rel_l2(out, o_out), PU.cos_sim(out, o_out)
    print(f"[layersync] flux {'full' if full else 'lora'} s{student} t{teacher}: pred rel_l2={r:.3e} loss hip={loss.item():.6f} oracle={o_loss.item():.6f} "
          f"sim hip={sim.item():.6f} oracle={o_sim.item():.6f} regulariser share={share:.3e}")
    assert share > 0.2, share
    assert r < 2e-2 and c > 0.9995 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))          # tests/test_flux_model_gpu.py / test_flux_full_rank_gpu.py
    if full:
        LS.check_full_grads(model, P)
    else:
        LS.check_lora_grads(model, lp, 5e-2, cos=0.999)


def _sd3_model(layers, full):
    from simpletuner_amd.sd3.transformer import SD3Transformer2DModel
    from tests.test_sd3_model_gpu import _arch
    model = SD3Transformer2DModel(device=DEV, **_arch(layers))
    model.init_synthetic(11)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    return model


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_step_with_layersync_matches_the_oracle(monkeypatch, full):
    from tests.test_sd3_model_gpu import _ocfg
    model = _sd3_model(3, full)
    student, teacher = 0, 2
    model.set_layersync(student, teacher)
    g = torch.Generator().manual_seed(5)
    bf = lambda x: x.to(BF16)
    d = dict(lat=bf(torch.randn(2, 16, 16, 24, generator=g)), prompt=bf(torch.randn(2, 33, 128, generator=g)), pooled=bf(torch.randn(2, 64, generator=g)),
             t=(torch.rand(2, generator=g) * 0.8 + 0.1) * 1000.0, target=bf(torch.randn(2, 16, 16, 24, generator=g)))
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, sim = model(hidden_states=dd["lat"], encoder_hidden_states=dd["prompt"], pooled_projections=dd["pooled"], timestep=dd["t"], return_dict=False)
    loss = ((out.float() - dd["target"].float()) ** 2).mean() - LAMBDA * sim
    loss.backward()
    torch.cuda.synchronize()
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_sim, P, lp, share = LS.sd3_oracle(monkeypatch, model, _ocfg(model), d, student, teacher, LAMBDA, full, None if full else lora, scale)
    r, c = PU.rel_l2(out, o_out), PU.cos_sim(out, o_out)
    print(f"[layersync] sd3 {'full' if full else 'lora'}: pred rel_l2={r:.3e} loss hip={loss.item():.6f} oracle={o_loss.item():.6f} sim hip={sim.item():.6f} "
          f"oracle={o_sim.item():.6f} regulariser share={share:.3e}")
    assert share > 0.2, share
    assert r < 2e-2 and c > 0.9995 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))          # tests/test_sd3_model_gpu.py
    if full:
        LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",))
    else:
        LS.check_lora_grads(model, lp, 5e-2, cos=0.999)


def test_flux_lora_trajectory_with_layersync_follows_the_oracle(monkeypatch):
    """Five optimizer steps of Flux LoRA through the plugin and the trainer with layersync_lambda = 0.2, against the fp32 oracle stepped by torch.optim.AdamW with the
    regulariser on its recorded block outputs.  Stated bounds: |loss difference| <= 2e-3 per step (the bound of the 20-step trajectory in tests/test_muon_gpu.py);
    the similarity rises or holds from step to step.
    The pair: 2 double + 2 single blocks, student depth 1 (double block 0), teacher depth 4 (the last single block).  At lambda 0.2 the regulariser is a few percent
    of the adapter gradient, and whether the similarity rises against the MSE term depends on the pair — on the fp32 oracle alone it falls for the 1 + 1-block
    model (0.94048 -> 0.94042 in five steps) and rises for this one (0.8417 -> 0.8435, ~4.5e-4 per step; the bf16 engine's similarity sits a near-constant
    few 1e-4 beside the oracle's, and its step-to-step change differs from the oracle's by under 1e-4).  The test takes the configuration in which the reference arithmetic rises and asserts the rise on both sides.
    Whether it rises also depends on the weights, so they are not left to the device's generator: base weights and adapters are initialised by the same code on
    the host (a twin component on the CPU, seeded) and copied into the component — the oracle's side of this test is then one fixed fp32 computation
    (similarity 0.84166, 0.84212, 0.84255, 0.84301, 0.84346: +4.3e-4 to +4.6e-4 per step), the same on every machine.  With the device generator's weights the
    reference arithmetic itself turns down in the fifth step (0.762392 -> 0.762277 on the MI355X), which says nothing about the engine."""
    from oracle import flux as OF
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.flux.transformer import FluxTransformer2DModel
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    steps, lr, lam = 5, 1e-3, 0.2
    cfg = default_config(lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, layersync_enabled=True, layersync_student_block=1, layersync_teacher_block=4,
                         layersync_lambda=lam)
    acc = St355Accelerator(DEV)
    plugin = Flux(cfg, acc)
    plugin.load_model(**PU.small_flux_cfg(layers=2, single=2))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    model = plugin.get_trained_component()
    twin = FluxTransformer2DModel(device="cpu", **PU.small_flux_cfg(layers=2, single=2))
    twin.init_synthetic(seed=5)
    twin.add_lora_adapter(rank=16, targets=plugin._lora_target_set(), seed=12, init_b_std=0.02)
    host = dict(twin.named_parameters())
    assert set(host) == {n for n, _ in model.named_parameters()}
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            p_.copy_(host[n])
    model._weights_changed()
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(1, 16, 16, 64, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    assert model._layersync == (0, 3)
    P, lora, scale = PU.oracle_state(model)
    ocfg = PU.oracle_cfg(model)
    names = sorted(lora)
    params = {k: (torch.nn.Parameter(lora[k][0].clone()), torch.nn.Parameter(lora[k][1].clone())) for k in names}
    opt = torch.optim.AdamW([t for k in names for t in params[k]], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    outs = LS.record_flux_blocks(monkeypatch)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    s = cpu["sigmas"].view(-1, 1, 1, 1)
    noisy = ((1 - s) * cpu["latents"] + s * cpu["noise"]).to(BF16).float()
    target = (cpu["noise"] - cpu["latents"]).to(BF16).float()
    Si = (16 // 2) * (16 // 2)
    hip, ora, sims, o_sims = [], [], [], []
    for _ in range(steps):
        hip.append(trainer.train_step(dict(batch)).item())
        sims.append(trainer.last_aux_logs["layersync_similarity"])
        assert abs(trainer.last_aux_logs["layersync_loss"] + lam * sims[-1]) < 1e-6
        opt.zero_grad()
        outs.clear()
        pred = OF.flux_model_predict(P, ocfg, noisy, cpu["prompt"], cpu["pooled"], cpu["sigmas"] * 1000.0, 1.0, lora={k: params[k] for k in names}, lora_scale=scale)
        sim = LS.autograd_similarity(LS.image_tokens(outs[0], Si), LS.image_tokens(outs[3], Si))
        l = ((pred - target) ** 2).mean(dim=(1, 2, 3)).mean() - lam * sim
        l.backward(); opt.step()
        ora.append(l.item()); o_sims.append(sim.item())
    worst = max(abs(a - b) for a, b in zip(hip, ora))
    print(f"[layersync] flux lora {steps} steps, lambda {lam}: max |d loss| = {worst:.3e}; loss hip {[round(x, 5) for x in hip]} oracle {[round(x, 5) for x in ora]}")
    print(f"[layersync] similarity hip {[round(x, 6) for x in sims]} oracle {[round(x, 6) for x in o_sims]}")
    assert worst <= 2e-3
    assert all(b >= a for a, b in zip(sims, sims[1:])) and all(b >= a for a, b in zip(o_sims, o_sims[1:])), (sims, o_sims)

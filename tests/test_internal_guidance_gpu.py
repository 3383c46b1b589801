"""Internal Guidance on the MI355X: the kernels of simpletuner_amd/csrc/internal_guidance.hip against the fp64 restatement (tests/internal_guidance_ref.py),
element-wise, inside the derived bounds of tests/internal_guidance_bounds.py; their untouched-rows and determinism contracts; what the wrappers refuse; and the SD3
engine on the HIP path — LoRA and full fine-tune, the head's gradient entering the hand-written dX chain, a short AdamW trajectory — against autograd through the
oracle."""
import pytest
import torch

from simpletuner_amd import ops
from tests import internal_guidance_ref as IG
from tests import layersync_ref as LS
from tests import parity_utils as PU
from tests.test_internal_guidance_cpu import check_fold_fwd_bwd_wgrad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
PRE = IG.PREFIX
OPS = {k: getattr(ops, k) for k in IG.STAND_INS}
B, ROWS = 2, 35          # a 5 x 7 token grid: M = 70 is neither a multiple of the forward's 4 rows per block, nor of the backward's 16-row tiles and 64-row workgroups, nor of 64


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
# D: one guarded pass (64: also a guarded 64-column MFMA chunk), three passes (1536), a guarded tail of the six-pass body (2432), six full passes (3072);
# lead 8: the views are strided, 8 text rows ahead of each sample's image rows
@pytest.mark.parametrize("bf16_params", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lead", [0, 8], ids=["compact", "strided"])
@pytest.mark.parametrize("D", [64, 1536, 2432, 3072])
def test_kernels_are_inside_the_derived_bounds_and_repeat_bit_for_bit(D, lead, bf16_params):
    first = check_fold_fwd_bwd_wgrad(OPS, DEV, B, ROWS, D, lead, bf16_params)
    second = check_fold_fwd_bwd_wgrad(OPS, DEV, B, ROWS, D, lead, bf16_params)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i          # no atomics, fixed-order reductions: two calls give the same bits


def test_a_single_partial_tile():
    """M = 6 rows: one live backward wave with 10 dead token lanes beside three dead waves that still stage and meet the barriers, two forward blocks"""
    check_fold_fwd_bwd_wgrad(OPS, DEV, 1, 6, 64, 8, False)


def test_backward_at_a_d_that_is_a_multiple_of_8_only():
    """D = 72 (D % 16 = 8: a lane's 16 backward columns are valid in halves, the last MFMA chunk is guarded) — the backward kernel alone on made-up operands, since
    the forward's projection GEMM wants D % 64 == 0; strided dx view, rows outside it untouched"""
    from tests import internal_guidance_bounds as IB
    g = torch.Generator().manual_seed(72)
    D, M = 72, B * ROWS
    xhat, dy = torch.randn(M, D, generator=g).to(BF16), (torch.randn(M, 64, generator=g) / 64).to(BF16)
    rstd, WfT = torch.rand(M, generator=g) + 0.5, (torch.randn(D, 64, generator=g) / 8).to(BF16)
    dxj = torch.randn(B, ROWS + 8, D, generator=g).to(BF16)
    dev = dxj.to(DEV)
    ops.ig_head_bwd(xhat.to(DEV), rstd.to(DEV), dy.to(DEV), WfT.to(DEV), dev[:, 8:])
    torch.cuda.synchronize()
    got = dev.cpu()
    ref, tol = IB.bwd_bounds(xhat, rstd, dy, WfT, dxj[:, 8:].reshape(M, D))
    assert ((got[:, 8:].reshape(M, D).double() - ref).abs() <= tol).all() and torch.equal(got[:, :8], dxj[:, :8])
    assert (got[:, 8:] != dxj[:, 8:]).any()


def test_tap_without_a_dx_view_fills_only_the_head_gradients():
    from simpletuner_amd.engine import InternalGuidanceHead, InternalGuidanceTap
    g = torch.Generator().manual_seed(2)
    H, W, D = 10, 14, 1536
    params = [t.to(DEV) for t in (1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(64, D, generator=g) / D ** 0.5,
                                  0.05 * torch.randn(64, generator=g))]
    joint = torch.randn(B, ROWS + 8, D, generator=g).to(BF16).to(DEV)
    d_pred = (torch.randn(B, 16, H, W, generator=g) / 64).to(BF16).to(DEV)
    outs = []
    for with_dx in (True, False):
        grads = [torch.zeros_like(p) for p in params]
        tap = InternalGuidanceTap(InternalGuidanceHead(1, D, params, grads, 0, 0, DEV))
        tap.tap(1, joint[:, 8:])
        assert tap.prediction(H, W).shape == (B, 16, H, W)
        dx = torch.zeros(B, ROWS, D, dtype=BF16, device=DEV)
        tap.backward(d_pred, dx if with_dx else None)
        torch.cuda.synchronize()
        assert (dx.abs().max().item() > 0) == with_dx and all(t.abs().max().item() > 0 for t in grads)
        outs.append([t.cpu() for t in grads])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from simpletuner_amd.lib import St355Error
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    D, M = 64, B * ROWS
    gamma, beta, W, b = z(D, dt=F32), z(D, dt=F32), z(64, D, dt=F32), z(64, dt=F32)
    Wf, WfT, c, xhat, rstd, y, dy = z(64, D), z(D, 64), z(64), z(M, D), z(M, dt=F32), z(M, 64), z(M, 64)
    h = z(B, ROWS, D)
    for bad in (lambda: ops.ig_fold(z(60, dt=F32), z(60, dt=F32), z(64, 60, dt=F32), b, z(64, 60), z(60, 64), c),                      # D % 8
                lambda: ops.ig_fold(gamma, beta, z(32, D, dt=F32), z(32, dt=F32), z(32, D), z(D, 32), z(32)),                          # N != 64
                lambda: ops.ig_fold(gamma, beta.to(BF16), W, b, Wf, WfT, c),                                                         # mixed parameter dtypes
                lambda: ops.ig_fold(gamma, beta, W, b, Wf.float(), WfT, c),                                                          # folded operands are bf16
                lambda: ops.ig_head_fwd(h.float(), Wf, c, xhat, rstd, y),                                                            # wrong dtype
                lambda: ops.ig_head_fwd(z(B, ROWS, D + 1)[:, :, 1:], Wf, c, xhat, rstd, y),                                          # misaligned view (row stride % 8, base % 16)
                lambda: ops.ig_head_fwd(h, Wf, c, xhat, rstd, z(M, 32)),                                                             # N != 64
                lambda: ops.ig_head_fwd(z(B, ROWS, 72), z(64, 72), c, z(M, 72), rstd, y),                                            # the projection's GEMM: D % 64
                lambda: ops.ig_head_fwd(h, Wf, c, z(M, 2 * D)[:, :D], rstd, y),                                                      # xhat must be compact
                lambda: ops.ig_head_bwd(xhat, rstd, z(M, 32), WfT, h),                                                               # N != 64
                lambda: ops.ig_head_bwd(xhat, rstd.to(BF16), dy, WfT, h),                                                            # rstd is fp32
                lambda: ops.ig_head_bwd(xhat, rstd, dy, WfT, z(B, ROWS, D + 4)[:, :, 4:]),                                           # misaligned dx view
                lambda: ops.ig_wgrad(xhat, dy, gamma, beta, W, z(D, dt=F32), z(D, dt=F32), z(64, D), z(64, dt=F32)),                 # gradients in the parameters' dtype
                lambda: ops.ig_wgrad(xhat, z(M - 1, 64), gamma, beta, W, z(D, dt=F32), z(D, dt=F32), z(64, D, dt=F32), z(64, dt=F32))):
        with pytest.raises(St355Error):
            bad()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# the SD3 engine on the HIP path
# ------------------------------------------------------------------------------------------------
WEIGHT = 8.0          # as in tests/test_internal_guidance_cpu.py: makes the regulariser comparable to the MSE term in these tiny models' gradients (share asserted)


def _sd3_model(layers, block, full):
    """the model sizes of tests/test_layersync_gpu.py::_sd3_model, with the head laid out and seeded"""
    from simpletuner_amd.sd3.transformer import SD3Transformer2DModel
    from tests.test_sd3_model_gpu import _arch
    model = SD3Transformer2DModel(device=DEV, internal_guidance_block_index=block, **_arch(layers))
    model.init_synthetic(11)
    if full:
        model.enable_full_finetune()
    else:
        model.add_lora_adapter(rank=16, alpha=16.0, init_b_std=0.02)
    IG.seed_head(model)
    return model


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_step_with_internal_guidance_matches_the_oracle(monkeypatch, full):
    from tests.test_sd3_model_gpu import _ocfg
    block = 1
    model = _sd3_model(3, block, full)
    g = torch.Generator().manual_seed(5)
    bf = lambda x: x.to(BF16)
    d = dict(lat=bf(torch.randn(2, 16, 16, 24, generator=g)), prompt=bf(torch.randn(2, 33, 128, generator=g)), pooled=bf(torch.randn(2, 64, generator=g)),
             t=(torch.rand(2, generator=g) * 0.8 + 0.1) * 1000.0, target=bf(torch.randn(2, 16, 16, 24, generator=g)))
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, igp = model(hidden_states=dd["lat"], encoder_hidden_states=dd["prompt"], pooled_projections=dd["pooled"], timestep=dd["t"], return_dict=False)
    tgt = dd["target"].float()
    loss = ((out.float() - tgt) ** 2).mean() + WEIGHT * ((igp.float() - tgt) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_igp, P, lp, share, head = IG.sd3_oracle(monkeypatch, model, _ocfg(model), d, block, WEIGHT, full, None if full else lora, scale)
    r, c = PU.rel_l2(out, o_out), PU.cos_sim(out, o_out)
    print(f"[internal guidance] sd3 {'full' if full else 'lora'}: pred rel_l2={r:.3e} head pred rel_l2={PU.rel_l2(igp, o_igp):.3e} loss hip={loss.item():.6f} "
          f"oracle={o_loss.item():.6f} regulariser share={share:.3e}")
    assert share >= 0.1, share
    assert r < 2e-2 and c > 0.9995 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))          # tests/test_layersync_gpu.py's SD3 step
    assert PU.rel_l2(igp, o_igp) < 2e-2
    if full:
        LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",))
    else:
        LS.check_lora_grads(model, lp, 5e-2, cos=0.999)
    own = dict(model.named_parameters())
    for nm in IG.NAMES:          # the head's four gradients, in the form of layersync_ref.check_full_grads
        p, ref = own[PRE + nm], head[PRE + nm].grad
        rg, cg = PU.rel_l2(p.grad, ref), PU.cos_sim(p.grad, ref)
        assert rg < 6e-2 and cg > 0.998, f"{nm}: rel={rg:.3e} cos={cg:.5f}"


def test_sd3_lora_trajectory_moves_the_head_along_the_oracles(monkeypatch):
    """Three optimizer steps of SD3 LoRA through the plugin and the trainer (st355-adamw, internal_guidance_loss_weight 0.5, block 1) against the fp32 oracle stepped
    by torch.optim.AdamW over the adapters AND the head.  Stated bounds: |loss difference| <= 2e-3 per step (the bound of the trajectories in
    tests/test_layersync_gpu.py / tests/test_muon_gpu.py).  The head's parameters must move, and follow the oracle's: in its first steps AdamW moves every element by
    about lr * sign(g), so two runs whose gradients agree to the engine tests' 6e-2 rel-L2 can differ in direction only in elements whose |g| lies below that error —
    for roughly Gaussian entries fewer than P(|z| < 3 * 0.06) = 14 % of them; if every one of those flipped, the cosine of the two displacements would still be
    1 - 2 * 0.14 = 0.72.  Asserted: cosine(displacement, oracle's displacement) > 0.7 for each of the four tensors."""
    import torch.nn.functional as F
    from oracle import sd3 as OS
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_sd3_model_gpu import _arch, _ocfg
    steps, lr, w, block = 3, 1e-3, 0.5, 1
    cfg = default_config(model_family="sd3", lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, internal_guidance_enabled=True,
                         internal_guidance_block_index=block, internal_guidance_loss_weight=w)
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(3))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    model = plugin.get_trained_component()
    IG.seed_head(model)
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 24, 33, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    P, lora, scale = PU.oracle_state(model)
    head0 = {k: P.pop(k) for k in list(P) if k.startswith(PRE)}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    names = sorted(lora)
    params = {k: (torch.nn.Parameter(lora[k][0].clone()), torch.nn.Parameter(lora[k][1].clone())) for k in names}
    hp = [torch.nn.Parameter(head0[PRE + nm].clone()) for nm in IG.NAMES]
    # (the trainer's arena order: adapters, then the head)
    opt = torch.optim.AdamW([t for k in names for t in params[k]] + hp, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    outs = LS.record_sd3_blocks(monkeypatch)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    s = cpu["sigmas"].view(-1, 1, 1, 1)
    noisy = ((1 - s) * cpu["latents"] + s * cpu["noise"]).to(BF16).float()
    target = (cpu["noise"] - cpu["latents"]).to(BF16).float()
    hip, ora = [], []
    for _ in range(steps):
        hip.append(trainer.train_step(dict(batch)).item())
        assert set(trainer.last_aux_logs) == {"internal_guidance_loss", "internal_guidance_unweighted_loss"}
        opt.zero_grad()
        outs.clear()
        pred = OS.sd3_forward(P, _ocfg(model), noisy, cpu["prompt"], cpu["pooled"], cpu["sigmas"] * 1000.0, lora={k: params[k] for k in names}, lora_scale=scale)
        igp = IG.head_autograd(outs[block], *hp, 16, target.shape[2], target.shape[3])
        per = lambda x: ((x - target) ** 2).mean(dim=(1, 2, 3)).mean()
        l = per(pred) + w * per(igp)
        l.backward(); opt.step()
        ora.append(l.item())
    torch.cuda.synchronize()
    print(f"[internal guidance] sd3 LoRA trajectory: hip {[round(x, 5) for x in hip]} oracle {[round(x, 5) for x in ora]}")
    assert max(abs(a - b) for a, b in zip(hip, ora)) <= 2e-3
    own = dict(model.named_parameters())
    for nm, p_o in zip(IG.NAMES, hp):
        start = head0[PRE + nm]
        mine, theirs = own[PRE + nm].detach().float().cpu() - start, p_o.detach() - start
        assert mine.abs().max() > 0.5 * lr, nm                                   # the optimizer's one launch moved the head with the adapters
        cosd = F.cosine_similarity(mine.reshape(1, -1), theirs.reshape(1, -1)).item()
        assert cosd > 0.7, f"{nm}: cosine of the displacement against the oracle's {cosd:.4f}"

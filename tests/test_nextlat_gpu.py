"""NextLat on the MI355X: the kernels of simpletuner_amd/csrc/nextlat.hip against the fp64 restatement (tests/nextlat_ref.py), element-wise, inside the derived
bounds of tests/nextlat_bounds.py; their untouched-rows and determinism contracts; what the wrappers refuse; and the SD3 engine on the HIP path — LoRA and full
fine-tune, the predictor's gradient entering the hand-written dX chain, a short AdamW trajectory — against autograd through the oracle."""
import pytest
import torch

from simpletuner_amd import ops
from tests import layersync_ref as LS
from tests import nextlat_ref as NL
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_nextlat_cpu import HEAD_REL_CPU, WEIGHT, check_kernels, head_rel, hip_side, sd3_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
PRE = NL.PREFIX
OPS = {k: getattr(ops, k) for k in NL.STAND_INS}
B, S = 2, 35          # 35 token rows, 34 of them predictor rows: M = 68 is neither a multiple of 64 nor of the row kernels' 4 rows per block


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
# D: one guarded pass (64: also one fold tile and a quarter of a wgrad chunk), three passes (1536), a guarded tail of the six-pass body (2432), six full passes
# (3072); lead 8: the views are strided, 8 text rows ahead of each sample's token rows.  The loss forms alternate over the cases; both run at every D.
@pytest.mark.parametrize("bf16_params", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lead", [0, 8], ids=["compact", "strided"])
@pytest.mark.parametrize("D", [64, 1536, 2432, 3072])
def test_kernels_are_inside_the_derived_bounds_and_repeat_bit_for_bit(D, lead, bf16_params):
    mode = NL.MODES[(lead // 8 + int(bf16_params)) % 2]
    first = check_kernels(OPS, DEV, B, S, D, lead, bf16_params, mode)
    second = check_kernels(OPS, DEV, B, S, D, lead, bf16_params, mode)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i          # no atomics, fixed-order reductions: two calls give the same bits


def test_a_single_partial_tile():
    """B = 1, 3 tokens: M = 2 rows — one row workgroup half empty, one loss workgroup with two idle waves, one partial fold tile, one wgrad chunk"""
    for mode in NL.MODES:
        check_kernels(OPS, DEV, 1, 3, 64, 8, False, mode)


def test_row_kernels_at_a_d_that_is_a_multiple_of_8_only():
    """D = 72: the GEMM-bound row pass refuses it, the loss and the LayerNorm backward take D % 8 == 0 (one guarded pass with a ragged last lane group)"""
    from tests import nextlat_bounds as NB
    g = torch.Generator().manual_seed(72)
    D, rows, lead = 72, S - 1, 8
    M = B * rows
    joint = torch.randn(B, lead + S, D, generator=g).to(BF16)
    x64, rs64 = NL.rows64(joint[:, lead:lead + rows].reshape(M, D))
    xhat, rstd = x64.to(BF16).to(DEV), rs64.float().to(DEV)
    gg, dxj = torch.randn(M, D, generator=g).to(BF16).to(DEV), torch.randn(B, lead + S, D, generator=g).to(BF16).to(DEV)
    pred = (joint[:, lead + 1:].float().reshape(M, D) + 1.2 * torch.randn(M, D, generator=g)).to(BF16).to(DEV)
    joint = joint.to(DEV)
    dx0 = dxj.clone()
    scale = torch.tensor([0.37], dtype=F32, device=DEV)
    ops.nextlat_ln_bwd_add(gg, xhat, rstd, scale, dxj[:, lead:lead + rows])
    ref, tol = NB.ln_bwd_add_bounds(gg.cpu(), xhat.cpu(), rstd.cpu(), scale.item(), dx0.cpu()[:, lead:lead + rows].reshape(M, D))
    assert ((dxj.cpu()[:, lead:lead + rows].reshape(M, D).double() - ref).abs() <= tol).all()
    assert torch.equal(dxj.cpu()[:, :lead], dx0.cpu()[:, :lead]) and torch.equal(dxj.cpu()[:, lead + rows:], dx0.cpu()[:, lead + rows:])
    psi, loss = pred.clone(), torch.zeros(1, device=DEV)
    ops.nextlat_loss(psi, joint[:, lead + 1:], "smooth_l1", loss)
    l64, tl, p64, tp = NB.loss_bounds(pred.cpu(), joint[:, lead + 1:].cpu().reshape(M, D), "smooth_l1")
    assert abs(loss.item() - l64.item()) <= tl.item() and ((psi.cpu().double() - p64).abs() <= tp).all()


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from simpletuner_amd.lib import St355Error
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    D, rows = 64, S - 1
    M, N = B * rows, 128
    P = lambda dt=F32, D=D: [z(D, dt=dt), z(D, dt=dt), z(2 * D, D, dt=dt), z(2 * D, dt=dt), z(D, 2 * D, dt=dt), z(D, dt=dt)]
    F_ = lambda D=D: [z(2 * D, D), z(D, 2 * D), z(2 * D), z(D, 2 * D), z(2 * D, D), z(D)]
    p, f = P(), F_()
    h, xhat, rstd, loss, s = z(B, S, D), z(M, D), z(M, dt=F32), z(1, dt=F32), z(1, dt=F32)
    odd = z(D + 1, dt=F32)[1:]                                                                                                          # starts 4 bytes off a 16-byte boundary
    for bad in (lambda: ops.nextlat_fold(*P(D=60), *F_(D=60)),                                                                            # D % 8
                lambda: ops.nextlat_fold(p[0], p[1].to(BF16), *p[2:], *f),                                                               # mixed parameter dtypes
                lambda: ops.nextlat_fold(*p[:2], z(D, D, dt=F32), *p[3:], *f),                                                           # W_up is [2D, D]
                lambda: ops.nextlat_fold(*p, f[0].float(), *f[1:]),                                                                      # folded operands are bf16
                lambda: ops.nextlat_fold(odd, *p[1:], *f),                                                                           # a parameter off a 16-byte boundary
                lambda: ops.nextlat_fold(*p, *f[:5], z(2 * D)[:D * 2:2]),                                                                # outputs are compact
                lambda: ops.nextlat_rows(h.float()[:, :rows], xhat, rstd),                                                               # wrong dtype
                lambda: ops.nextlat_rows(z(B, S, D + 1)[:, :rows, 1:], xhat, rstd),                                                      # misaligned view (row stride % 8, base % 16)
                lambda: ops.nextlat_rows(z(B, S, 72)[:, :rows], z(M, 72), rstd),                                                         # the up projection's GEMM: D % 64
                lambda: ops.nextlat_rows(h[:, :rows], z(M, 2 * D)[:, :D], rstd),                                                         # xhat must be compact
                lambda: ops.gelu_erf(z(M, N), z(M, N).float()),                                                                          # bf16 only
                lambda: ops.gelu_erf(z(M, N + 4)[:, :N], z(M, N)),                                                                       # compact
                lambda: ops.gelu_erf(z(3, 5), z(3, 5)),                                                                                  # a multiple of 8 elements
                lambda: ops.gelu_erf_bwd(z(M, N), z(M, N), z(M, N // 2)),                                                                # one shape
                lambda: ops.nextlat_loss(xhat, h[:, 1:], "l1", loss),                                                                    # the two loss forms
                lambda: ops.nextlat_loss(xhat, h[:, 1:], "mse", loss.to(BF16)),                                                          # the loss is fp32
                lambda: ops.nextlat_loss(z(M, 2 * D)[:, :D], h[:, 1:], "mse", loss),                                                     # pred must be compact
                lambda: ops.nextlat_loss(z(M - 1, D), h[:, 1:], "mse", loss),                                                            # one prediction row per target row
                lambda: ops.nextlat_loss(z(M, D + 4)[:, 4:].contiguous(), z(B, S, D + 4)[:, 1:, 4:], "mse", loss),                       # misaligned target view
                lambda: ops.nextlat_ln_bwd_add(xhat, xhat, rstd.to(BF16), s, h[:, :rows]),                                               # rstd is fp32
                lambda: ops.nextlat_ln_bwd_add(xhat, xhat, rstd, z(2, dt=F32), h[:, :rows]),                                             # ONE scale
                lambda: ops.nextlat_ln_bwd_add(xhat, xhat, rstd, 0.5, h[:, :rows]),                                                      # ... on the device
                lambda: ops.nextlat_ln_bwd_add(xhat, xhat, rstd, s, z(B, S, D + 4)[:, :rows, 4:]),                                       # misaligned dx view
                lambda: ops.nextlat_wgrad_up(z(N, D), z(N, dt=F32), *p[:3], s, z(D, dt=F32), z(D, dt=F32), z(N, D), z(N, dt=F32)),     # gradients in the parameters' dtype
                lambda: ops.nextlat_wgrad_up(z(N, D, dt=F32), z(N, dt=F32), *p[:3], s, z(D, dt=F32), z(D, dt=F32), z(N, D, dt=F32), z(N, dt=F32)),      # P1 is bf16
                lambda: ops.nextlat_wgrad_up(z(N, D), z(N - 1, dt=F32), *p[:3], s, z(D, dt=F32), z(D, dt=F32), z(N, D, dt=F32), z(N, dt=F32)),           # db1 [2D]
                lambda: ops.nextlat_wgrad_down(z(D, N), z(D, dt=F32), s, z(D, N, dt=F32), z(D)),                                         # one gradient dtype
                lambda: ops.nextlat_wgrad_down(z(N, D), z(D, dt=F32), s, z(D, N, dt=F32), z(D, dt=F32)),                                 # P2 [D, 2D]
                lambda: ops.nextlat_wgrad_down(z(D, N), z(D, dt=F32), s, z(D, N, dt=F32), z(D + 1, dt=F32)[1:])):                        # g_b off a 16-byte boundary
        with pytest.raises(St355Error):
            bad()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# the SD3 engine on the HIP path
# ------------------------------------------------------------------------------------------------
def _gpu_model(full, mode="smooth_l1"):
    """the model, weights and block of tests/test_nextlat_cpu.py's measurement at these shapes (tests/test_sd3_model_gpu._arch(3)), on the device"""
    from tests.test_sd3_model_gpu import _arch
    return sd3_model(None, None, 3, 1, full, dev=DEV, arch=_arch, mode=mode)


@pytest.mark.parametrize("full", [False, True], ids=["lora", "full"])
def test_sd3_step_with_nextlat_matches_the_oracle(monkeypatch, full):
    """One SD3 step at tests/test_sd3_model_gpu._arch(3), tap at block 1, weight 8 (the regulariser's share of the trunk gradient asserted >= 0.1), against autograd
    through the oracle.  Thresholds of tests/test_internal_guidance_gpu.py's SD3 step: prediction rel-L2 < 2e-2, cosine > 0.9995, |loss difference| < 1e-3
    max(1, |loss|), check_lora_grads(5e-2, cos 0.999) / check_full_grads.  The six predictor gradients: P1 and P2 are bf16 (Internal Guidance's P is fp32), so
    their tolerance is measured, not borrowed — the CPU stand-ins against the oracle at these shapes, weights and inputs give a worst rel-L2 of 4.02e-3 (LoRA) and
    3.96e-3 (full fine-tune) (tests/test_nextlat_cpu.py, HEAD_REL_CPU = 4.1e-3); the GPU is allowed twice that, 8.2e-3."""
    from tests.test_sd3_model_gpu import _ocfg
    block = 1
    model = _gpu_model(full)
    d = SH._inputs(2, 16, 24, 33)
    dd = {k: v.to(DEV) for k, v in d.items()}
    out, loss, state = hip_side(model, dd, WEIGHT)
    torch.cuda.synchronize()
    _, lora, scale = PU.oracle_state(model)
    o_out, o_loss, o_state, P, lp, share, head = NL.sd3_oracle(monkeypatch, model, _ocfg(model), d, block, WEIGHT, full, None if full else lora, scale)
    r, c = PU.rel_l2(out, o_out), PU.cos_sim(out, o_out)
    rg, cg = head_rel(model, head)
    print(f"[nextlat] sd3 {'full' if full else 'lora'}: pred rel_l2={r:.3e} state hip={state.item():.6f} oracle={o_state.item():.6f} loss hip={loss.item():.6f} "
          f"oracle={o_loss.item():.6f} regulariser share={share:.3e} predictor gradients worst rel_l2={rg:.3e} cos={cg:.6f}")
    assert share >= 0.1, share
    assert r < 2e-2 and c > 0.9995 and abs(loss.item() - o_loss.item()) < 1e-3 * max(1.0, abs(o_loss.item()))
    if full:
        LS.check_full_grads(model, P, skip=("pos_embed.pos_embed",))
    else:
        LS.check_lora_grads(model, lp, 5e-2, cos=0.999)
    assert rg <= 2 * HEAD_REL_CPU, f"predictor gradients: rel={rg:.3e} cos={cg:.6f}"


def test_sd3_lora_trajectory_moves_the_predictor_along_the_oracles(monkeypatch):
    """Three optimizer steps of SD3 LoRA through the plugin and the trainer (st355-adamw, nextlat_weight 0.5, block 1) against the fp32 oracle stepped by
    torch.optim.AdamW over the adapters AND the predictor.  Stated bounds: |loss difference| <= 2e-3 per step (the bound of the trajectories in
    tests/test_layersync_gpu.py / tests/test_internal_guidance_gpu.py).  The predictor's parameters must move, and follow the oracle's — the displacement-cosine
    argument and its 0.7 bound are those of tests/test_internal_guidance_gpu.py's trajectory: in its first steps AdamW moves every element by about lr * sign(g),
    so two runs whose gradients agree to 6e-2 rel-L2 can differ in direction in fewer than 14 % of the elements, which leaves a cosine of at least 0.72."""
    import torch.nn.functional as F
    from oracle import sd3 as OS
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_sd3_model_gpu import _arch, _ocfg
    steps, lr, w, block = 3, 1e-3, 0.5, 1
    cfg = default_config(model_family="sd3", lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, nextlat_enabled=True, nextlat_block_index=block, nextlat_weight=w)
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(3))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    model = plugin.get_trained_component()
    NL.seed_predictor(model)
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 24, 33, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    P, lora, scale = PU.oracle_state(model)
    head0 = {k: P.pop(k) for k in list(P) if k.startswith(PRE)}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    names = sorted(lora)
    params = {k: (torch.nn.Parameter(lora[k][0].clone()), torch.nn.Parameter(lora[k][1].clone())) for k in names}
    hp = [torch.nn.Parameter(head0[PRE + nm].clone()) for nm in NL.NAMES]
    # (the trainer's arena order: adapters, then the predictor)
    opt = torch.optim.AdamW([t for k in names for t in params[k]] + hp, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    outs = LS.record_sd3_blocks(monkeypatch)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    s = cpu["sigmas"].view(-1, 1, 1, 1)
    noisy = ((1 - s) * cpu["latents"] + s * cpu["noise"]).to(BF16).float()
    target = (cpu["noise"] - cpu["latents"]).to(BF16).float()
    hip, ora = [], []
    for _ in range(steps):
        hip.append(trainer.train_step(dict(batch)).item())
        assert list(trainer.last_aux_logs) == ["nextlat_loss", "nextlat_state_loss"]
        opt.zero_grad()
        outs.clear()
        pred = OS.sd3_forward(P, _ocfg(model), noisy, cpu["prompt"], cpu["pooled"], cpu["sigmas"] * 1000.0, lora={k: params[k] for k in names}, lora_scale=scale)
        l = ((pred - target) ** 2).mean(dim=(1, 2, 3)).mean() + w * NL.state_autograd(outs[block], hp)
        l.backward(); opt.step()
        ora.append(l.item())
    torch.cuda.synchronize()
    print(f"[nextlat] sd3 LoRA trajectory: hip {[round(x, 5) for x in hip]} oracle {[round(x, 5) for x in ora]}")
    assert max(abs(a - b) for a, b in zip(hip, ora)) <= 2e-3
    own = dict(model.named_parameters())
    for nm, p_o in zip(NL.NAMES, hp):
        start = head0[PRE + nm]
        mine, theirs = own[PRE + nm].detach().float().cpu() - start, p_o.detach() - start
        assert mine.abs().max() > 0.5 * lr, nm                                   # the optimizer's one launch moved the predictor with the adapters
        cosd = F.cosine_similarity(mine.reshape(1, -1), theirs.reshape(1, -1)).item()
        assert cosd > 0.7, f"{nm}: cosine of the displacement against the oracle's {cosd:.4f}"

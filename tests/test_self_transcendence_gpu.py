"""Self-Transcendence on the MI355X: the kernels of simpletuner_amd/csrc/self_transcendence.hip against the fp64 restatement (tests/self_transcendence_ref.py),
element-wise, inside the derived bounds of tests/self_transcendence_bounds.py, with guard bytes around every output and two launches compared bit for bit; what the
wrappers refuse; and the SD3 engine on the HIP path — one LoRA step per stage and a short AdamW trajectory in stage `self` — against autograd through the oracle."""
import pytest
import torch

from simpletuner_amd import ops
from tests import layersync_ref as LS
from tests import parity_utils as PU
from tests import self_transcendence_bounds as TB
from tests import self_transcendence_ref as ST
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_self_transcendence_cpu import HP, PROJECTOR_GRAD_REL_CPU, TMAX, TMIN, _dcfg, check_step, engine_step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
PRE = ST.PREFIX


# ------------------------------------------------------------------------------------------------
# kernels: B = 2, latents [2, 16, 10, 14] -> S = 35 tokens, M = 70 rows — neither a multiple of 64 nor of a 256-lane workgroup's chunk count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TB.VAE_CASES, ids=lambda c: c["id"])
def test_vae_loss_is_inside_the_derived_bounds_and_repeats_bit_for_bit(case):
    TB.check_vae_loss(ops.st_vae_loss, case, DEV)


@pytest.mark.parametrize("case", TB.CFG_CASES, ids=lambda c: c["id"])
def test_cfg_loss_is_inside_the_derived_bounds_and_repeats_bit_for_bit(case):
    TB.check_cfg_loss(ops.st_cfg_loss, case, DEV)


@pytest.mark.parametrize("case", TB.FOLD_CASES, ids=lambda c: c["id"])
def test_fold_is_exact_to_one_rounding_and_leaves_the_unread_rows_untouched(case):
    TB.check_fold(ops.st_fold, case, DEV)


@pytest.mark.parametrize("case", TB.WGRAD_CASES, ids=lambda c: c["id"])
def test_wgrad_writes_and_accumulates_with_a_ragged_last_chunk(case):
    TB.check_wgrad(ops.st_wgrad, case, DEV)


@pytest.mark.parametrize("case", TB.DX_CASES, ids=lambda c: c["id"])
def test_dx_add_adds_into_the_strided_view_only(case):
    TB.check_dx_add(ops.st_dx_add, case, DEV)


def test_wrappers_refuse_what_the_kernels_cannot_take():
    """one refused precondition per ST_REQUIRE family, through the wrapper"""
    from simpletuner_amd.lib import St355Error
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    D, Hp, B, S, P = 64, 128, 2, 35, 64
    M = B * S
    prm = lambda D=D, Hp=Hp: [z(Hp, D, dt=F32), z(Hp, dt=F32), z(Hp, Hp, dt=F32), z(Hp, dt=F32), z(D, Hp, dt=F32), z(D, dt=F32)]
    outs = lambda D=D, Hp=Hp, P3=P: [z(Hp, D), z(D, Hp), z(Hp), z(Hp, Hp), z(Hp, Hp), z(Hp), z(D, Hp), z(Hp, P3), z(D)]
    p, o = prm(), outs()
    sig, per, st, s = z(B, dt=F32), z(B, dt=F32), z(3, dt=F32), z(1, dt=F32)
    tgt, cap = z(B, 16, 10, 14), z(2 * B, S, D)
    odd = z(Hp * D + 1, dt=F32)[1:].view(Hp, D)                                                                      # starts 4 bytes off a 16-byte boundary
    for bad in (lambda: ops.st_fold(*prm(D=60), *outs(D=60)),                                                        # D % 8
                lambda: ops.st_fold(*p, *outs(P3=12)),                                                               # P3 % 8
                lambda: ops.st_fold(*p, *outs(P3=128)),                                                              # P3 > D
                lambda: ops.st_fold(odd, *p[1:], *o),                                                                # a master off a 16-byte boundary
                lambda: ops.st_fold(p[0].to(BF16), *p[1:], *o),                                                      # masters are fp32
                lambda: ops.st_fold(*p, o[0].float(), *o[1:]),                                                       # operands are bf16
                lambda: ops.st_fold(*p[:2], z(Hp, D, dt=F32), *p[3:], *o),                                           # W2 is [Hp, Hp]
                lambda: ops.st_vae_loss(z(M, P), tgt, (5, 5), sig, 0.4, 0.7, per, st),                               # the grid does not divide the latent
                lambda: ops.st_vae_loss(z(M, P), tgt, (5, 14), sig, 0.4, 0.7, per, st),                              # ... or does not hold S tokens: pred has other rows
                lambda: ops.st_vae_loss(z(M, 2 * P)[:, :P], tgt, (5, 7), sig, 0.4, 0.7, per, st),                    # pred must be compact
                lambda: ops.st_vae_loss(z(M, P), tgt.to(torch.float16), (5, 7), sig, 0.4, 0.7, per, st),             # target bf16 or fp32
                lambda: ops.st_vae_loss(z(M, P), tgt, (5, 7), sig, 0.7, 0.4, per, st),                               # min <= max
                lambda: ops.st_vae_loss(z(M, P), tgt, (5, 7), sig.to(BF16), 0.4, 0.7, per, st),                      # sigmas fp32
                lambda: ops.st_vae_loss(z(M, P), tgt, (5, 7), sig, 0.4, 0.7, per, z(2, dt=F32)),                     # stats [3]
                lambda: ops.st_vae_loss(z(M, 12), z(B, 3, 10, 14), (5, 7), sig, 0.4, 0.7, per, st),                  # P % 8
                lambda: ops.st_vae_loss(z(M, P), tgt.permute(0, 1, 3, 2), (7, 5), sig, 0.4, 0.7, per, st),           # samples contiguous
                lambda: ops.st_cfg_loss(z(M, D), z(3, S, D), 3.0, sig, 0.4, 0.7, per, st),                           # an even batch
                lambda: ops.st_cfg_loss(z(M, D), z(2 * B, S, D + 4)[:, :, 4:], 3.0, sig, 0.4, 0.7, per, st),         # misaligned capture view
                lambda: ops.st_cfg_loss(z(M, D), cap.float(), 3.0, sig, 0.4, 0.7, per, st),                          # bf16 capture
                lambda: ops.st_cfg_loss(z(M - 1, D), cap, 3.0, sig, 0.4, 0.7, per, st),                              # one prediction row per teacher row
                lambda: ops.st_wgrad(z(Hp, D), z(Hp, dt=F32), 0.5, z(Hp, D, dt=F32), z(Hp, dt=F32)),                 # the scale lives on the device
                lambda: ops.st_wgrad(z(Hp, D), z(Hp, dt=F32), z(2, dt=F32), z(Hp, D, dt=F32), z(Hp, dt=F32)),        # ONE scale
                lambda: ops.st_wgrad(z(Hp, D, dt=F32), z(Hp, dt=F32), s, z(Hp, D, dt=F32), z(Hp, dt=F32)),           # P is bf16
                lambda: ops.st_wgrad(z(Hp, 60), z(Hp, dt=F32), s, z(Hp, 60, dt=F32), z(Hp, dt=F32)),                 # Cc % 8
                lambda: ops.st_wgrad(z(Hp, D), z(Hp - 1, dt=F32), s, z(Hp, D, dt=F32), z(Hp, dt=F32)),               # db [R]
                lambda: ops.st_wgrad(z(Hp, D), z(Hp, dt=F32), s, z(Hp * D + 1, dt=F32)[1:].view(Hp, D), z(Hp, dt=F32)),      # g_W off a 16-byte boundary
                lambda: ops.st_dx_add(z(M, D), s, z(B, S, D + 4)[:, :, 4:]),                                         # misaligned dx view
                lambda: ops.st_dx_add(z(M, D).float(), s, z(B, S, D)),                                               # g is bf16
                lambda: ops.st_dx_add(z(M + 1, D), s, z(B, S, D)),                                                   # one addend row per view row
                lambda: ops.st_dx_add(z(M, D), 0.5, z(B, S, D))):                                                    # the scale lives on the device
        with pytest.raises(St355Error):
            bad()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# the SD3 engine on the HIP path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,student", [("vae", 0), ("self", 1)])
def test_sd3_step_with_self_transcendence_matches_the_oracle(monkeypatch, stage, student):
    """One SD3 LoRA step per stage at tests/test_sd3_model_gpu._arch(3) with inputs SH._inputs(2, 16, 24, 33), student block 0 / 1, teacher block 2, Hp = 128, the
    weight of tests/test_self_transcendence_cpu.W_GUIDE (the regulariser's share asserted >= 0.1), against autograd through the oracle.  Thresholds of
    tests/test_nextlat_gpu.py's SD3 step: prediction rel-L2 < 2e-2, cosine > 0.9995, |loss difference| < 1e-3 max(1, |loss|), check_lora_grads(5e-2, cos 0.999).
    The projector's gradients: the three P products are bf16 gemm_tn outputs, so their tolerance is measured, not borrowed — the CPU stand-ins against the oracle
    at exactly these shapes, weights and inputs give a worst rel-L2 of 5.19e-3 (vae) and 3.92e-3 (self) (PROJECTOR_GRAD_REL_CPU = 5.2e-3 / 4.0e-3); the GPU is
    allowed twice that."""
    from tests.test_sd3_model_gpu import _arch
    model, hip, oracle, seen = engine_step(monkeypatch, None, stage, student, dev=DEV, arch=_arch)
    torch.cuda.synchronize()
    share, worst, rg = check_step(model, hip, oracle, seen, 2 * PROJECTOR_GRAD_REL_CPU[stage])
    print(f"[self-transcendence] sd3 {stage} student {student}: share={share:.3e} adapters rel-L2={worst:.3e} projector gradients worst rel-L2={rg:.3e}")


def test_sd3_lora_trajectory_in_stage_self_follows_the_oracles_and_keeps_the_snapshot(monkeypatch):
    """Three optimizer steps of SD3 LoRA through the plugin and the trainer (st355-adamw, stage `self`, student block 1, teacher block 2, weight 0.5, cfg_scale 3)
    against the fp32 oracle stepped by torch.optim.AdamW over the adapters AND the projector, its teacher the oracle run with the starting adapters on the
    conditional and the empty-prompt embeddings.  Stated bounds as tests/test_nextlat_gpu.py's trajectory: |loss difference| <= 2e-3 max(1, |loss|) per step, every
    projector tensor moves by more than lr / 2 and along the oracle's displacement (cosine > 0.7).  The teacher snapshot is bit-identical at the end."""
    import torch.nn.functional as F
    from oracle import sd3 as OS
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_sd3_model_gpu import _arch, _ocfg
    steps, lr, w, student, teacher, scale_cfg = 3, 1e-3, 0.5, 1, 2, 3.0
    cfg = default_config(model_family="sd3", lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, distillation_method="self_transcendence",
                         distillation_config=_dcfg("self", weight=w, cfg_scale=scale_cfg, student_block=student, teacher_block=teacher))
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(3))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    model = plugin.get_trained_component()
    ST.seed_projector(model)
    trainer = Trainer(cfg, plugin, acc)
    cpu, devt = PU.make_inputs(2, 16, 24, 33, 128, 64, DEV, seed=5)
    sig_host = torch.tensor([0.55, 0.62])
    sig = sig_host.to(DEV)
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    g = torch.Generator().manual_seed(19)
    neg_prompt, neg_pooled = (0.5 * torch.randn(cpu["prompt"].shape, generator=g)).to(BF16), (0.5 * torch.randn(cpu["pooled"].shape, generator=g)).to(BF16)
    P, lora, scale = PU.oracle_state(model)
    head0 = {k: P.pop(k).clone() for k in list(P) if k.startswith(PRE)}
    P["pos_embed.pos_embed"] = model.pos_embed.pos_embed.detach().float().cpu()
    names = sorted(lora)
    params = {k: (torch.nn.Parameter(lora[k][0].clone()), torch.nn.Parameter(lora[k][1].clone())) for k in names}
    frozen = {k: (lora[k][0].clone(), lora[k][1].clone()) for k in names}
    hp = [torch.nn.Parameter(head0[PRE + nm].clone()) for nm in ST.NAMES]
    opt = torch.optim.AdamW([t for k in names for t in params[k]] + hp, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    outs = LS.record_sd3_blocks(monkeypatch)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"],
             "negative_prompt_embeds": neg_prompt.to(DEV), "negative_add_text_embeds": neg_pooled.to(DEV)}
    s = sig_host.view(-1, 1, 1, 1)
    noisy = ((1 - s) * cpu["latents"] + s * cpu["noise"]).to(BF16).float()
    target = (cpu["noise"] - cpu["latents"]).to(BF16).float()
    t = sig_host * 1000.0
    start = model.lora_flat.clone()
    hip, ora = [], []
    for _ in range(steps):
        hip.append(trainer.train_step(dict(batch)).item())
        assert [k for k in trainer.last_aux_logs if k.startswith("self_transcendence/")] == ["self_transcendence/loss", "self_transcendence/weight", "self_transcendence/teacher_cfg_scale"]
        opt.zero_grad()
        with torch.no_grad():
            outs.clear()
            OS.sd3_forward(P, _ocfg(model), noisy, cpu["prompt"], cpu["pooled"], t, lora=frozen, lora_scale=scale)
            c = outs[teacher].clone()
            outs.clear()
            OS.sd3_forward(P, _ocfg(model), noisy, neg_prompt.float(), neg_pooled.float(), t, lora=frozen, lora_scale=scale)
            u = outs[teacher].clone()
        outs.clear()
        pred = OS.sd3_forward(P, _ocfg(model), noisy, cpu["prompt"], cpu["pooled"], t, lora={k: params[k] for k in names}, lora_scale=scale)
        guide = ST.guide_autograd(outs[student], hp, "self", (c, u), sig_host, TMIN, TMAX, scale_cfg)
        l = ((pred - target) ** 2).mean(dim=(1, 2, 3)).mean() + w * guide
        l.backward(); opt.step()
        ora.append(l.item())
    torch.cuda.synchronize()
    print(f"[self-transcendence] sd3 LoRA trajectory (self): hip {[round(x, 5) for x in hip]} oracle {[round(x, 5) for x in ora]}")
    assert max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(hip, ora)) <= 2e-3
    assert torch.equal(trainer.distiller.snapshot, start) and not torch.equal(model.lora_flat, start)
    own = dict(model.named_parameters())
    for nm, p_o in zip(ST.NAMES, hp):
        first = head0[PRE + nm]
        mine, theirs = own[PRE + nm].detach().float().cpu() - first, p_o.detach() - first
        assert mine.abs().max() > 0.5 * lr, (nm, mine.abs().max().item(), theirs.abs().max().item())
        cosd = F.cosine_similarity(mine.reshape(1, -1), theirs.reshape(1, -1)).item()
        assert cosd > 0.7, f"{nm}: cosine of the displacement against the oracle's {cosd:.4f}"

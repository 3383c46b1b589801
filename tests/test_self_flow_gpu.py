"""Self-Flow on the MI355X: the kernels of simpletuner_amd/csrc/self_flow.hip and the alignment path's reused kernels against the fp64 restatement
(tests/self_flow_ref.py), element-wise, inside the derived bounds of tests/self_flow_bounds.py; their guard-byte, untouched-rows and determinism contracts; what the
entries refuse; and the SD3 engine on the HIP path — the EMA teacher's capture forward, the tokenwise training forward with the tap, every gradient — against
autograd through the oracle."""
import ctypes as C

import pytest
import torch

from simpletuner_amd import lib, ops
from tests import parity_utils as PU
from tests import self_flow_bounds as SB
from tests import self_flow_ref as SF
from tests import test_sd3_host_sequencing_cpu as SH
from tests.test_self_flow_cpu import CFG, W_ALIGN, check_step, hip_side, oracle_side, record_tap_dx, sd3_model, shadow_of, teacher_features, token_timesteps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
PRE = SF.PREFIX


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["compact", "strided"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("ratio", SB.VIEW_RATIOS)
@pytest.mark.parametrize("shape", SB.VIEW_SHAPES)
def test_views_kernel_is_inside_the_derived_bounds_repeats_and_keeps_the_guards(shape, ratio, dtype, strided):
    """(1, 16, 2, 2): a single token, one vector row of lanes; (3, 16, 6, 10): image rows of 10 elements, so a lane's 8 / 4 elements cross rows and tokens; samples
    with sigma_alt above, below and equal to sigma; inputs with a batch stride inside guard buffers, every output carved from one"""
    worst = SB.check_views_case(ops, DEV, shape, ratio, dtype, strided)
    torch.cuda.synchronize()
    print(f"[self-flow] views {shape} ratio {ratio} {str(dtype)[6:]} {'strided' if strided else 'compact'}: worst ratio to the bound "
          f"student {worst['noisy_student']:.3f} teacher {worst['noisy_teacher']:.3f}")


@pytest.mark.parametrize("D,B,S,strided", SB.HEAD_CASES)
def test_head_and_align_path_is_inside_the_derived_bounds_and_repeats(D, B, S, strided):
    """D = 128: a partial first pass of the row kernels, two fold tiles a side, half a wgrad chunk; D = 1536: three passes, 24 tiles, six chunks.  M = 30 is no multiple
    of the row kernels' 4 rows per block, of 16 or of 64 (the TN GEMM reads the zero tail of the 64-row parents); M = 64 is.  The teacher: compact, or a view with
    its own batch stride."""
    worst, _ = SB.check_head_case(ops, DEV, D, B, S, strided)
    torch.cuda.synchronize()
    print(f"[self-flow] head D {D} M {B * S} {'strided' if strided else 'compact'} teacher: worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_entries_refuse_their_preconditions_and_launch_nothing():
    from simpletuner_amd.lib import St355Error
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    v = z(1, dt=F32)
    with pytest.raises(St355Error, match=r"H % patch_size != 0 or W % patch_size != 0"):
        ops.self_flow_views(z(1, 16, 3, 2), z(1, 16, 3, 2), v, v, v, v, z(1, 1, 1, dt=F32), 0.1, 2)
    with pytest.raises(St355Error, match=r"H % patch_size != 0 or W % patch_size != 0"):
        ops.self_flow_views(z(1, 16, 2, 5), z(1, 16, 2, 5), v, v, v, v, z(1, 1, 2, dt=F32), 0.1, 2)
    for bad in (lambda: ops.self_flow_views(z(1, 16, 2, 2), z(1, 16, 2, 2), v, v, v, v, z(1, 1, 1, dt=F32), 0.6, 2),                        # ratio
                lambda: ops.self_flow_views(z(1, 16, 2, 2), z(1, 16, 2, 2, dt=F32), v, v, v, v, z(1, 1, 1, dt=F32), 0.1, 2),                # mixed dtypes
                lambda: ops.self_flow_views(z(1, 3, 2, 2), z(1, 3, 2, 2), v, v, v, v, z(1, 1, 1, dt=F32), 0.1, 2),                          # 12 elements: no multiple of 8
                lambda: ops.self_flow_views(z(65)[1:].view(1, 16, 2, 2), z(1, 16, 2, 2), v, v, v, v, z(1, 1, 1, dt=F32), 0.1, 2),          # off a 16-byte boundary
                lambda: ops.self_flow_views(z(1, 16, 2, 2), z(1, 16, 2, 2), z(2, dt=F32), v, v, v, z(1, 1, 1, dt=F32), 0.1, 2),            # [B] vectors
                lambda: ops.self_flow_fold(z(72, dt=F32), z(72, dt=F32), z(72, 72, dt=F32), z(72, dt=F32), z(72, 72), z(72, 64), z(72)),    # WfT's shape
                lambda: ops.self_flow_fold(z(68, dt=F32), z(68, dt=F32), z(68, 68, dt=F32), z(68, dt=F32), z(68, 68), z(68, 68), z(68)),    # D % 8
                lambda: ops.self_flow_rows(z(2, 5, 72), z(10, 72), z(10, dt=F32)),                                                           # D % 64: the GEMM's granule
                lambda: ops.self_flow_rows(z(2, 5, 128), z(10, 128), z(9, dt=F32)),                                                          # rstd's length
                lambda: ops.self_flow_wgrad(z(64, 64), z(64, dt=F32), z(64, dt=F32), z(64, dt=F32), z(64, 64, dt=F32), 0.5, z(64, dt=F32), z(64, dt=F32),
                                            z(64, 64, dt=F32), z(64, dt=F32))):                                                                # a host scale
        with pytest.raises(St355Error):
            bad()
    # the C entries themselves: ST355_EINVAL with the reason, and nothing launched — the outputs keep their sentinel
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lat, out = z(1, 16, 3, 2), torch.full((2, 96), 7.0, dtype=BF16, device=DEV)
    tok, sT, tT = (torch.full((4,), 7.0, dtype=F32, device=DEV) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())
    u = z(1, 1, 1, dt=F32)
    for H, W, ratio, text in ((3, 2, 0.1, "H % patch_size != 0 or W % patch_size != 0"), (2, 3, 0.1, "H % patch_size != 0 or W % patch_size != 0"),
                              (2, 2, 0.75, "mask ratio must lie in [0, 0.5]")):
        rc = L.st355_self_flow_views(st, p(lat), p(lat), 1, 96, 96, p(v), p(v), p(v), p(v), p(u), ratio, 2, p(out[0]), p(out[1]), p(tok), p(sT), p(tT), None, 1, 16, H, W)
        assert rc != 0 and text in L.st355_last_error().decode()
    rc = L.st355_self_flow_rows(st, p(z(2, 5, 68)), p(z(10, 68)), p(z(10, dt=F32)), 2, 5, 68, 68, 340)
    assert rc != 0 and "D must be a multiple of 8" in L.st355_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (tok == 7.0).all() and (sT == 7.0).all() and (tT == 7.0).all()


# ------------------------------------------------------------------------------------------------
# the SD3 engine on the HIP path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ckpt", ["plain", "segmented"])
def test_sd3_step_with_self_flow_matches_the_oracle(monkeypatch, ckpt):
    """One tiny SD3 LoRA step through the C ABI: the EMA teacher's capture forward (adapter operands packed from a shadow that has moved, the masters untouched),
    the tokenwise training forward with the tap at block 1 against the teacher's block 2, weight 4 (the regulariser's share of the adapters' gradient asserted),
    against autograd through the oracle — tests/test_self_flow_cpu.py's check_step: prediction, loss, similarity, every adapter gradient, the four projector
    gradients, dX at the student block."""
    from tests.test_sd3_model_gpu import _arch
    model = sd3_model(None, None, 3, 1, 2, dev=DEV, arch=_arch)
    if ckpt != "plain":
        model.enable_gradient_checkpointing()
        model.set_gradient_checkpointing_interval(2)
    d = SH._inputs(2, 16, 24, 33)
    tok, t_T = token_timesteps(2, 8 * 12)
    masters = model.lora_flat.clone()
    feats = teacher_features(model, d, shadow_of(model), t_T, 2)
    assert torch.equal(masters, model.lora_flat) and feats.is_contiguous() and feats.dtype == BF16
    seen = record_tap_dx(monkeypatch)
    hip = hip_side(model, d, tok, feats, W_ALIGN)
    torch.cuda.synchronize()
    share, worst, rg = check_step(model, hip, oracle_side(monkeypatch, model, d, tok, feats, 1, W_ALIGN), seen)
    print(f"[self-flow] sd3 lora {ckpt}: sim hip={hip[2].item():.6f} share={share:.3e} adapters worst rel_l2={worst:.3e} projector worst rel_l2={rg:.3e}")


def test_trainer_steps_with_the_ema_teacher_on_the_device():
    """Trainer.train_step, three steps, st355-adamw with the EMA fused into its launch: the views kernel in prepare_batch, the teacher forward from the flat shadow,
    the logs; the loss stays finite, the projector and the shadow move, and a step whose scheduler weight is 0 leaves the projector's gradient zero"""
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests.test_sd3_model_gpu import _arch, _batch
    cfg = default_config(model_family="sd3", lora_rank=8, train_batch_size=2, seed=3, lora_init_b_std=0.02, learning_rate=1e-3, flow_schedule_shift=3.0,
                         **{**CFG, "crepa_self_flow_mask_ratio": 0.25, "crepa_cutoff_step": 2})
    acc = St355Accelerator(DEV)
    plugin = SD3(cfg, acc)
    plugin.load_model(**_arch(3))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    SF.seed_projector(comp)
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(2, 16, 24, 33, 128, 64, DEV, seed=3)
    lo, hi = comp._sf.flat_lo, comp._sf.flat_hi
    head0, losses = comp.lora_flat[lo:hi].clone(), []
    for step in range(3):
        losses.append(trainer.train_step(_batch(devt)).item())
        logs = trainer.last_aux_logs
        assert logs["crepa_cutoff"] is (step >= 2) and -1.0 <= logs["crepa_alignment_score"] <= 1.0
        if step == 1:
            head1 = comp.lora_flat[lo:hi].clone()
    torch.cuda.synchronize()
    assert all(x == x and abs(x) < 1e3 for x in losses)
    sh = trainer.ema_model.shadow_flat
    assert not torch.equal(head0, head1) and not torch.equal(sh, comp.lora_flat[:sh.numel()])
    assert comp._last_grad_flat[lo:hi].abs().max().item() == 0.0          # the cutoff step: nothing reached the projector

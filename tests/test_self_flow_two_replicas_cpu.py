"""Self-Flow at world size 2: the `gloo` run of the real training loop on the CPU (tests/test_trainer_two_replicas_cpu.py's form, kernels replaced by the emulator and
the stand-ins of tests/self_flow_ref.py) with the SD3 engine, `crepa_enabled` / `crepa_feature_source=self_flow` and a moving EMA teacher — two replicas, each with
half of a batch, against one process with the whole batch.  Every sample has the same token count, so the mean of the replicas' mean cosines is the whole batch's; the
projector's range of the gradient arena is handed to the exchange like the adapters' (SelfFlowTap.backward), and the replicas start from rank 0's projector."""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

STEPS = 3


def _run(rank, world):
    import pytest
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    from tests import self_flow_ref as SF
    from tests import test_sd3_host_sequencing_cpu as SH
    patch = pytest.MonkeyPatch()
    SF.install(patch)
    B = 2 // world
    cfg = default_config(model_family="sd3", train_batch_size=B, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, crepa_enabled=True,
                         crepa_feature_source="self_flow", crepa_block_index=0, crepa_teacher_block_index=1, crepa_lambda=0.5, crepa_self_flow_mask_ratio=0.25, use_ema=True,
                         ema_decay=0.9)
    acc = St355Accelerator(torch.device("cpu"))
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    with torch.no_grad():
        for p in plugin.model.parameters():
            p.add_(0.01 * rank)                                   # replicas deliberately start apart: the constructor must bring them to rank 0's weights
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    comp = plugin.get_trained_component()
    with torch.no_grad():                                         # ... the projector too
        comp.lora_flat[comp._sf.flat_lo:comp._sf.flat_hi].add_(0.01 * rank)
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    g = torch.Generator().manual_seed(17)
    alt = torch.rand(2, generator=g) * 0.8 + 0.1
    extra = {"alt": alt, "alt_t": alt * 1000.0, "uniforms": torch.rand(2, 8, 4, generator=g)}
    mine = {k: v[rank * B:(rank + 1) * B] for k, v in {**devt, **extra}.items()}
    sig = mine["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    losses, sims = [], []
    for _ in range(STEPS):
        losses.append(float(trainer.train_step({"latent_batch": mine["latents"], "prompt_embeds": mine["prompt"], "add_text_embeds": mine["pooled"], "noise": mine["noise"],
                                                "crepa_alt_sigmas": mine["alt"], "crepa_alt_timesteps": mine["alt_t"], "crepa_self_flow_uniforms": mine["uniforms"]})))
        sims.append(trainer.last_aux_logs["crepa_alignment_score"])
    flat, shadow = comp.lora_flat.clone(), trainer.ema_model.shadow_flat.clone()
    patch.undo()
    return flat, shadow, losses, sims, comp.grad_sync is not None, comp._sf.flat_lo


def _worker(rank, world, init_file, out_dir):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    flat, shadow, losses, sims, has_sync, lo = _run(rank, world)
    torch.save({"flat": flat, "shadow": shadow, "losses": losses, "sims": sims, "has_sync": has_sync, "lo": lo}, os.path.join(out_dir, f"self_flow_{rank}.pt"))
    dist.destroy_process_group()


def test_two_self_flow_replicas_equal_one_process_with_the_whole_batch():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"self_flow_{r}.pt")) for r in range(2))
    one, shadow_one, losses_one, sims_one, _, lo = _run(0, 1)
    assert r0["has_sync"] and r1["has_sync"]
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["shadow"], r1["shadow"]), "replicas must hold identical adapters, projector and EMA teacher after every step"
    assert r0["losses"] == r1["losses"]
    assert max(abs(a - b) for a, b in zip(r0["losses"], losses_one)) < 2e-3    # == the whole batch's loss
    # the whole batch's similarity is the mean of the two halves' (equal token counts)
    assert max(abs(0.5 * (a + b) - c) for a, b, c in zip(r0["sims"], r1["sims"], sims_one)) < 2e-3
    # weights after K steps: Adam's update is lr * sign-like, so the two runs may differ by a few lr per element where a gradient is rounding noise
    diff = (r0["flat"].float() - one.float()).abs().max().item()
    assert diff <= 2.05 * 1e-3 * STEPS, diff
    assert one.numel() - lo > 0 and not torch.equal(r0["flat"][lo:], one[lo:] * 0)          # the projector is part of the exchanged arena

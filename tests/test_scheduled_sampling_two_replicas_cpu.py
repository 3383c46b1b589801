"""Scheduled sampling with ReflexFlow at world size 2: the `gloo` run of the real training loop on the CPU (tests/test_dora_two_replicas_cpu.py's form, kernels replaced by
the emulator and the stand-ins of tests/reflexflow_ref.py) with the SD3 engine — two replicas, each with half of a batch and ITS OWN plan, against one process with the
whole batch and both plans.  The rollout is local to a rank (no collective inside it); the per-sample loss terms make the batch mean separable."""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

STEPS = 2
OFFSETS = (2, 1)


def _run(rank, world):
    import pytest
    from simpletuner_amd.scheduled_sampling import ScheduledSamplingPlan
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU
    from tests import reflexflow_ref as RR
    from tests import test_sd3_host_sequencing_cpu as SH
    patch = pytest.MonkeyPatch()
    RR.install(patch)
    B = 2 // world
    cfg = default_config(model_family="sd3", train_batch_size=B, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, scheduled_sampling_max_step_offset=2)
    acc = St355Accelerator(torch.device("cpu"))
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(2, 8, 8, 24, 128, 64, "cpu", seed=3)
    mine = {k: v[rank * B:(rank + 1) * B] for k, v in devt.items()}
    sig = mine["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    base = (sig * 1000.0).long()
    off = torch.tensor(OFFSETS[rank * B:(rank + 1) * B])
    losses = []
    for _ in range(STEPS):
        plan = ScheduledSamplingPlan(target_timesteps=base, source_timesteps=torch.clamp(base + off, max=999), rollout_steps=off)
        losses.append(float(trainer.train_step({"latent_batch": mine["latents"], "prompt_embeds": mine["prompt"], "add_text_embeds": mine["pooled"], "noise": mine["noise"],
                                                "scheduled_sampling_plan": plan})))
    comp = plugin.get_trained_component()
    flat = comp.lora_flat.clone()
    logs = trainer.last_aux_logs
    patch.undo()
    return flat, losses, comp.grad_sync is not None, logs


def _worker(rank, world, init_file, out_dir):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    flat, losses, has_sync, logs = _run(rank, world)
    torch.save({"flat": flat, "losses": losses, "has_sync": has_sync, "logs": logs}, os.path.join(out_dir, f"ss_{rank}.pt"))
    dist.destroy_process_group()


def test_two_replicas_with_a_plan_per_rank_equal_one_process_with_the_whole_batch():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"ss_{r}.pt")) for r in range(2))
    one, losses_one, _, _ = _run(0, 1)
    assert r0["has_sync"] and r1["has_sync"]
    assert torch.equal(r0["flat"], r1["flat"]), "replicas must hold identical adapters after every synchronised step"
    assert r0["losses"] == r1["losses"]                                          # the gathered, sample-weighted loss
    assert "reflexflow_adr" in r0["logs"] and "reflexflow_adr" in r1["logs"]
    assert max(abs(a - b) for a, b in zip(r0["losses"], losses_one)) < 2e-3 * max(1.0, max(losses_one))    # == the whole batch's loss (tests/test_dora_two_replicas_cpu.py's bound, relative to a loss of order 20)
    # weights after K steps: Adam's update is lr * sign-like, so the two runs may differ by a few lr per element where a gradient is rounding noise
    diff = (r0["flat"].float() - one.float()).abs().max().item()
    assert diff <= 2.05 * 1e-3 * STEPS, diff

"""Flow-DPO at world size 2: the `gloo` run of the real training loop on the CPU (tests/test_scheduled_sampling_two_replicas_cpu.py's form, kernels replaced by the
emulator and the stand-ins of tests/flow_dpo_ref.py) with the SD3 engine — two replicas, each with ONE pair of a 2-pair batch.  The auto-beta EMA follows the rank
mean of mean_b |margin_b| (one all_reduce of a device scalar between the head's two launches), so both ranks hold the same EMA and the same beta, and the
replicas hold identical adapters after every synchronised step."""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

STEPS = 2


def _run(rank, world):
    import pytest
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import flow_dpo_ref as FR
    from tests import parity_utils as PU
    from tests import test_sd3_host_sequencing_cpu as SH
    patch = pytest.MonkeyPatch()
    FR.install(patch)
    B = 2 // world
    cfg = default_config(model_family="sd3", train_batch_size=B, seed=3, lora_rank=8, lora_init_b_std=0.5, learning_rate=1e-3, distillation_method="flow_dpo",
                         distillation_config={"flow_dpo": dict(norm_type="mean", auto_beta=True, auto_beta_decay=0.5, auto_beta_max=1000.0)})
    acc = St355Accelerator(torch.device("cpu"))
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(2, 8, 8, 24, 128, 64, "cpu", seed=3)
    lose = torch.randn(devt["latents"].shape, generator=torch.Generator().manual_seed(103)).to(torch.bfloat16)
    mine = {k: v[rank * B:(rank + 1) * B] for k, v in dict(devt, lose=lose).items()}
    sig = mine["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    losses, emas, betas, margins = [], [], [], []
    for _ in range(STEPS):
        losses.append(float(trainer.train_step({"latent_batch": mine["latents"], "prompt_embeds": mine["prompt"], "add_text_embeds": mine["pooled"], "noise": mine["noise"],
                                                "conditioning_latents": mine["lose"], "conditioning_type": "reference_strict"})))
        emas.append(trainer.distiller.margin_ema)
        betas.append(trainer.last_aux_logs["flow_dpo_beta"])
        margins.append(trainer.last_aux_logs["flow_dpo_margin"])
    comp = plugin.get_trained_component()
    flat = comp.lora_flat.clone()
    patch.undo()
    return dict(flat=flat, losses=losses, has_sync=comp.grad_sync is not None, emas=emas, betas=betas, margins=margins)


def _worker(rank, world, init_file, out_dir):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    torch.save(_run(rank, world), os.path.join(out_dir, f"dpo_{rank}.pt"))
    dist.destroy_process_group()


def test_two_replicas_hold_the_same_auto_beta_ema_and_identical_adapters():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"dpo_{r}.pt")) for r in range(2))
    one = _run(0, 1)
    assert r0["has_sync"] and r1["has_sync"]
    assert r0["emas"] == r1["emas"] and r0["betas"] == r1["betas"] and None not in r0["emas"]          # the EMA is equal on both ranks, bit for bit
    assert r0["margins"] != r1["margins"]                                                              # (each rank saw its own pair)
    assert torch.equal(r0["flat"], r1["flat"]), "replicas must hold identical adapters after every synchronised step"
    # the rank mean of the per-rank means is the whole batch's mean (one pair per rank): the single process with both pairs sees the same EMA up to fp32 rounding
    assert all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(r0["emas"], one["emas"])), (r0["emas"], one["emas"])
    assert r0["losses"] == r1["losses"] and max(abs(a - b) for a, b in zip(r0["losses"], one["losses"])) < 2e-3 * max(1.0, max(one["losses"]))

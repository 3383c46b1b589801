"""DoRA at world size 2: the `gloo` run of the real training loop on the CPU (tests/test_trainer_two_replicas_cpu.py's form, kernels replaced by the emulator and the
stand-ins of tests/dora_ref.py) with the SD3 engine and `use_dora` — two replicas, each with half of a batch, against one process with the whole batch.  The magnitudes'
range of the gradient arena is handed to the exchange like the adapters' (LoraGroup._grads_dora), and the replicas start from rank 0's magnitudes."""
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
    from tests import dora_ref as DR
    from tests import parity_utils as PU
    from tests import test_sd3_host_sequencing_cpu as SH
    patch = pytest.MonkeyPatch()
    DR.install(patch)
    B = 2 // world
    cfg = default_config(model_family="sd3", train_batch_size=B, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3)
    cfg.use_dora = True
    acc = St355Accelerator(torch.device("cpu"))
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    with torch.no_grad():
        for p in plugin.model.parameters():
            p.add_(0.01 * rank)                                   # replicas deliberately start apart: the constructor must bring them to rank 0's weights
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    trainer = Trainer(cfg, plugin, acc)
    _, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    mine = {k: v[rank * B:(rank + 1) * B] for k, v in devt.items()}
    sig = mine["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    losses = []
    for _ in range(STEPS):
        losses.append(float(trainer.train_step({"latent_batch": mine["latents"], "prompt_embeds": mine["prompt"], "add_text_embeds": mine["pooled"], "noise": mine["noise"]})))
    comp = plugin.get_trained_component()
    flat = comp.lora_flat.clone()
    m_lo = min(g.dora.flat_lo for g in comp.lora_groups)
    patch.undo()
    return flat, losses, comp.grad_sync is not None, m_lo


def _worker(rank, world, init_file, out_dir):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    flat, losses, has_sync, m_lo = _run(rank, world)
    torch.save({"flat": flat, "losses": losses, "has_sync": has_sync, "m_lo": m_lo}, os.path.join(out_dir, f"dora_{rank}.pt"))
    dist.destroy_process_group()


def test_two_dora_replicas_equal_one_process_with_the_whole_batch():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"dora_{r}.pt")) for r in range(2))
    one, losses_one, _, m_lo = _run(0, 1)
    assert r0["has_sync"] and r1["has_sync"]
    assert torch.equal(r0["flat"], r1["flat"]), "replicas must hold identical adapters and magnitudes after every synchronised step"
    assert r0["losses"] == r1["losses"]
    assert max(abs(a - b) for a, b in zip(r0["losses"], losses_one)) < 2e-3    # == the whole batch's loss
    # weights after K steps: Adam's update is lr * sign-like, so the two runs may differ by a few lr per element where a gradient is rounding noise
    diff = (r0["flat"].float() - one.float()).abs().max().item()
    assert diff <= 2.05 * 1e-3 * STEPS, diff
    n_m = one.numel() - m_lo
    assert n_m > 0 and not torch.equal(r0["flat"][m_lo:], torch.zeros(n_m))          # the magnitudes are part of the exchanged arena

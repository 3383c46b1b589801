"""Evaluation loss (eval_steps_interval / eval_epoch_interval) on the CPU: (a) the host rules against the EXECUTED reference (tests/golden/eval_loss_vectors.pt, written
by tools/gen_eval_loss_golden.py): the timestep grid, the custom-timestep batch with its dtype chain, would_evaluate, the tracker table, the num_eval_images quirk and
pooled versus per-dataset passes; (b) the stand-ins of the two new ops inside the kernels' derived bounds; (c) the pass through the emulator on the tiny SD3 and
tiny Flux engines against the fp64 oracle, stacked and not, and that it does not move training; (d) the refusals by their full text; (e) flag absent."""
import logging
import os
import sys
import tempfile
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import flux as OF
from oracle import sd3 as OS
from oracle import train_math as TM
from tests import eval_loss_bounds as EB
from tests import eval_loss_ref as ER
from tests import parity_utils as PU
from tests import test_sd3_host_sequencing_cpu as SH

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = SimpleNamespace
DT = {"torch.float32": F32, "torch.bfloat16": BF16}


@pytest.fixture(scope="module")
def G():
    return torch.load(os.path.join(ROOT, "tests", "golden", "eval_loss_vectors.pt"), weights_only=False)


def _ev(cfg, main=True, sets=None):
    from simpletuner_amd.training.evaluation import Evaluation
    return Evaluation(NS(**cfg), NS(is_main_process=main, device=torch.device("cpu")), sets or {})


def _schedulers():
    from simpletuner_amd.sampling import FlowMatchEulerDiscreteScheduler, fix_flow_match_euler_schedule_bounds
    return {"shift1": lambda: fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=1.0)),
            "shift3": lambda: fix_flow_match_euler_schedule_bounds(FlowMatchEulerDiscreteScheduler(shift=3.0)),
            "dynamic": lambda: FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=True)}


def _mu_model():
    """a plugin as far as `calculate_dynamic_shift_mu` reads it: a trained component whose config carries patch_size 2"""
    from simpletuner_amd.sd3.model import SD3
    m = SD3.__new__(SD3)
    m.config = NS()
    m.model = NS(config=NS(patch_size=2))
    return m


# ------------------------------------------------------------------------------------------------
# (a) the host rules against the executed reference
# ------------------------------------------------------------------------------------------------
def test_timestep_grid_equals_the_executed_reference_with_and_without_dynamic_shift(G):
    for name, rec in G["schedule"]["grids"].items():
        ev = _ev(dict(eval_timesteps=rec["eval_timesteps"]))
        sched = _schedulers()[rec["scheduler"]]()
        ts = ev.get_timestep_schedule(sched, latents=torch.zeros(1, 16, *rec["hw"]), model=_mu_model())
        assert ts.dtype == rec["timesteps"].dtype and torch.equal(ts, rec["timesteps"]) and torch.equal(sched.sigmas, rec["sigmas"]), name
        if rec["mu"] is not None:
            assert _mu_model().calculate_dynamic_shift_mu(sched, torch.zeros(1, 16, *rec["hw"])) == rec["mu"], name
    ev = _ev(dict(eval_timesteps=4))
    for model, lat, key in ((None, torch.zeros(1, 16, 16, 16), "no_model"), (_mu_model(), None, "no_latents")):
        with pytest.raises(ValueError) as ei:
            ev.get_timestep_schedule(_schedulers()["dynamic"](), latents=lat, model=model)
        assert str(ei.value) == G["schedule"]["errors"][key] == "Flow scheduler requires `mu` for dynamic shifting but none could be derived."


def test_the_pass_recomputes_the_grid_when_the_latent_size_changes(monkeypatch):
    """dynamic shifting: mu follows H x W, so a second bucket gets its own grid (validation.py:5566-5570), an equal one does not"""
    from simpletuner_amd.training import evaluation as EV
    sets = {"a": [{"hw": (16, 16)}, {"hw": (16, 16)}, {"hw": (32, 48)}]}
    ev = _ev(dict(eval_timesteps=4, eval_dataset_pooling=True, num_eval_images=None), sets=sets)
    model = _mu_model()
    model._noise_step = model._noise_offset = 0
    model.prepare_batch = lambda raw, state: {"latents": torch.zeros(2, 16, *raw["hw"], dtype=BF16), "timesteps": torch.zeros(2)}
    calls = []
    real = ev.get_timestep_schedule
    monkeypatch.setattr(ev, "get_timestep_schedule", lambda s, latents=None, model=None: calls.append(tuple(latents.shape[-2:])) or real(s, latents=latents, model=model))
    monkeypatch.setattr(EV.Evaluation, "_evaluate_batch", lambda self, model, prepared, grid, row, k: row.fill_(1.0))
    out = ev.execute_eval(model, _schedulers()["dynamic"]())
    assert calls == [(16, 16), (32, 48)]
    # two grids of four timesteps that share their first value (sigma 1 shifts to 1): 7 keys; 3 batches x 4 entries
    assert len(out["pooled"]) == 7 and len(out["pooled"][1000.0]) == 3 and sum(len(v) for v in out["pooled"].values()) == 12


@pytest.mark.parametrize("dn", ["bf16", "fp32"])
def test_custom_timestep_batch_equals_the_executed_reference_dtype_chain_included(G, dn, monkeypatch):
    """timesteps and sigmas bit for bit (the chain: grid value -> weight dtype -> / 1000 and clamp in the latents' dtype -> x 1000 in the latents' dtype -> the prepared
    timesteps' dtype); the noisy rows of the kernel contract (fp32 arithmetic on that sigma, ONE rounding) against the reference's rows (g = 1 - s, g x, s n and the sum
    each rounded to the latents' dtype: four roundings) within eps (2 |(1 - s) x| + |s n| + 2 |y|), eps the latents' dtype's"""
    from simpletuner_amd.training.evaluation import prepare_custom_timestep_batch
    seen = 0
    for name, rec in G["custom_batch"].items():
        if not name.startswith(dn + "."):
            continue
        dtype = DT[rec["dtype"]]
        prepared = {"latents": rec["latents"], "noise": rec["noise"], "timesteps": rec["prepared_timesteps"], "sigmas": rec["prepared_sigmas"]}
        got = prepare_custom_timestep_batch(prepared, rec["grid"], 1000.0, dtype)
        rs, rt = ER.dtype_chain(rec["grid"], dtype, dtype, rec["prepared_timesteps"].dtype)
        assert got["sigmas"].dtype == dtype and got["timesteps"].dtype == rec["prepared_timesteps"].dtype
        assert torch.equal(got["sigmas"], rs) and torch.equal(got["timesteps"], rt), name
        eps = float(torch.finfo(dtype).eps)
        for j, st in enumerate(rec["steps"]):
            assert st["sigmas"].dtype == dtype and st["sigmas"].shape == rec["prepared_sigmas"].shape and st["timesteps"].dtype == got["timesteps"].dtype
            assert torch.equal(st["sigmas"].flatten(), got["sigmas"][j].expand(2)) and torch.equal(st["timesteps"], got["timesteps"][j].expand(2)), (name, j)
            assert torch.equal(st["given"].float(), rec["grid"][j].to(dtype).float().expand(2))
            s = float(got["sigmas"][j])
            x, n = rec["latents"].double(), rec["noise"].double()
            y = (1 - s) * x + s * n
            tol = eps * (2 * ((1 - s) * x).abs() + (s * n).abs() + 2 * y.abs()) + 1e-30
            assert bool(((st["noisy_latents"].double() - y).abs() <= tol).all()), (name, j)
            if dtype == BF16:
                view = ER.eval_flow_views(rec["latents"], rec["noise"], got["sigmas"][j:j + 1].float())[0]
                assert bool(((view.double() - st["noisy_latents"].double()).abs() <= tol).all()), (name, j)
            seen += 1
    assert seen >= 39


def test_a_grid_value_of_at_most_one_is_taken_as_a_sigma(G):
    """the reference decides "timestep or sigma" per call: the unshifted grid's last value, timestep 1.0, becomes sigma 1.0 and reaches the model as 1.0 (kept)"""
    from simpletuner_amd.training.evaluation import prepare_custom_timestep_batch
    rec = G["custom_batch"]["bf16.shift1.T4"]
    assert float(rec["grid"][-1]) == 1.0 and float(rec["steps"][-1]["sigmas"].flatten()[0]) == 1.0 and float(rec["steps"][-1]["timesteps"][0]) == 1.0
    got = prepare_custom_timestep_batch({"latents": rec["latents"], "timesteps": rec["prepared_timesteps"]}, rec["grid"])
    assert float(got["sigmas"][-1]) == 1.0 and float(got["timesteps"][-1]) == 1.0 and float(got["timesteps"][0]) == 1000.0


def test_rounded_timesteps_of_the_default_grid_stay_distinct(G):
    """what executing the reference shows: the 28-step grid at shift 3 reaches the model as bf16 numbers (987.355 -> 988), each sigma is bf16(t / 1000), and the
    28 values stay distinct"""
    rec = G["custom_batch"]["bf16.shift3.T28"]
    ts = [float(s["timesteps"][0]) for s in rec["steps"]]
    assert len(set(ts)) == 28 and ts[1] == 988.0 and abs(float(rec["grid"][1]) - 987.355) < 1e-3
    assert float(rec["steps"][1]["sigmas"].flatten()[0]) == 0.98828125


def test_would_evaluate_equals_the_executed_reference(G, caplog):
    for name, run in G["would"].items():
        caplog.clear()
        ev = _ev(run["config"], main=run["main"])
        with caplog.at_level(logging.WARNING, logger="simpletuner_amd.training.evaluation"):
            got = [ev.would_evaluate(dict(s)) for s in run["states"]]
        assert got == run["answers"], (name, got, run["answers"])
        assert [r.getMessage() for r in caplog.records] == run["warnings"], name
    assert any(G["would"]["steps3_resume4"]["answers"]) and sum(G["would"]["both"]["answers"]) == 5


def test_tracker_table_equals_the_executed_reference(G):
    for name, rec in G["table"].items():
        got = _ev({}, main=name != "not_main").generate_tracker_table(rec["given"])
        assert got == rec["table"], (name, got, rec["table"])
    assert G["table"]["two_sets"]["table"] == {"loss/val/a": 1.0, "loss/val/b": 1.4583333333333333}


def _stub_pass(monkeypatch, G, pooling, cap, k=1):
    from simpletuner_amd.training import evaluation as EV
    stub = G["stub"]
    ev = _ev(dict(eval_timesteps=4, eval_dataset_pooling=pooling, num_eval_images=cap, eval_timestep_stack=k), sets=G["passes"]["sets"])
    model = NS(_noise_step=7, _noise_offset=4096, config=NS(flow_schedule_shift=3.0), noise_schedule=None)

    def prepare_batch(raw, state):
        torch.rand(3)
        return {"latents": torch.zeros(2, 4, *raw["hw"], dtype=BF16), "timesteps": torch.zeros(2), "id": raw["id"]}
    model.prepare_batch = prepare_batch
    seen = []

    def evaluate_batch(self, model, prepared, grid, row, k):
        given = grid["given"]
        seen.extend((prepared["id"], float(t)) for t in given)
        row.copy_(stub["base"] * (1 + prepared["id"]) + stub["scale"] * given.double())
    monkeypatch.setattr(EV.Evaluation, "_evaluate_batch", evaluate_batch)
    torch.manual_seed(1234)
    before = torch.get_rng_state().clone()
    acc = ev.execute_eval(model, ev.noise_scheduler_of(model))
    assert torch.equal(before, torch.get_rng_state()) and (model._noise_step, model._noise_offset) == (7, 4096) and not hasattr(model, "_eval_noise_seed")
    return ev, acc, seen


@pytest.mark.parametrize("pooling", [True, False])
@pytest.mark.parametrize("cap", [None, 1, 2, 4, 9])
def test_passes_equal_the_executed_reference_num_eval_images_caps_batches_and_per_dataset_mode_returns_no_pooled_table(monkeypatch, G, pooling, cap):
    run = G["passes"]["runs"][f"pooling{int(pooling)}.cap{cap}"]
    ev, acc, seen = _stub_pass(monkeypatch, G, pooling, cap)
    assert list(acc) == run["names"] and ("pooled" in acc) == pooling
    assert seen == [(i, t) for i, t, mask, grad in run["seen"]] and all(not mask and not grad for _, _, mask, grad in run["seen"])
    for name, entries in run["entries"].items():
        got = sorted((t, v) for t, vals in acc[name].items() for v in vals)
        assert len(got) == len(entries)
        for (t0, v0), (t1, v1) in zip(got, entries):
            assert t0 == t1 and abs(v0 - v1) <= 2.0 ** -23 * max(1.0, abs(v1)), (name, t0, v0, v1)          # the table holds fp32 values
    table = ev.generate_tracker_table(acc)
    assert set(table) == set(run["table"]) and all(abs(table[k] - v) <= 2.0 ** -22 * max(1.0, abs(v)) for k, v in run["table"].items())
    if cap == 2 and pooling:
        assert len(seen) == 2 * 4          # the quirk: num_eval_images=2 evaluates two BATCHES (of two images each)


# ------------------------------------------------------------------------------------------------
# (b) the stand-ins inside the kernels' bounds
# ------------------------------------------------------------------------------------------------
def _rows(B, n, K, seed):
    g = torch.Generator().manual_seed(seed)
    lat, noise = torch.randn(B, n, generator=g).to(BF16), torch.randn(B, n, generator=g).to(BF16)
    pred = (torch.randn(K, B, n, generator=g) * 1.5).to(BF16)
    sigma = torch.rand(K, generator=g)
    sigma[-1] = 1.0
    sigma[0] = 0.0
    return lat, noise, pred, sigma


@pytest.mark.parametrize("B,n,K", [(1, 8, 1), (3, 2056, 3), (2, 4096, 7)])
def test_stand_ins_sit_inside_the_derived_bounds_and_round_once(B, n, K):
    lat, noise, pred, sigma = _rows(B, n, K, 5 + K)
    out = ER.eval_flow_views(lat, noise, sigma)
    ref, tol = EB.views_ref(lat, noise, sigma)
    ok, worst = EB.inside(out, ref, tol)
    assert ok and out.shape == (K, B, n) and out.dtype == BF16, worst
    assert torch.equal(out[0], lat) and (K == 1 or torch.equal(out[-1], noise))          # sigma 0 and 1 are exact
    target = (noise.float() - lat.float()).to(BF16)
    g = torch.Generator().manual_seed(9)
    for lt, c in (("l2", None), ("huber", 0.1), ("smooth_l1", 0.1), ("huber", torch.rand(K * B, generator=g) * 0.5 + 0.01), ("smooth_l1", torch.rand(K * B, generator=g) + 0.01)):
        loss, per = ER.eval_loss(pred, target, lt, c)
        r = EB.loss_ref(pred, target, lt, c)
        assert EB.inside(loss, *r["loss"])[0] and EB.inside(per, *r["per_sample"])[0], lt
        o_loss, o_per = TM.conditional_loss(pred[0].float(), target.float(), lt, c if not torch.is_tensor(c) else c[:B])
        assert abs(float(loss[0]) - float(o_loss)) < 1e-5 * max(1.0, float(o_loss))          # the restatement is the oracle's conditional_loss
        # a bound that a wrong formula would miss: the other loss types sit outside it
        other = ER.loss64(pred, target, "l2" if lt != "l2" else "huber", 0.1)[0]
        assert not EB.inside(other, *r["loss"])[0]
    table = torch.zeros(2, K + 2)
    ER.eval_loss(pred, target, "l2", None, loss_out=table[1, 1:K + 1])
    assert torch.equal(table[1, 1:K + 1], ER.eval_loss(pred, target)[0]) and float(table[0].abs().sum() + table[1, 0].abs() + table[1, -1].abs()) == 0.0


def test_abi_exports_the_eval_loss_symbols():
    """include/st355.h declares, lib.py lists and types, and (when it is built) the library exports the three new entries"""
    from simpletuner_amd import lib
    names = ["st355_eval_loss_workspace", "st355_eval_flow_views", "st355_eval_loss"]
    header = open(os.path.join(ROOT, "include", "st355.h")).read()
    for n in names:
        assert n in lib.SYMBOLS and f"{n}(" in header, n
    assert "eval_loss.hip" in open(os.path.join(ROOT, "simpletuner_amd", "csrc", "Makefile")).read()
    if lib.is_built():
        L = lib.load()
        assert all(hasattr(L, n) for n in names)


# ------------------------------------------------------------------------------------------------
# (c) the pass through the emulator on the tiny engines
# ------------------------------------------------------------------------------------------------
def _acc():
    return NS(device=torch.device("cpu"), num_processes=1, process_index=0, is_main_process=True, gradient_accumulation_steps=1, sync_gradients=True,
              backward=lambda loss: loss.backward(), wait_for_everyone=lambda: None)


def _raw(t, noise=True):
    b = {"latent_batch": t["latents"], "prompt_embeds": t["prompt"], "add_text_embeds": t["pooled"]}
    if noise:
        b["noise"] = t["noise"]
    return b


def _trainer(monkeypatch, family, eval_noise=True, fix_sigmas=True, **cfg_kw):
    """the two-block SD3 / the 1 + 1 Flux of the host-sequencing tests (B = 2, 16 x 8 latents) with two eval batches (seeds 4 and 6)"""
    from simpletuner_amd.training.trainer import Trainer, default_config
    ER.install(monkeypatch)
    cfg = default_config(model_family=family, train_batch_size=2, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, **cfg_kw)
    if family == "flux":
        from simpletuner_amd.flux import transformer as T
        from simpletuner_amd.flux.model import Flux
        monkeypatch.setattr(T, "_FUSED_QKV", False); monkeypatch.setattr(T, "_BLOCK_ABI", False)
        plugin = Flux(cfg, _acc())
        plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    else:
        from simpletuner_amd.sd3.model import SD3
        plugin = SD3(cfg, _acc())
        plugin.load_model(**SH._arch(2))
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    cpu, devt = PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=3)
    evals = [PU.make_inputs(2, 16, 8, 24, 128, 64, "cpu", seed=s) for s in (4, 6)]
    sets = {"val": [_raw(e[1], eval_noise) for e in evals]}
    trainer = Trainer(cfg, plugin, plugin.accelerator, eval_sets=sets)
    if fix_sigmas:
        plugin.sample_flow_sigmas = lambda batch, state: (devt["sigmas"], devt["sigmas"] * 1000.0)
    return plugin, trainer, _raw(devt), [e[0] for e in evals]


def oracle_table(family, comp, eval_cpu, grid, loss_type="l2", huber_c=0.1):
    """[batches, T] fp64: the oracle forward in fp64 at the chain's (sigma, timestep) on the bf16 noisy rows, oracle/train_math's loss against bf16(noise - latents)"""
    P, lora, scale = PU.oracle_state(comp, dtype=F64)
    if family == "sd3":
        P["pos_embed.pos_embed"] = comp.pos_embed.pos_embed.detach().to(F64).cpu()
        ocfg = SH._ocfg(comp)
        fwd = lambda x, c, t: OS.sd3_forward(P, ocfg, x, c["prompt"].to(F64), c["pooled"].to(F64), t, lora=lora, lora_scale=scale)
    else:
        ocfg = PU.oracle_cfg(comp)
        fwd = lambda x, c, t: OF.flux_model_predict(P, ocfg, x, c["prompt"].to(F64), c["pooled"].to(F64), t, 1.0, lora=lora, lora_scale=scale)
    sig, ts = ER.dtype_chain(grid)
    rows = []
    with torch.no_grad():
        for c in eval_cpu:
            x, n = c["latents"].to(F64), c["noise"].to(F64)
            B = x.shape[0]
            target = (n - x).to(BF16).to(F64)
            row = []
            for s, t in zip(sig.to(F64), ts.to(F64)):
                noisy, _ = TM.flow_noisy_and_target(x, n, s.expand(B))
                pred = fwd(noisy.to(BF16).to(F64), c, t.expand(B))
                row.append(float(TM.conditional_loss(pred, target, loss_type, huber_c)[0]))
            rows.append(row)
    return torch.tensor(rows, dtype=F64)


def _table(trainer, name="val"):
    by_t = trainer.last_eval_table[name]
    return torch.tensor([by_t[t] for t in by_t], dtype=F64).T          # [batches, T] in grid order


_ORACLE = {}


def _oracle_for(family, trainer, eval_cpu):
    """computed once per family (the weights before any step are the same in every test below) and left unchanged"""
    if family not in _ORACLE:
        grid = trainer.evaluation.get_timestep_schedule(trainer.evaluation.noise_scheduler_of(trainer.model), model=trainer.model)
        _ORACLE[family] = oracle_table(family, trainer.model.get_trained_component(), eval_cpu, grid)
    return _ORACLE[family]


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_val_loss_is_logged_exactly_where_would_evaluate_is_true(monkeypatch, family):
    """FAILS ON THE PARENT COMMIT (the flags are read nowhere there: the constructor takes no eval sets and nothing is logged)"""
    plugin, trainer, batch, _ = _trainer(monkeypatch, family, eval_steps_interval=2, eval_timesteps=4)
    logged = {}
    step = trainer.train_step

    def stepped(b):
        out = step(b)
        logged[trainer.state["global_step"]] = None
        return out
    trainer.train_step = stepped
    trainer.train([batch] * 5, 5)
    for s, logs in trainer.eval_history:
        logged[s] = logs
    want = [s for s in range(1, 6) if trainer.evaluation.would_evaluate({"global_step": s})]
    assert want == [2, 4] and [s for s, v in logged.items() if v] == want
    for s in want:
        assert set(logged[s]) == {"loss/val/val"} and isinstance(logged[s]["loss/val/val"], float) and logged[s]["loss/val/val"] > 0
    assert trainer.last_eval_logs is None          # step 5 ran no eval
    vals = [v for by_t in [trainer.last_eval_table["val"]] for t in by_t for v in by_t[t]]
    assert len(vals) == 8 and abs(logged[4]["loss/val/val"] - sum(vals) / 8) < 1e-6


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_table_equals_the_fp64_oracle_and_stacking_does_not_change_it(monkeypatch, family):
    """the loss tolerance of the host-sequencing parity tests (|d| < 2e-3 max(1, loss)), for every stack size; T = 4 with k = 3 leaves a shorter last chunk"""
    tables = {}
    for k in (1, 2, 3, 4):
        plugin, trainer, batch, eval_cpu = _trainer(monkeypatch, family, eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=k)
        want = _oracle_for(family, trainer, eval_cpu)
        calls = []
        predict = plugin.model_predict
        plugin.model_predict = lambda pb: calls.append((pb["noisy_latents"].shape[0], torch.is_grad_enabled())) or predict(pb)
        logs = trainer.evaluate()
        assert calls == [(2 * n, False) for _ in range(2) for n in ([k] * (4 // k) + ([4 % k] if 4 % k else []))], (k, calls)
        got = tables[k] = _table(trainer)
        assert got.shape == want.shape == (2, 4)
        worst = float(((got - want).abs() / want.clamp_min(1.0)).max())
        print(f"[emu] {family} stack {k}: table {got.flatten().tolist()} vs oracle {want.flatten().tolist()}, worst |d| / max(1, loss) {worst:.3e}")
        assert worst < 2e-3, (k, worst)
        assert abs(logs["loss/val/val"] - float(want.mean())) < 2e-3 * max(1.0, float(want.mean()))
        monkeypatch.undo()
    for k in (2, 3, 4):
        assert float(((tables[k] - tables[1]).abs() / tables[1].clamp_min(1.0)).max()) < 2e-3, k


@pytest.mark.parametrize("loss_type,schedule", [("huber", "constant"), ("smooth_l1", "snr")])
def test_huber_losses_follow_the_stacked_timesteps(monkeypatch, loss_type, schedule):
    """one huber_c per stacked row, from the row's own (model) timestep"""
    plugin, trainer, batch, eval_cpu = _trainer(monkeypatch, "sd3", eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=4, loss_type=loss_type,
                                                huber_schedule=schedule, huber_c=0.1)
    grid = trainer.evaluation.get_timestep_schedule(trainer.evaluation.noise_scheduler_of(plugin), model=plugin)
    _, ts = ER.dtype_chain(grid)
    comp = plugin.get_trained_component()
    want = torch.stack([oracle_table("sd3", comp, eval_cpu, grid[j:j + 1], loss_type,
                                     TM.scheduled_huber_c(ts[j:j + 1].expand(2), schedule, 0.1, True))[:, 0] for j in range(4)], dim=1)
    trainer.evaluate()
    got = _table(trainer)
    assert float(((got - want).abs() / want.clamp_min(1.0)).max()) < 2e-3, (got, want)


@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_eval_at_every_step_leaves_training_bit_equal(monkeypatch, family):
    """4 steps with an eval after every step against the run without: losses and adapter arena bit for bit.  The training side draws its sigmas from torch's
    generator, its noise from the counter stream and walks a round-robin list: all three must be where training left them."""
    runs = {}
    for name, kw in (("plain", {}), ("eval", dict(eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=2))):
        plugin, trainer, batch, _ = _trainer(monkeypatch, family, eval_noise=False, fix_sigmas=False, flow_custom_timesteps="100,350,600,850,975",
                                             flow_timesteps_mode="round-robin", **kw)
        batch.pop("noise")
        torch.manual_seed(77)
        losses = [l.clone() for l in trainer.train([dict(batch) for _ in range(4)], 4)]
        runs[name] = (losses, plugin.get_trained_component().lora_flat.clone(), plugin._noise_step, plugin._noise_offset, plugin._flow_custom_timestep_cursor,
                      torch.get_rng_state().clone(), len(trainer.eval_history))
        if name == "eval":
            before = (plugin._noise_step, plugin._noise_offset, plugin._flow_custom_timestep_cursor, torch.get_rng_state().clone())
            a = trainer.evaluate()
            after = (plugin._noise_step, plugin._noise_offset, plugin._flow_custom_timestep_cursor, torch.get_rng_state().clone())
            assert before[:3] == after[:3] and torch.equal(before[3], after[3]) and not hasattr(plugin, "_eval_noise_seed")
            t1 = _table(trainer)
            assert a == trainer.evaluate() and torch.equal(t1, _table(trainer))          # the eval noise stream is fixed: every eval sees the same noise
        monkeypatch.undo()
    p, e = runs["plain"], runs["eval"]
    assert p[6] == 0 and e[6] == 4
    assert all(torch.equal(a, b) for a, b in zip(p[0], e[0])) and torch.equal(p[1], e[1])
    assert p[2:5] == e[2:5] and torch.equal(p[5], e[5])
    assert len({float(l) for l in p[0]}) == 4          # (the steps do differ from one another: the comparison is not vacuous)


def test_the_default_stack_is_the_measured_one_per_family():
    """profiles/eval_loss_kernel_stats.md: the smallest k measured faster than k = 1 by more than the run-to-run spread — 2 for both built families; an unknown
    family keeps 1; a set value wins"""
    from simpletuner_amd.training.evaluation import timestep_stack
    assert timestep_stack(NS(model_family="sd3")) == 2 and timestep_stack(NS(model_family="flux")) == 2 and timestep_stack(NS(model_family="other")) == 1
    assert timestep_stack(NS(model_family="sd3", eval_timestep_stack=1)) == 1 and timestep_stack(NS(model_family="flux", eval_timestep_stack=7)) == 7


def test_layersync_passes_through_and_the_schedule_object_is_not_moved(monkeypatch):
    """LayerSync does not enter loss(): the eval table is the plain run's, and the training schedule's own timesteps are untouched by set_timesteps"""
    plugin0, trainer0, _, _ = _trainer(monkeypatch, "sd3", eval_steps_interval=1, eval_timesteps=4)
    trainer0.evaluate()
    t0 = _table(trainer0)
    monkeypatch.undo()
    plugin, trainer, _, _ = _trainer(monkeypatch, "sd3", eval_steps_interval=1, eval_timesteps=4, layersync_enabled=True, layersync_student_block=0, layersync_teacher_block=1,
                                     layersync_lambda=0.1)
    plugin.setup_training_noise_schedule()
    before = plugin.noise_schedule.timesteps.clone()
    trainer.evaluate()
    assert torch.equal(_table(trainer), t0)
    assert torch.equal(plugin.noise_schedule.timesteps, before) and plugin.noise_schedule.num_inference_steps is None


# ---- world size 2 over gloo ----
def _run_rank(rank, world, with_eval):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    patch = pytest.MonkeyPatch()
    ER.install(patch)
    kw = dict(eval_steps_interval=1, eval_timesteps=4, eval_timestep_stack=2) if with_eval else {}
    cfg = default_config(model_family="sd3", train_batch_size=1, seed=3, lora_rank=8, lora_init_b_std=0.02, learning_rate=1e-3, **kw)
    acc = St355Accelerator(torch.device("cpu"))
    plugin = SD3(cfg, acc)
    plugin.load_model(**SH._arch(2))
    plugin.get_trained_component().init_synthetic(3)
    plugin.add_lora_adapter()
    plugin.post_model_load_setup()
    _, devt = PU.make_inputs(2, 8, 8, 24, 128, 64, "cpu", seed=3)
    _, ev = PU.make_inputs(1, 8, 8, 24, 128, 64, "cpu", seed=4)
    trainer = Trainer(cfg, plugin, acc, eval_sets={"val": [_raw(ev)]} if with_eval else None)
    mine = {k: v[rank:rank + 1] for k, v in devt.items()}
    plugin.sample_flow_sigmas = lambda batch, state: (mine["sigmas"], mine["sigmas"] * 1000.0)
    collectives = []
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "barrier", "reduce_scatter_tensor"):
        real = getattr(dist, name)
        patch.setattr(dist, name, lambda *a, _n=name, _r=real, **k: collectives.append(_n) or _r(*a, **k))
    marks = []
    evaluate = trainer.evaluate
    trainer.evaluate = lambda: (marks.append(len(collectives)), evaluate(), marks.append(len(collectives)))[1]
    losses = [float(l) for l in trainer.train([_raw(mine) for _ in range(3)], 3)]
    flat = plugin.get_trained_component().lora_flat.clone()
    history = list(trainer.eval_history)
    direct = trainer.evaluate()
    patch.undo()
    return dict(losses=losses, flat=flat, history=history, direct=direct, marks=marks, has_eval=trainer.evaluation is not None)


def _worker(rank, world, init_file, out_dir):
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    out = {"plain": _run_rank(rank, world, False), "eval": _run_rank(rank, world, True)}
    torch.save(out, os.path.join(out_dir, f"eval_{rank}.pt"))
    dist.destroy_process_group()


def test_world_size_two_rank_one_logs_nothing_and_both_trajectories_are_unchanged():
    with tempfile.TemporaryDirectory() as d:
        init = os.path.join(d, "init")
        mp.spawn(_worker, args=(2, init, d), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"eval_{i}.pt"), weights_only=False) for i in range(2)]
    for i in range(2):
        assert r[i]["plain"]["losses"] == r[i]["eval"]["losses"] and torch.equal(r[i]["plain"]["flat"], r[i]["eval"]["flat"]), i
        assert r[i]["eval"]["has_eval"] and not r[i]["plain"]["has_eval"]
    assert torch.equal(r[0]["eval"]["flat"], r[1]["eval"]["flat"])
    assert [s for s, _ in r[0]["eval"]["history"]] == [1, 2, 3] and all(set(l) == {"loss/val/val"} for _, l in r[0]["eval"]["history"])
    assert r[1]["eval"]["history"] == [] and r[1]["eval"]["direct"] == {} and set(r[0]["eval"]["direct"]) == {"loss/val/val"}
    for i in range(2):          # no collective inside any evaluate(): the count before equals the count after
        m = r[i]["eval"]["marks"]
        assert m and all(m[j] == m[j + 1] for j in range(0, len(m), 2)), (i, m)


# ------------------------------------------------------------------------------------------------
# (d) refusals, by their full text
# ------------------------------------------------------------------------------------------------
OFF = " or eval_loss_disable=true"
WHY = "the reference's eval forwards are training-mode forwards that {}, which the no-grad route of the st355 path does not; not built; "
REFUSALS = [
    (dict(lora_dropout=0.1), "eval_steps_interval=5 with lora_dropout=0.1: " + WHY.format("drop") + "set lora_dropout=0" + OFF),
    (dict(tread_config={"routes": [{"selection_ratio": 0.5}]}), "eval_steps_interval=5 with TREAD routing: " + WHY.format("route tokens") + "unset tread_config or set eval_loss_disable=true"),
    (dict(crepa_enabled=True), "eval_steps_interval=5 with crepa_enabled: the evaluation loss next to Self-Flow's views is not built on the st355 path; set crepa_enabled=false" + OFF),
    (dict(twinflow_enabled=True), "eval_steps_interval=5 with twinflow_enabled: the evaluation loss next to TwinFlow's signed times is not built on the st355 path; "
     "set twinflow_enabled=false" + OFF),
    (dict(distillation_method="flow_dpo"), "eval_steps_interval=5 with distillation_method=flow_dpo: the evaluation loss of a distillation run is not built on the st355 path; "
     "unset distillation_method or set eval_loss_disable=true"),
    (dict(scheduled_sampling_max_step_offset=2), "eval_steps_interval=5 with scheduled_sampling_max_step_offset=2: the reference's eval batches carry a rollout plan, which the "
     "stacked pass does not run; set scheduled_sampling_max_step_offset=0" + OFF),
    (dict(scheduled_sampling_reflexflow=True), "eval_steps_interval=5 with scheduled_sampling_reflexflow: the reference's eval loss then carries the ReflexFlow terms, which the "
     "eval loss kernel does not compute; set scheduled_sampling_reflexflow=false" + OFF),
]


@pytest.mark.parametrize("family", ["sd3", "flux"])
@pytest.mark.parametrize("kw,message", REFUSALS)
def test_sd3_and_flux_refuse_what_is_not_built_by_exact_message(family, kw, message):
    from simpletuner_amd.training.evaluation import refuse_unbuilt
    flow = NS(PREDICTION_TYPE=NS(value="flow_matching"), xm_config=None)
    with pytest.raises(NotImplementedError) as ei:
        refuse_unbuilt(NS(model_family=family, model_type="lora", eval_steps_interval=5, **kw), flow, {"val": [{}]})
    assert str(ei.value) == message
    refuse_unbuilt(NS(model_family=family, model_type="lora", eval_steps_interval=5), flow, {"val": [{}]})


def test_other_refusals_by_exact_message():
    from simpletuner_amd.training.evaluation import refuse_unbuilt
    flow = NS(PREDICTION_TYPE=NS(value="flow_matching"), xm_config=None)
    for family, pt in (("sdxl", "epsilon"), ("pixart_sigma", "epsilon"), ("sd1x", "v_prediction")):
        with pytest.raises(NotImplementedError) as ei:
            refuse_unbuilt(NS(model_family=family, eval_epoch_interval=0.5), NS(PREDICTION_TYPE=NS(value=pt)), {"val": [{}]})
        assert str(ei.value) == (f"eval_epoch_interval=0.5: the evaluation loss is not built for model_family={family} on the st355 path (built: flux, sd3) — the DDPM grid needs "
                                 "diffusers' DDPMScheduler.set_timesteps; unset eval_steps_interval and eval_epoch_interval, or set eval_loss_disable=true")
    for sets in (None, {}):
        with pytest.raises(ValueError) as ei:
            refuse_unbuilt(NS(model_family="sd3", eval_steps_interval=100), flow, sets)
        assert str(ei.value) == ("eval_steps_interval=100: no eval set was given — pass eval_sets={name: batches} to the Trainer (the reference's _type='eval' backends), "
                                 "or set eval_loss_disable=true")
    with pytest.raises(NotImplementedError) as ei:
        refuse_unbuilt(NS(model_family="flux", eval_steps_interval=5), NS(PREDICTION_TYPE=NS(value="flow_matching"), xm_config=NS(enabled=True)), {"val": [{}]})
    assert str(ei.value) == ("eval_steps_interval=5 with XM noise candidates: the eval forwards would expand every row into candidates; not built on the st355 path — "
                             "disable the XM noise candidates or set eval_loss_disable=true")
    for bad in (0, -1, 2.0, "4", True):
        with pytest.raises(ValueError) as ei:
            refuse_unbuilt(NS(model_family="sd3", eval_steps_interval=5, eval_timestep_stack=bad), flow, {"val": [{}]})
        assert str(ei.value) == f"eval_timestep_stack must be an integer >= 1, got {bad!r}"
    with pytest.raises(ValueError) as ei:
        refuse_unbuilt(NS(model_family="sd3", eval_steps_interval=5, eval_timestep_stack=65), flow, {"val": [{}]})
    assert str(ei.value) == "eval_timestep_stack=65: at most 64 timesteps are stacked into one forward; set eval_timestep_stack<=64"
    with pytest.raises(ValueError) as ei:
        refuse_unbuilt(NS(model_family="sd3", eval_steps_interval=5, eval_timesteps=0), flow, {"val": [{}]})
    assert str(ei.value) == "eval_timesteps must be an integer >= 1, got 0"


def test_the_trainer_refuses_at_construction_and_eval_loss_disable_switches_everything_off(monkeypatch):
    from simpletuner_amd.sd3.model import SD3
    from simpletuner_amd.training.trainer import Trainer, default_config
    ER.install(monkeypatch)
    cfg = default_config(model_family="sd3", lora_rank=8, eval_steps_interval=3)
    plugin = SD3(cfg, _acc())
    plugin.load_model(**SH._arch(2))
    plugin.add_lora_adapter()
    with pytest.raises(ValueError, match=r"^eval_steps_interval=3: no eval set was given"):
        Trainer(cfg, plugin, plugin.accelerator)
    cfg.lora_dropout = 0.1
    with pytest.raises(NotImplementedError, match=r"^eval_steps_interval=3 with lora_dropout=0.1: "):
        Trainer(cfg, plugin, plugin.accelerator, eval_sets={"val": [{}]})
    cfg.hip_graph = True          # eval runs eager between replays: not refused
    cfg.lora_dropout = 0.0
    assert Trainer(cfg, plugin, plugin.accelerator, eval_sets={"val": [{}]}).evaluation is not None
    cfg.eval_loss_disable = True
    trainer = Trainer(cfg, plugin, plugin.accelerator)
    assert trainer.evaluation is None and trainer.evaluate() == {}


# ------------------------------------------------------------------------------------------------
# (e) flag absent
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sd3", "flux"])
def test_flag_absent_imports_nothing_and_launches_nothing(monkeypatch, family):
    from simpletuner_amd import ops
    results = []
    for kw in ({}, dict(eval_steps_interval=None, eval_epoch_interval=""), dict(eval_steps_interval=0), dict(eval_steps_interval=2, eval_loss_disable=True)):
        sys.modules.pop("simpletuner_amd.training.evaluation", None)
        plugin, trainer, batch, _ = _trainer(monkeypatch, family, **kw)
        for name in ER.STAND_INS:
            monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("an evaluation op ran with the flag absent"))
        losses = trainer.train([batch] * 2, 2)
        assert "simpletuner_amd.training.evaluation" not in sys.modules
        assert trainer.evaluation is None and trainer.last_eval_logs is None and trainer.eval_history == [] and trainer.evaluate() == {}
        results.append((losses[-1].clone(), plugin.get_trained_component().lora_flat.clone()))
        monkeypatch.undo()
    assert all(torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) for r in results[1:])

"""SOAP without a GPU: the fp64 restatement (tests/soap_ref.py) against the reference's own SOAP (tests/golden/soap_vectors.pt, written by
tools/gen_soap_golden.py), the recorded evidence for preconditioning the rank side only, the registry / settings / trainer
surface, every refusal, the state layout and the loading of the reference's state_dict — St355Soap's kernel calls replaced by the CPU stand-in
of tests/soap_ref.py."""
import copy
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from tests import soap_ref as SR

ROOT = Path(__file__).resolve().parent.parent
GOLD = torch.load(ROOT / "tests" / "golden" / "soap_vectors.pt")
F32 = torch.float32
WELL_POSED = ("one_sided_f3", "one_sided_f10", "zero_first_grad", "wd0", "nobias", "sb09")


def _arena(shapes, values=None):
    n = sum(a * b for a, b in shapes)
    flat, gflat = torch.zeros(n), torch.zeros(n)
    ps, off = [], 0
    for i, s in enumerate(shapes):
        k = s[0] * s[1]
        if values is not None:
            flat[off:off + k] = values[i].reshape(-1)
        p = torch.nn.Parameter(flat[off:off + k].view(s))
        p.grad = gflat[off:off + k].view(s)
        ps.append(p)
        off += k
    return flat, gflat, ps


@pytest.mark.parametrize("name", WELL_POSED)
def test_restatement_reproduces_the_recorded_reference_trajectory(name):
    """tolerance: the reference's own fp32-vs-fp64-decomposition distance on that run, times 4 (two fp32 evaluations each sit about that far from
    exact; a factor 2 for another summation order) — recorded, not chosen.  The distances are one or two fp32 ulps of a parameter, so the restatement
    stores what the class stores in fp32 (every operation exact in fp64, then rounded once): without that it could not come within an ulp at all"""
    run = GOLD[name]
    tol = 4.0 * max(max(d) for d in run["dist_f64dec"])
    traj = SR.run_fp64(run["p0"], run["grads"], run["settings"], store=F32)
    worst = 0.0
    for k, (mine, ref) in enumerate(zip(traj, run["traj"])):
        for a, b in zip(mine, ref):
            worst = max(worst, (a - b.double()).abs().max().item())
    print(f"[soap] {name}: fp64 restatement vs recorded reference, worst |d p| = {worst:.3e}, tolerance {tol:.3e}")
    assert torch.equal(run["traj"][0][0], run["p0"][0])                    # the first call leaves the parameters alone
    assert worst <= tol


def test_restatement_continues_from_the_recorded_state_dict():
    run = GOLD["one_sided_f3"]
    k0 = run["state_at"]
    sd = run["state_dict"]["state"]
    p_at = run["traj"][k0]
    tol = 4.0 * max(max(d) for d in run["dist_f64dec"])
    traj = SR.run_fp64(p_at, run["grads"], run["settings"], start_state=sd, first_call=k0 + 1, store=F32)
    for mine, ref in zip(traj, run["traj"][k0 + 1:]):
        for a, b in zip(mine, ref):
            assert (a - b.double()).abs().max().item() <= tol


@pytest.mark.parametrize("name", WELL_POSED)
def test_column_signs_of_the_decompositions_cancel_bit_for_bit(name):
    run = GOLD[name]
    for a, b in zip(run["traj"], run["traj_signs"]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_two_sided_default_is_not_reproducible_which_is_why_it_is_refused():
    """with the long side preconditioned too (the registry default max_precond_dim=10000) the reference run with its decompositions in fp64 leaves
    the fp32 run by more than a tenth of what one step moves a parameter"""
    run = GOLD["two_sided"]
    assert run["settings"].get("max_precond_dim", 10000) == 10000
    worst = max(max(d) for d in run["dist_f64dec"])
    assert worst > 0.1 * run["one_step"], (worst, run["one_step"])
    for name in WELL_POSED:                                               # and the one-sided runs sit four orders of magnitude closer
        assert max(max(d) for d in GOLD[name]["dist_f64dec"]) < 1e-4 * GOLD[name]["one_step"]


def test_registry_entry_settings_and_parsing():
    from simpletuner_amd.training.optimizer import OPTIMIZER_CHOICE, St355Soap, optimizer_settings
    entry = OPTIMIZER_CHOICE["soap"]
    assert entry["class"] is St355Soap and entry["precision"] == "any"
    assert entry["default_settings"] == GOLD["default_settings"]
    assert optimizer_settings("soap", SimpleNamespace()) == GOLD["default_settings"]
    merged = optimizer_settings("soap", SimpleNamespace(optimizer_config="max_precond_dim=128,precondition_frequency=5,correct_bias=false"))
    assert merged["max_precond_dim"] == 128 and merged["precondition_frequency"] == 5 and merged["correct_bias"] is False
    import inspect
    sig = inspect.signature(St355Soap.__init__)
    want = dict(lr=3e-3, betas=(0.95, 0.95), shampoo_beta=-1, eps=1e-8, weight_decay=0.01, precondition_frequency=10, max_precond_dim=10000,
                merge_dims=False, precondition_1d=False, normalize_grads=False, data_format="channels_first", correct_bias=True)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")} == want


def test_every_refusal_fires_by_name():
    from simpletuner_amd.training.optimizer import St355Soap
    _, _, ps = _arena([(32, 3072), (3072, 32)])
    with pytest.raises(NotImplementedError) as e:
        St355Soap(ps)                                                    # the registry default max_precond_dim=10000
    msg = str(e.value)
    assert "max_precond_dim=10000" in msg and "(32, 3072)" in msg and "32 <= max_precond_dim <= 3071" in msg
    assert "--optimizer_config=max_precond_dim=128" in msg
    with pytest.raises(NotImplementedError, match=r"16 <= max_precond_dim <= 199"):
        St355Soap(_arena([(16, 200)])[2], max_precond_dim=8)             # the short side would be left out as well
    St355Soap(ps, max_precond_dim=128, precondition_1d=True, data_format="channels_last")     # no effect on 2-D parameters: accepted
    with pytest.raises(NotImplementedError, match="merge_dims"):
        St355Soap(ps, max_precond_dim=128, merge_dims=True)
    with pytest.raises(NotImplementedError, match="normalize_grads"):
        St355Soap(ps, max_precond_dim=128, normalize_grads=True)
    with pytest.raises(NotImplementedError, match="1 dimensions"):
        St355Soap([torch.nn.Parameter(torch.zeros(16))], max_precond_dim=128)
    with pytest.raises(NotImplementedError, match="short side above 128"):
        St355Soap([torch.nn.Parameter(torch.zeros(129, 200))], max_precond_dim=150)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        St355Soap([torch.nn.Parameter(torch.zeros(8, 64, dtype=torch.bfloat16))], max_precond_dim=16)
    with pytest.raises(NotImplementedError, match="one contiguous fp32 run"):
        St355Soap([torch.nn.Parameter(torch.zeros(8, 64)), torch.nn.Parameter(torch.zeros(64, 8))], max_precond_dim=16)
    with pytest.raises(NotImplementedError, match="max_precond_dim"):
        St355Soap(_arena([(64, 64)])[2], max_precond_dim=64)             # a square matrix has no admissible value


class _Plugin:
    def __init__(self, comp):
        self.comp = comp
        self.accelerator = SimpleNamespace(num_processes=1)

    def get_trained_component(self):
        return self.comp


def test_trainer_wiring_and_refusals(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Soap
    from simpletuner_amd.training.trainer import Trainer, default_config
    SR.install(monkeypatch)
    _, _, ps = _arena([(8, 64), (64, 8)])
    comp = SimpleNamespace(trainable_parameters=lambda: ps, full=False)
    acc = SimpleNamespace(num_processes=1)
    tr = Trainer(default_config(optimizer="soap", optimizer_config="max_precond_dim=32", learning_rate=2e-3), _Plugin(comp), acc)
    assert isinstance(tr.optimizer, St355Soap) and tr.optimizer.fuses_ema is False
    assert tr.optimizer.param_groups[0]["lr"] == 2e-3 and tr.optimizer.param_groups[0]["max_precond_dim"] == 32
    with pytest.raises(NotImplementedError, match="max_precond_dim=10000"):
        Trainer(default_config(optimizer="soap"), _Plugin(comp), acc)
    with pytest.raises(NotImplementedError, match="LoRA adapters only"):
        Trainer(default_config(optimizer="soap", optimizer_config="max_precond_dim=32"),
                _Plugin(SimpleNamespace(trainable_parameters=lambda: ps, full=True)), acc)
    with pytest.raises(NotImplementedError, match="hip_graph"):
        Trainer(default_config(optimizer="soap", optimizer_config="max_precond_dim=32", hip_graph=True), _Plugin(comp), acc)
    with pytest.raises(NotImplementedError) as e:
        Trainer(default_config(optimizer="adamw_schedulefree"), _Plugin(comp), acc)
    assert "soap" in str(e.value)                                       # the refusal lists the built optimizers


def test_state_layout_is_the_references_and_views_flat_buffers(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Soap
    SR.install(monkeypatch)
    shapes = [(8, 40), (40, 8), (4, 33)]
    flat, gflat, ps = _arena(shapes)
    opt = St355Soap(ps, lr=1e-3, max_precond_dim=16, shampoo_beta=0.9)
    gflat.normal_(generator=torch.Generator().manual_seed(0))
    opt.step()
    st = opt._flat[0]
    assert st["gg"].numel() == st["q"].numel() == 64 + 64 + 16 and st["gg"].dtype == st["q"].dtype == F32
    assert opt.abi_calls == 1 and opt.fuses_ema is False
    for p, off, r in zip(ps, (0, 64, 128), (8, 8, 4)):
        s = opt.state[p]
        side = 0 if p.shape[0] < p.shape[1] else 1
        assert isinstance(s["step"], int) and s["step"] == 0
        assert s["precondition_frequency"] == 10 and s["shampoo_beta"] == 0.9
        for key, buf in (("GG", st["gg"]), ("Q", st["q"])):
            assert isinstance(s[key], list) and len(s[key]) == 2 and s[key][1 - side] == []
            t = s[key][side]
            assert t.shape == (r, r) and t.dtype == F32 and t.data_ptr() == buf.data_ptr() + 4 * off
        for key, buf in (("exp_avg", st["m"]), ("exp_avg_sq", st["v"])):
            assert s[key].shape == p.shape and s[key].dtype == F32
            assert s[key].data_ptr() == buf.data_ptr() + (p.data_ptr() - ps[0].data_ptr())
        assert torch.equal(s["exp_avg"], torch.zeros_like(p))            # the first call moves nothing
        q = s["Q"][side]
        assert (q.T @ q - torch.eye(r)).abs().max() < 1e-5
    assert torch.equal(flat, torch.zeros_like(flat))
    opt.step()
    assert all(opt.state[p]["step"] == 1 for p in ps) and opt.abi_calls == 2
    assert opt.state[ps[0]]["shampoo_beta"] == 0.9
    opt2 = St355Soap(_arena(shapes)[2], max_precond_dim=16)
    opt2.step()                                                          # no gradients set to None here, but an all-None group is skipped
    assert opt2.state[opt2.param_groups[0]["params"][0]]["shampoo_beta"] == 0.95      # shampoo_beta=-1: betas[1] (:144)


def test_reference_state_dict_loads_into_the_declared_buffers_and_continues(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Soap
    SR.install(monkeypatch)
    run = GOLD["one_sided_f3"]
    k0 = run["state_at"]
    flat, gflat, ps = _arena(run["shapes"], values=run["traj"][k0])
    opt = St355Soap(ps, **run["settings"])
    sd = copy.deepcopy(run["state_dict"])
    opt.load_state_dict(sd)
    st = opt._flat[0]
    assert st["step"] == k0 and st["ready"] is True                       # call 0 is the skipped one: k0 calls later the step count is k0
    for i, p in enumerate(ps):
        old, s = sd["state"][i], opt.state[p]
        side = 0 if p.shape[0] < p.shape[1] else 1
        assert s["step"] == old["step"] == k0
        assert torch.equal(s["exp_avg"], old["exp_avg"]) and torch.equal(s["exp_avg_sq"], old["exp_avg_sq"])
        assert torch.equal(s["GG"][side], old["GG"][side]) and torch.equal(s["Q"][side], old["Q"][side]) and s["GG"][1 - side] == []
        assert s["exp_avg"].data_ptr() == st["m"].data_ptr() + (p.data_ptr() - ps[0].data_ptr())
        assert s["Q"][side].data_ptr() - st["q"].data_ptr() == 4 * st["plan"].q_offsets[i]
    tol = 4.0 * max(max(d) for d in run["dist_f64dec"]) + 8 * 2.0 ** -24 * float(flat.abs().max())     # the fp32 stand-in rounds every product
    for k in range(k0 + 1, len(run["grads"])):
        gflat.copy_(torch.cat([g.reshape(-1) for g in run["grads"][k]]))
        opt.step()
        for p, ref in zip(ps, run["traj"][k]):
            assert (p.detach() - ref).abs().max().item() <= tol
    two = GOLD["two_sided"]
    fresh = St355Soap(_arena([(8, 40)])[2], lr=1e-3, max_precond_dim=16)
    with pytest.raises(NotImplementedError, match="another side"):
        fresh.load_state_dict(copy.deepcopy(two["final_state_dict"]))


def test_a_checkpoint_written_before_the_first_step_reloads_as_not_yet_initialised(monkeypatch):
    """load_state_dict builds the buffers (an all-zero Q among them); a state_dict() taken then, before any step, must not count as an existing basis"""
    from simpletuner_amd.training.optimizer import St355Soap
    SR.install(monkeypatch)
    shapes = [(8, 40), (40, 8)]
    _, _, ps = _arena(shapes)
    opt = St355Soap(ps, lr=1e-3, max_precond_dim=16)
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))                   # an empty state: builds the group
    early = copy.deepcopy(opt.state_dict())
    assert early["state"] and not early["state"][0]["Q"][0].any()
    flat, gflat, ps2 = _arena(shapes, values=[torch.full(s, 0.1) for s in shapes])
    opt2 = St355Soap(ps2, lr=1e-3, max_precond_dim=16, weight_decay=0.0)
    opt2.load_state_dict(early)
    assert opt2._flat[0]["ready"] is False and opt2._flat[0]["step"] == 0
    gflat.normal_(generator=torch.Generator().manual_seed(1))
    before = flat.clone()
    opt2.step()                                                           # the first call: builds the basis, moves nothing
    assert torch.equal(flat, before) and opt2._flat[0]["ready"] and opt2._flat[0]["q"].any()
    opt2.step()
    assert not torch.equal(flat, before) and opt2.state[ps2[0]]["step"] == 1


def test_own_state_dict_round_trips_bit_for_bit(monkeypatch):
    from simpletuner_amd.training.optimizer import St355Soap
    SR.install(monkeypatch)
    run = GOLD["one_sided_f3"]

    def drive(opt, gflat, calls):
        for k in calls:
            gflat.copy_(torch.cat([g.reshape(-1) for g in run["grads"][k]]))
            opt.step()

    flat, gflat, ps = _arena(run["shapes"], values=run["p0"])
    opt = St355Soap(ps, **run["settings"])
    drive(opt, gflat, range(4))
    saved, p_mid = copy.deepcopy(opt.state_dict()), flat.clone()
    drive(opt, gflat, range(4, 8))
    flat2, gflat2, ps2 = _arena(run["shapes"], values=[p_mid[:320].view(8, 40), p_mid[320:].view(40, 8)])
    opt2 = St355Soap(ps2, **run["settings"])
    opt2.load_state_dict(saved)
    drive(opt2, gflat2, range(4, 8))
    assert torch.equal(flat, flat2)
    assert torch.equal(opt._flat[0]["v"], opt2._flat[0]["v"]) and torch.equal(opt._flat[0]["q"], opt2._flat[0]["q"])


def test_abi_exports_the_three_soap_symbols():
    from simpletuner_amd import lib
    header = (ROOT / "include" / "st355.h").read_text()
    L = lib.load()
    for s in ("st355_soap_plan", "st355_soap_step", "st355_soap_eigh"):
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in lib.SYMBOLS and hasattr(L, s), s

#!/usr/bin/env python3
"""Generate tests/golden/flow_dpo_vectors.pt by EXECUTING the reference's FlowDPODistiller on the CPU, seeded.

Like tools/gen_scheduled_sampling_golden.py: the reference package cannot be imported as a package here, so
  * helpers/distillation/common.py (DistillationBase; pure torch) and helpers/distillation/flow_dpo/distiller.py are loaded as files over stand-in modules for what
    they import at module level — `simpletuner.helpers.models.common` (only the PredictionTypes enum is read), `...data_backend.dataset_types` (only names handed
    to the registry) and `...distillation.registry` (a register() that does nothing);
  * `DistillerFactory._method_config` is lifted from helpers/distillation/factory.py by AST (the flat / method-keyed resolution).
The teacher is a stub: a seeded deterministic `model_predict`, `PREDICTION_TYPE`, `get_flow_matching_target`, and a trained component whose `enable_lora` /
`disable_lora` switch a fixed perturbation (policy = reference + 0.1 * noise, pulled by 0.1 towards the preferred target: an asymmetric bias, so that every
margin is far above the fp32 summation bound — checked below, zero undecided samples allowed).  Nothing of the reference is copied into the repository; only the
recorded tensors are.  The reference tree is read ONLY by this script, never at test time.

    python tools/gen_flow_dpo_golden.py
"""
from __future__ import annotations

import ast
import enum
import importlib.util
import sys
import types
from pathlib import Path

import torch

REF = Path("/root/reference/simpletuner")
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "flow_dpo_vectors.pt"
NS = types.SimpleNamespace
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
B, C, H, W = 3, 4, 8, 8
U = 2.0 ** -24


class PredictionTypes(enum.Enum):
    EPSILON = "epsilon"; V_PREDICTION = "v_prediction"; FLOW_MATCHING = "flow_matching"; SAMPLE = "sample"


def load_file(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, str(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("simpletuner", "simpletuner.helpers", "simpletuner.helpers.models", "simpletuner.helpers.data_backend", "simpletuner.helpers.distillation",
                "simpletuner.helpers.distillation.flow_dpo"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    common = types.ModuleType("simpletuner.helpers.models.common")
    common.PredictionTypes = PredictionTypes
    sys.modules["simpletuner.helpers.models.common"] = common
    dt = types.ModuleType("simpletuner.helpers.data_backend.dataset_types")
    dt.DatasetType = NS(IMAGE="image", VIDEO="video", CONDITIONING="conditioning")
    sys.modules["simpletuner.helpers.data_backend.dataset_types"] = dt
    reg = types.ModuleType("simpletuner.helpers.distillation.registry")
    reg.DistillationRegistry = type("DistillationRegistry", (), {"register": classmethod(lambda cls, *a, **k: None)})
    sys.modules["simpletuner.helpers.distillation.registry"] = reg
    load_file("simpletuner.helpers.distillation.common", REF / "helpers/distillation/common.py")
    return load_file("simpletuner.helpers.distillation.flow_dpo.distiller", REF / "helpers/distillation/flow_dpo/distiller.py").FlowDPODistiller


def lift_method_config():
    tree = ast.parse((REF / "helpers/distillation/factory.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DistillerFactory")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_method_config")
    fn.decorator_list = []
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    mod = ast.Module(body=[fn], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"__builtins__": __builtins__}
    exec(compile(mod, "factory.py", "exec"), ns)
    return ns["_method_config"]


class Teacher:
    """the stub plugin: teacher and student at once"""
    PREDICTION_TYPE = PredictionTypes.FLOW_MATCHING

    def __init__(self, seed):
        self.config = NS(lora_type="standard")
        self.accelerator = NS(num_processes=1)
        self.adapter_on = True
        self.seed = seed
        self.calls = []
        outer = self
        self.component = NS(enable_lora=lambda: setattr(outer, "adapter_on", True), disable_lora=lambda: setattr(outer, "adapter_on", False))

    def get_trained_component(self):
        return self.component

    def get_flow_matching_target(self, prepared_batch, latents=None, prefer_explicit_target=False):
        return prepared_batch["noise"].float() - latents.float()

    def predict_values(self, batch, adapter_on):
        """bf16-representable fp32 values, a deterministic function of the batch and of the adapter switch"""
        rejected = batch.get("clean_latents") is not None
        t = batch["noise"].float() - batch["latents"].float()
        g = torch.Generator().manual_seed(self.seed * 7919 + (1 if rejected else 0))
        ref = 0.6 * batch["noisy_latents"].float() + 0.5 * torch.randn(t.shape, generator=g)
        ref = ref.to(BF16).float()
        if not adapter_on:
            return ref
        pol = ref + 0.1 * torch.randn(t.shape, generator=g)
        if not rejected:
            pol = pol + 0.1 * (t - ref)
        return pol.to(BF16).float()

    def model_predict(self, prepared_batch):
        pred = self.predict_values(prepared_batch, self.adapter_on)
        if self.adapter_on and torch.is_grad_enabled():
            pred.requires_grad_(True)
        self.calls.append((self.adapter_on, prepared_batch.get("clean_latents") is not None, pred))
        return {"model_prediction": pred}


def make_batch(seed, mask_kind):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    win, lose, noise = rn(B, C, H, W).to(BF16), rn(B, C, H, W).to(BF16), rn(B, C, H, W).to(BF16)
    sig = torch.rand(B, generator=g).mul(0.8).add(0.1).view(B, 1, 1, 1).to(BF16)
    batch = {"conditioning_type": "reference_strict", "latents": win, "conditioning_latents": lose, "noise": noise, "input_noise": noise, "sigmas": sig,
             "timesteps": sig.float().reshape(B) * 1000.0, "noisy_latents": ((1 - sig) * win + sig * noise)}
    if mask_kind is not None:
        batch["loss_mask_type"] = mask_kind
        cpv = 1.5 * rn(B, 3, 2 * H, 2 * W)          # outside [-1, 1] too: the clamp of the distiller's mask is exercised
        if mask_kind == "segmentation":
            cpv[:, :, :6, :] = -1.0                  # a region whose channel mean maps to exactly 0: outside the binarised mask
        batch["conditioning_pixel_values"] = cpv
    return batch


def margin_bound(rec, norm_type):
    """the fp32 summation bound of the reference's four-sum margin (its `.float()` calls make every executed value fp32): each error is a sum of n terms with at
    most 4 roundings per term — gamma(n + 4) E — scaled by nu, and the three differences add one rounding each"""
    f = lambda t: t.to(F64).reshape(B, -1)
    m = f(rec["mask"]).repeat(1, C) if rec["mask"] is not None else torch.ones(B, C * H * W, dtype=F64)
    n = C * H * W
    nu = 1.0 if norm_type == "sum" else (1.0 / m.sum(1).clamp_min(1.0) if (norm_type == "masked_mean" and rec["mask"] is not None) else 1.0 / n)
    E = lambda p, t: (m * (f(p) - f(t)) ** 2).sum(1) * nu
    es = [E(rec["policy_win"], rec["target_win"]), E(rec["ref_win"], rec["target_win"]), E(rec["policy_lose"], rec["target_lose"]), E(rec["ref_lose"], rec["target_lose"])]
    gam = (n + 4) * U / (1 - (n + 4) * U)
    return (gam + 3 * U) * sum(es), (es[1] - es[0]) + (es[2] - es[3])


CASES = []
for norm in ("sum", "mean", "masked_mean"):
    for mask_kind, dil in ((None, 0), ("mask", 0), ("segmentation", 0), ("segmentation", 1)):
        CASES.append(dict(norm_type=norm, mask=mask_kind, mask_dilate=dil, anchor_alpha=0.0, sft_loss_weight=0.0, auto_beta=False, beta=0.05 if norm == "sum" else 2.0))
CASES += [dict(norm_type="sum", mask=None, mask_dilate=0, anchor_alpha=0.5, sft_loss_weight=0.0, auto_beta=False, beta=0.05),
          dict(norm_type="mean", mask="mask", mask_dilate=0, anchor_alpha=0.0, sft_loss_weight=0.3, auto_beta=False, beta=2.0),
          dict(norm_type="mean", mask="mask", mask_dilate=1, anchor_alpha=0.25, sft_loss_weight=0.3, auto_beta=False, beta=2.0, loss_weight=0.7),
          dict(norm_type="sum", mask=None, mask_dilate=0, anchor_alpha=0.0, sft_loss_weight=0.0, auto_beta=True),
          dict(norm_type="mean", mask="segmentation", mask_dilate=1, anchor_alpha=0.5, sft_loss_weight=0.0, auto_beta=True, auto_beta_max=50.0),
          dict(norm_type="masked_mean", mask="mask", mask_dilate=0, anchor_alpha=0.0, sft_loss_weight=0.2, auto_beta=True, auto_beta_target_gf=0.35, auto_beta_max=None,
               auto_beta_decay=0.5)]


def main():
    Distiller = load_reference()
    method_config = lift_method_config()
    out = {"shape": (B, C, H, W), "cases": [], "method_config": []}
    method = NS(value="flow_dpo")
    for cfg in ({"distillation_config": {"beta": 3.0, "norm_type": "mean"}}, {"distillation_config": {"flow_dpo": {"beta": 4.0}, "dmd": {"beta": 9.0}}},
                {"distillation_config": None}, {"distillation_config": {"flow_dpo": 5}}, {}):
        out["method_config"].append((cfg, method_config(method, cfg)))
    out["defaults"] = dict(Distiller._DEFAULTS)
    worst = float("inf")
    for ci, case in enumerate(CASES):
        teacher = Teacher(seed=100 + ci)
        dcfg = {k: v for k, v in case.items() if k != "mask"}
        dcfg["model_type"] = "lora"
        dist = Distiller(teacher, noise_scheduler=None, config=dcfg)
        calls = []
        for step in range(3 if case["auto_beta"] else 1):
            teacher.seed = 100 + ci + 1000 * step
            teacher.calls.clear()
            batch = make_batch(seed=17 * ci + step + 1, mask_kind=case["mask"])
            teacher.adapter_on = True
            pw = teacher.model_predict(batch)["model_prediction"]
            teacher.calls.clear()
            original = torch.tensor(0.37 + 0.01 * step, dtype=F32, requires_grad=True)
            loss, logs = dist.compute_distill_loss(batch, {"model_prediction": pw}, original)
            pl = next(p for on, rej, p in teacher.calls if on and rej)
            rw = next(p for on, rej, p in teacher.calls if not on and not rej)
            rl = next(p for on, rej, p in teacher.calls if not on and rej)
            gw, gl, go = torch.autograd.grad(loss, [pw, pl, original], allow_unused=True)
            mask = dist._mask_for_loss(batch, pw)
            rec = dict(batch={k: v for k, v in batch.items() if torch.is_tensor(v) or isinstance(v, str)}, policy_win=pw.detach().to(BF16), policy_lose=pl.detach().to(BF16), ref_win=rw.to(BF16),
                       ref_lose=rl.to(BF16),          # (bf16 numbers already: stored in their own width)
                       target_win=(batch["noise"].float() - batch["latents"].float()).to(BF16),
                       target_lose=(batch["noise"].float() - batch["conditioning_latents"].float()).to(BF16),
                       mask=None if mask is None else mask.float().reshape(B, -1), original_loss=original.detach(), loss=loss.detach(), logs=logs, grad_win=gw,
                       grad_lose=gl, grad_original=go, margin_ema=dist.margin_ema)
            bound, margin = margin_bound(rec, case["norm_type"])
            assert bool((margin.abs() > bound).all()), (ci, step, margin, bound)          # the input condition: every sample decided
            worst = min(worst, float((margin.abs() / bound).min()))
            calls.append(rec)
        out["cases"].append(dict(config=case, calls=calls))
    # the constructor's ValueErrors, executed
    errors = {}
    for name, kw, teach in (("norm_type", dict(norm_type="l2"), Teacher(1)), ("target_gf", dict(auto_beta_target_gf=0.5), Teacher(1)),
                            ("model_type", dict(model_type="full"), Teacher(1))):
        try:
            Distiller(teach, config={"model_type": "lora", **kw})
        except ValueError as e:
            errors[name] = str(e)
    eps = Teacher(1)
    eps.PREDICTION_TYPE = PredictionTypes.EPSILON
    try:
        Distiller(eps, config={"model_type": "lora"})
    except ValueError as e:
        errors["flow_matching"] = str(e)
    d = Distiller(Teacher(1), config={"model_type": "lora"})
    good = make_batch(1, None)
    for name, edit in (("conditioning_type", lambda b: b.update(conditioning_type="mask")), ("conditioning_latents", lambda b: b.update(conditioning_latents=None)),
                       ("missing", lambda b: (b.pop("sigmas"), b.pop("input_noise"))),
                       ("list", lambda b: b.update(conditioning_latents=[b["latents"], b["latents"]], conditioning_latents_type=["a", "b"])),
                       ("tensor", lambda b: b.update(conditioning_latents=["x"])),
                       ("shape", lambda b: b.update(conditioning_latents=b["latents"][:, :2]))):
        b = dict(good)
        edit(b)
        try:
            d.compute_distill_loss(b, {"model_prediction": torch.zeros(B, C, H, W)}, torch.zeros(()))
        except ValueError as e:
            errors[name] = str(e)
    out["errors"] = errors
    assert len(errors) == 10, errors
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(CASES)} cases, smallest |margin| / bound = {worst:.1f}, errors: {sorted(errors)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/lcm_vectors.pt by EXECUTING the reference's LCMDistiller (DDPM branch) on the CPU, seeded.

Like tools/gen_flow_dpo_golden.py: the reference package cannot be imported as a package here, so helpers/distillation/common.py (DistillationBase; pure torch) and
helpers/distillation/lcm/__init__.py are loaded as files over stand-in modules for what they import at module level — `simpletuner.helpers.models.common` (only the
PredictionTypes enum is read), `...data_backend.dataset_types` and `...distillation.registry` (a register() that does nothing), and `diffusers` (the three scheduler
names the file imports are annotations and one `from_config` call in get_scheduler, which is not executed).  The defaults are lifted from
helpers/distillation/factory.py::_create_lcm_distiller by AST.

  * the teacher is a stub plugin: its trained component is a seeded deterministic function of (sample, timestep, encoder_hidden_states) near the true epsilon / v of
    the sample, whose `enable_lora` / `disable_lora` switch a fixed perturbation — so a run that forgot to switch the adapters off would record other numbers; a
    recording wrapper keeps every call (adapter state, inputs, output): that is where x_prev and the three teacher predictions come from; the student prediction
    handed to compute_distill_loss is built so that no residual is smaller than MIN_D (`conditioned_student`: why, and the check);
  * the scheduler is a stub that carries `alphas_cumprod` (the fp32 scaled-linear schedule), `config`, and `add_noise` by the standard formula;
  * torch.randint / randn_like / rand are seeded; the draws are recorded (index, noise, guidance scale).  Case "edges" patches torch.randint so that the batch holds
    index 0 and index N - 1.

Every case runs twice on the same draws: once as the reference runs (fp32 latents: `f32`) and once with fp64 latents (`f64`: every tensor the distiller makes follows
the latents' dtype, the schedule tables stay fp32-valued), so that the restatement can be held to the executed arithmetic free of fp32 rounding as well.
Nothing of the reference is copied into the repository; only the recorded tensors are.  The reference tree is read ONLY by this script, never at test time.

    python tools/gen_lcm_golden.py
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
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "lcm_vectors.pt"
NS = types.SimpleNamespace
F32, F64 = torch.float32, torch.float64
B, C, H, W = 4, 4, 8, 8
T = 1000


class PredictionTypes(enum.Enum):
    EPSILON = "epsilon"; V_PREDICTION = "v_prediction"; FLOW_MATCHING = "flow_matching"; SAMPLE = "sample"


def load_file(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, str(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("simpletuner", "simpletuner.helpers", "simpletuner.helpers.models", "simpletuner.helpers.data_backend", "simpletuner.helpers.distillation"):
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
    if "diffusers" not in sys.modules:
        dif = types.ModuleType("diffusers")
        for name in ("DDPMScheduler", "FlowMatchEulerDiscreteScheduler", "LCMScheduler"):
            setattr(dif, name, type(name, (), {}))
        sys.modules["diffusers"] = dif
    load_file("simpletuner.helpers.distillation.common", REF / "helpers/distillation/common.py")
    return load_file("simpletuner.helpers.distillation.lcm", REF / "helpers/distillation/lcm/__init__.py")


def lift_defaults():
    """the literal `lcm_config = {...}` of DistillerFactory._create_lcm_distiller"""
    tree = ast.parse((REF / "helpers/distillation/factory.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DistillerFactory")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_create_lcm_distiller")
    assign = next(n for n in ast.walk(fn) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "lcm_config")
    return ast.literal_eval(assign.value)


def lift_full_model_error():
    src = (REF / "helpers/distillation/factory.py").read_text()
    msg = "Full model LCM distillation requires a separate student model."
    assert msg in src
    return msg


def scaled_linear_acp():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=F32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class Scheduler:
    def __init__(self, prediction_type):
        self.alphas_cumprod = scaled_linear_acp()
        self.config = NS(num_train_timesteps=T, prediction_type=prediction_type)

    def add_noise(self, original, noise, timesteps):
        acp = self.alphas_cumprod.to(dtype=original.dtype)
        a = acp[timesteps] ** 0.5
        s = (1 - acp[timesteps]) ** 0.5
        shape = (-1,) + (1,) * (original.dim() - 1)
        return a.reshape(shape) * original + s.reshape(shape) * noise


class Component:
    """the trained component: called as (sample, timestep, encoder_hidden_states, return_dict=False)[0]"""
    device = torch.device("cpu")

    def __init__(self, owner):
        self.owner = owner

    def enable_lora(self):
        self.owner.adapter_on = True

    def disable_lora(self):
        self.owner.adapter_on = False

    def __call__(self, sample, timestep, encoder_hidden_states, return_dict=False):
        o = self.owner
        out = o.predict_values(sample, timestep, encoder_hidden_states, o.adapter_on)
        o.calls.append(dict(adapter_on=o.adapter_on, sample=sample.clone(), timestep=timestep.clone(), encoder_hidden_states=encoder_hidden_states.clone(), out=out.clone()))
        return (out,)


class Teacher:
    """the stub plugin: teacher and student at once"""

    def __init__(self, prediction_type, seed):
        self.PREDICTION_TYPE = PredictionTypes.EPSILON if prediction_type == "epsilon" else PredictionTypes.V_PREDICTION
        self.ptype = prediction_type
        self.config = NS(lora_type="standard")
        self.accelerator = NS(num_processes=1)
        self.adapter_on = True
        self.seed = seed
        self.calls = []
        self.component = Component(self)
        self.acp = scaled_linear_acp()

    def get_trained_component(self):
        return self.component

    def predict_values(self, sample, timestep, ehs, adapter_on):
        """near the sample's own epsilon / v reading (an image prior of zero: eps_hat = x / sqrt(...) mixes), plus a seeded field that depends on the conditioning: the
        unconditional call (zeros) differs from the conditional one.  bf16-representable values, in the sample's dtype."""
        g = torch.Generator().manual_seed(self.seed * 7919 + int(timestep.sum()) % 1000)
        field = torch.randn(sample.shape, generator=g, dtype=F32)
        cond = ehs.float().mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        a = self.acp[timestep].sqrt().reshape(-1, 1, 1, 1)
        s = (1 - self.acp[timestep]).sqrt().reshape(-1, 1, 1, 1)
        x = sample.float()
        eps_hat = s * x + 0.3 * field + 0.5 * cond          # the posterior-mean epsilon of a unit-variance Gaussian image prior, perturbed
        out = eps_hat if self.ptype == "epsilon" else (eps_hat - s * x) / a.clamp_min(0.05) * 0.5 + 0.2 * field
        if adapter_on:
            out = out + 0.25 * torch.randn(sample.shape, generator=g, dtype=F32)
        return out.to(torch.bfloat16).to(sample.dtype)


CASES = [dict(name="epsilon_n50", prediction_type="epsilon", N=50, loss_type="l2", edges=True),
         dict(name="v_n50", prediction_type="v_prediction", N=50, loss_type="l2", edges=True),
         dict(name="epsilon_n30", prediction_type="epsilon", N=30, loss_type="huber", edges=True),          # 30 does not divide 1000: k = 33, the grid ends at 989
         dict(name="v_n30_random", prediction_type="v_prediction", N=30, loss_type="huber", edges=False)]


MIN_D = 0.05


def conditioned_student(ref, out, prediction_type, sched, seed):
    """The student prediction of the record, built backwards from the residual it should leave: m - target = d with |d| in [MIN_D, MIN_D + ~1.5], random signs.
    The input condition of the huber record: the reference subtracts `model_pred.float() - target.float()`, so the recorded d carries an fp32 rounding of ~2e-7 of its
    O(3) terms, and the huber gradient d / sqrt(d^2 + c^2) with c = 0.001 turns that into a RELATIVE error of up to 2e-7 / c = 2e-4 wherever |d| <~ c — the record
    itself would then not be reproducible to 1e-5 by any restatement.  With |d| >= MIN_D the sensitivity c^2 / (d^2 + c^2)^1.5 is below 1e-2 and the record is good to
    ~1e-8.  (Small |d| is covered where the arithmetic is bounded element-wise: tests/lcm_bounds.py.)  Checked below, on the executed loss' own operands."""
    g = torch.Generator().manual_seed(seed)
    x, tg, start = out["noisy_latents"].to(F64), out["target"].to(F64), out["timesteps"]
    r = 0.5 * torch.randn(x.shape, generator=g, dtype=F64)
    d = torch.sign(r) * (MIN_D + r.abs())
    cs, co = out["c_skip_start"].to(F64), out["c_out_start"].to(F64)
    a = sched.alphas_cumprod[start].to(F64).sqrt().reshape(-1, 1, 1, 1)
    s = (1 - sched.alphas_cumprod[start].to(F64)).sqrt().reshape(-1, 1, 1, 1)
    x0 = (tg + d - cs * x) / co
    return (x - a * x0) / s if prediction_type == "epsilon" else (a * x - x0) / s


def run_case(ref, defaults, case, ci, dtype):
    cfg = dict(defaults)
    cfg.update(num_ddim_timesteps=case["N"])
    g = torch.Generator().manual_seed(1000 + ci)
    latents = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16).to(dtype)
    ehs = torch.randn(B, 5, 16, generator=g).to(torch.bfloat16).to(dtype)
    neg = torch.randn(B, 5, 16, generator=g).to(torch.bfloat16).to(dtype) if ci % 2 else None
    teacher = Teacher(case["prediction_type"], seed=50 + ci)
    sched = Scheduler(case["prediction_type"])
    dist = ref.LCMDistiller(teacher, noise_scheduler=sched, config=cfg)
    batch = {"latents": latents, "encoder_hidden_states": ehs}
    if neg is not None:
        batch["negative_encoder_hidden_states"] = neg
    torch.manual_seed(77 + ci)
    real_randint = torch.randint
    if case["edges"]:
        fixed = torch.tensor([0, case["N"] - 1, case["N"] // 2, 1])
        torch.randint = lambda *a, **k: fixed.clone()
    try:
        out = dist.prepare_batch(dict(batch))
    finally:
        torch.randint = real_randint
    assert teacher.adapter_on and len(teacher.calls) == 3 and not any(c["adapter_on"] for c in teacher.calls)
    cond_call, uncond_call, target_call = teacher.calls
    # the student prediction at (x_s, start), adapters on, with gradient
    teacher.calls.clear()
    student = conditioned_student(ref, out, case["prediction_type"], sched, seed=300 + ci).to(dtype).requires_grad_(True)
    rec = dict(latents=latents, encoder_hidden_states=ehs, negative_encoder_hidden_states=neg, index=out["index"], noise=None, w=out["guidance_scale"].reshape(B),
               noisy_latents=out["noisy_latents"], timesteps=out["timesteps"], target_timesteps=target_call["timestep"], p_cond=cond_call["out"],
               p_uncond=uncond_call["out"], uncond_encoder_hidden_states=uncond_call["encoder_hidden_states"], x_prev=target_call["sample"], p_target=target_call["out"],
               target=out["target"], c_skip_start=out["c_skip_start"].reshape(B), c_out_start=out["c_out_start"].reshape(B), student=student.detach().clone(), losses={})
    # the noise the distiller drew: x_s = a x + s n, recovered exactly by re-drawing under the same seed in the same order
    torch.manual_seed(77 + ci)
    if not case["edges"]:
        torch.randint(0, case["N"], (B,))
    rec["noise"] = torch.randn_like(latents)
    assert torch.equal(sched.add_noise(latents, rec["noise"], out["timesteps"]), out["noisy_latents"])
    with torch.no_grad():
        m = out["c_skip_start"] * out["noisy_latents"] + out["c_out_start"] * dist._get_predicted_original_sample(student, out["timesteps"], out["noisy_latents"])
        rec["min_abs_d"] = float((m.float() - out["target"].float()).abs().min())
    assert rec["min_abs_d"] >= 0.9 * MIN_D, rec["min_abs_d"]          # the input condition
    for lt in ("l2", "huber"):
        dist.config["loss_type"] = lt
        loss, logs = dist.compute_distill_loss(out, {"model_prediction": student}, torch.tensor(123.0))
        (grad,) = torch.autograd.grad(loss, [student])
        rec["losses"][lt] = dict(loss=loss.detach(), grad=grad, logs=logs)
    return rec


def main():
    ref = load_reference()
    defaults = lift_defaults()
    defaults.pop("shift", None)
    out = {"shape": (B, C, H, W), "alphas_cumprod": scaled_linear_acp(), "defaults": defaults, "full_model_error": lift_full_model_error(),
           "text_encoder_error": sys.modules["simpletuner.helpers.distillation.common"].DISTILLATION_TEXT_ENCODER_ERROR, "cases": {}}
    for ci, case in enumerate(CASES):
        out["cases"][case["name"]] = dict(config=case, f32=run_case(ref, defaults, case, ci, F32), f64=run_case(ref, defaults, case, ci, F64))
        r = out["cases"][case["name"]]["f32"]
        print(f"{case['name']}: index {r['index'].tolist()} start {r['timesteps'].tolist()} t {r['target_timesteps'].tolist()} x_prev dtype {r['x_prev'].dtype} "
              f"l2 {float(r['losses']['l2']['loss']):.6f} huber {float(r['losses']['huber']['loss']):.6f}")
    # the solver's grids, executed
    out["solver"] = {}
    for N in (50, 30, 7):
        s = ref.DDIMSolver(scaled_linear_acp().numpy(), timesteps=T, ddim_timesteps=N)
        out["solver"][N] = dict(ddim_timesteps=s.ddim_timesteps, ddim_alpha_cumprods_prev=s.ddim_alpha_cumprods_prev)
    tt = torch.tensor([0, 1, 19, 499, 999])
    out["scalings"] = dict(timesteps=tt, values=ref.scalings_for_boundary_conditions(tt, timestep_scaling=10.0))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(CASES)} cases x (f32, f64)")


if __name__ == "__main__":
    main()

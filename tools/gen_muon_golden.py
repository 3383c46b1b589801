#!/usr/bin/env python3
"""Generate tests/golden/muon_vectors.pt by EXECUTING THE REFERENCE'S MuonClip (optimizers/muon/__init__.py, pure torch) on the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path; its one package import
(`simpletuner.helpers.training.optimizers.adamw_bfloat16.stochastic`) is satisfied by loading that file, also where it lies.  Nothing of the
reference is copied here; the tests read only the recorded tensors.  What is recorded (DESIGN.md §7 explains why it matters):

  tall_bf16_nosr   bf16 tall matrices, stochastic_rounding=False, 3 steps: the reference is correct Muon there (the transposed view is not
                   contiguous, so torch.addmm computes into a temporary) -> the restatement must match
  cans             use_cans=True on a wide and a tall bf16 matrix (stochastic_rounding=False), 2 steps: the CANS branch writes into a
                   separate buffer -> must match
  defect_alias     _zeropower_via_newtonschulz on wide / square inputs: `addmm(X, B, X, out=X)` overwrites its own operand -> recorded
                   output, the restatement must DIFFER from it
  defect_fp32_mom  fp32 tall parameter, 2 steps: X.to(float32) aliases the momentum buffer, which ends up holding the iterate; the first
                   step's parameter is right, the buffer and the second step are not
  defect_bf16_sr   bf16 tall parameter, stochastic_rounding=True: add_stochastic_(p, O, alpha=-lr) computes O - lr p
  qk_clip_lora     LoRA-named parameters + max logits keyed by the base layer name: the step equals the same step without logits
  default_settings the registry entry (optimizer_param.py:432-447), read from the source with ast

    python tools/gen_muon_golden.py <SimpleTuner checkout>      (writes tests/golden/muon_vectors.pt)
"""
from __future__ import annotations

import ast
import importlib.util
import sys
import types
from pathlib import Path

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "muon_vectors.pt"


def _load(ref: Path):
    stoch_path = ref / "helpers/training/optimizers/adamw_bfloat16/stochastic/__init__.py"
    spec = importlib.util.spec_from_file_location("ref_stochastic", stoch_path)
    stoch = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stoch)
    names = ["simpletuner", "simpletuner.helpers", "simpletuner.helpers.training", "simpletuner.helpers.training.optimizers",
             "simpletuner.helpers.training.optimizers.adamw_bfloat16"]
    for n in names:
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["simpletuner.helpers.training.optimizers.adamw_bfloat16.stochastic"] = stoch
    spec = importlib.util.spec_from_file_location("ref_muon", ref / "helpers/training/optimizers/muon/__init__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, stoch


def _default_settings(ref: Path) -> dict:
    tree = ast.parse((ref / "helpers/training/optimizer_param.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Dict):
            for k, v in zip(node.keys, node.values):
                if isinstance(k, ast.Constant) and k.value == "muon" and isinstance(v, ast.Dict):
                    for k2, v2 in zip(v.keys, v.values):
                        if isinstance(k2, ast.Constant) and k2.value == "default_settings":
                            return ast.literal_eval(v2)
    raise KeyError("optimizer_param.py: no 'muon' entry")


def _run(mod, shapes, dtype, steps, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((0.1 * torch.randn(s, generator=g)).to(dtype)) for s in shapes]
    p0 = [p.detach().clone() for p in ps]
    grads = [[torch.randn(s, generator=g).to(dtype) for s in shapes] for _ in range(steps)]
    opt = mod.MuonClip(ps, **kw)
    traj = []
    for k in range(steps):
        for p, gr in zip(ps, grads[k]):
            p.grad = gr.clone()
        opt.step()
        traj.append([p.detach().clone() for p in ps])
    mom = [opt.state[p]["momentum_buffer"].clone() for p in ps]
    return dict(p0=p0, grads=grads, traj=traj, momentum=mom, settings=dict(kw), dtype=str(dtype))


def main(ref: Path):
    mod, stoch = _load(ref)
    out = {}
    out["tall_bf16_nosr"] = _run(mod, [(96, 16), (160, 32)], torch.bfloat16, 3, 11, lr=2e-2, stochastic_rounding=False)
    out["cans"] = _run(mod, [(16, 96), (96, 16)], torch.bfloat16, 2, 12, lr=2e-2, use_cans=True, stochastic_rounding=False)
    ali = {}
    g = torch.Generator().manual_seed(13)
    for name, shape in (("wide_32x512", (32, 512)), ("square_64", (64, 64)), ("wide_16x200", (16, 200)), ("tall_200x16", (200, 16))):
        x = torch.randn(shape, generator=g)
        ali[name] = dict(x=x, out=mod._zeropower_via_newtonschulz(x.clone()))
    out["defect_alias"] = ali
    out["defect_fp32_mom"] = _run(mod, [(96, 16)], torch.float32, 2, 14, lr=2e-2)
    torch.manual_seed(15)                                   # add_stochastic_ draws from the global generator
    out["defect_bf16_sr"] = _run(mod, [(96, 16)], torch.bfloat16, 1, 15, lr=2e-2, weight_decay=0.0, stochastic_rounding=True)
    # QK-clip under LoRA names: the logits are keyed by the base layer's weight name, the optimizer holds only lora_A / lora_B
    g = torch.Generator().manual_seed(16)
    names = ["transformer_blocks.0.attn.to_q.lora_A.default.weight", "transformer_blocks.0.attn.to_q.lora_B.default.weight"]
    ps = [torch.nn.Parameter(0.1 * torch.randn(s, generator=g)) for s in ((8, 64), (64, 8))]
    p0 = [p.detach().clone() for p in ps]
    grads = [torch.randn(p.shape, generator=g) for p in ps]
    logits = {"transformer_blocks.0.attn.to_q.weight": torch.full((4,), 1e4)}
    after = {}
    for key, lg in (("with_logits", logits), ("without_logits", None)):
        qs = [torch.nn.Parameter(p.clone()) for p in p0]
        opt = mod.MuonClip(qs, lr=2e-2, qk_clip_threshold=1.0)
        opt.register_attention_params(dict(zip(names, qs)))
        for q, gr in zip(qs, grads):
            q.grad = gr.clone()
        opt.step(attention_max_logits=lg)
        after[key] = [q.detach().clone() for q in qs]
    out["qk_clip_lora"] = dict(names=names, p0=p0, grads=grads, logits=logits, after=after, state_dict_param_names=opt.state_dict()["param_names"])
    out["default_settings"] = _default_settings(ref)
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]) / "simpletuner")

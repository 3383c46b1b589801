#!/usr/bin/env python3
"""Generate tests/golden/nextlat_vectors.pt by EXECUTING THE REFERENCE'S NextLat module (helpers/training/nextlat.py, pure torch) on the CPU.

The module is loaded where it lies in a SimpleTuner checkout, by file path, at generation time only; nothing of it is copied here and the tests read only the
recorded tensors, numbers and messages.  Recorded (B = 2, 35 tokens, D = 64, fp32, all six parameters seeded non-zero — a zero `down` would make the gradient into
the hidden states and four of the six parameter gradients vanish):

  smooth_l1 / mse   hidden states, the weight; the predictor's output on h[:, :-1]; `compute_loss`'s loss and logs; autograd.grad of the loss with respect to the
                    hidden states and the six parameters; the share of |pred - target| >= 1, smooth-L1's linear regime (asserted here to lie in [0.1, 0.9]: at least 10 % in each regime)
  constant_row      the same (smooth-L1) with one constant row (xhat = 0)
  index_table       the block the reference resolves for 3 blocks and a configured None / 0 / -1 / 2 / 1
  init              what a fresh predictor holds: `down` zero, LayerNorm (1, 0), the bound of `up`
  errors            every ValueError text
  state_keys        `state_dict()` keys, `block_index`'s dtype and shape, MODULE_NAME

    python tools/gen_nextlat_golden.py <SimpleTuner checkout>      (writes tests/golden/nextlat_vectors.pt)
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "nextlat_vectors.pt"
B, S, D = 2, 35, 64
NAMES = ("norm.weight", "norm.bias", "up.weight", "up.bias", "down.weight", "down.bias")


def _load(ref: Path):
    spec = importlib.util.spec_from_file_location("ref_nextlat", ref / "helpers/training/nextlat.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))


def _err(fn, kind=ValueError):
    try:
        fn()
    except kind as e:
        return str(e)
    raise AssertionError(f"expected a {kind.__name__}")


def _cfg(**kw):
    return SimpleNamespace(nextlat_enabled=True, **{"nextlat_weight": 0.3, **kw})


ACC = SimpleNamespace(device=torch.device("cpu"))


def _regulariser(mod, params, n_blocks=3, **kw):
    reg = mod.NextLatRegularizer(_cfg(**kw), ACC, D, n_blocks)
    model = _Model()
    reg.attach_to_model(model, torch.float32)
    if params is not None:
        own = dict(reg.predictor.named_parameters())
        with torch.no_grad():
            for nm in NAMES:
                own[nm].copy_(params[nm])
    return reg, model


def _run(mod, params, hidden, weight, state_loss):
    reg, _ = _regulariser(mod, params, nextlat_weight=weight, nextlat_state_loss=state_loss, nextlat_block_index=1)
    h = hidden.clone().requires_grad_(True)
    pred = reg.predictor(h[:, :-1])
    loss, logs = reg.compute_loss({f"layer_{reg.block_index}": h}, {})
    own = dict(reg.predictor.named_parameters())
    grads = torch.autograd.grad(loss, [h] + [own[nm] for nm in NAMES])
    linear_share = float(((pred.detach() - hidden[:, 1:]).abs() >= 1).float().mean())
    return {"hidden": hidden, "weight": float(weight), "state_loss": state_loss, "block": int(reg.block_index), "prediction": pred.detach(), "loss": loss.detach(),
            "logs": dict(logs), "grad_hidden": grads[0], "grads": {nm: g for nm, g in zip(NAMES, grads[1:])}, "linear_share": linear_share}


def main(ref: Path):
    mod = _load(ref)
    g = torch.Generator().manual_seed(9731)
    hidden = torch.randn(B, S, D, generator=g)
    params = {"norm.weight": 1.0 + 0.25 * torch.randn(D, generator=g), "norm.bias": 0.1 * torch.randn(D, generator=g),
              "up.weight": torch.randn(2 * D, D, generator=g) / D ** 0.5, "up.bias": 0.05 * torch.randn(2 * D, generator=g),
              "down.weight": torch.randn(D, 2 * D, generator=g) / (2 * D) ** 0.5, "down.bias": 0.05 * torch.randn(D, generator=g)}
    out = {"shape": (B, S, D), "params": params}
    out["smooth_l1"] = _run(mod, params, hidden, 0.3, "smooth_l1")
    out["mse"] = _run(mod, params, hidden, 0.3, "mse")
    share = out["smooth_l1"]["linear_share"]
    assert 0.10 <= share <= 0.90, f"smooth-L1 regimes: {share:.3f} of the elements in the linear regime, need at least 10 % in each"
    hc = hidden.clone()
    hc[0, 3] = 0.375                                   # constant row: xhat = 0, rstd = 1 / sqrt(eps)
    out["constant_row"] = dict(_run(mod, params, hc, 0.3, "smooth_l1"), row=(0, 3))
    # row S - 1 of every sample: exactly zero gradient (only the detached target reads it)
    assert all(float(out[k]["grad_hidden"][:, -1].abs().max()) == 0.0 for k in ("smooth_l1", "mse", "constant_row"))
    out["index_table"] = {repr(c): int(mod.NextLatRegularizer(_cfg(nextlat_block_index=c), ACC, D, 3).block_index) for c in (None, 0, -1, 2, 1)}
    fresh = mod.NextLatPredictor(D, 1)
    out["init"] = {"down_zero": bool((fresh.down.weight == 0).all() and (fresh.down.bias == 0).all()), "norm_weight_one": bool((fresh.norm.weight == 1).all()),
                   "norm_bias_zero": bool((fresh.norm.bias == 0).all()), "up_abs_max": float(fresh.up.weight.detach().abs().max()), "up_bound": 1.0 / D ** 0.5,
                   "eps": float(fresh.norm.eps)}
    R = mod.NextLatRegularizer
    reg, _ = _regulariser(mod, params)
    reg_kl, _ = _regulariser(mod, params, nextlat_kl_weight=0.5)
    unattached = R(_cfg(), ACC, D, 3)
    out["errors"] = {
        "zero_weight": _err(lambda: R(_cfg(nextlat_weight=0), ACC, D, 3)),
        "bad_weight": _err(lambda: R(_cfg(nextlat_weight=-0.5), ACC, D, 3)),
        "index_high": _err(lambda: R(_cfg(nextlat_block_index=3), ACC, D, 3)),
        "bad_state_loss": _err(lambda: R(_cfg(nextlat_state_loss="l1"), ACC, D, 3)),
        "bad_kl": _err(lambda: R(_cfg(nextlat_kl_weight=-1.0), ACC, D, 3)),
        "kl_no_head": _err(lambda: reg_kl.compute_loss({f"layer_{reg_kl.block_index}": hidden}, {})),
        "no_buffer": _err(lambda: reg.compute_loss(None, {})),
        "not_captured": _err(lambda: reg.compute_loss({"layer_0": hidden}, {})),
        "one_token": _err(lambda: reg.compute_loss({f"layer_{reg.block_index}": hidden[:, :1]}, {})),
        "two_dims": _err(lambda: reg.predictor(hidden[0, 0])),
        "unattached": _err(lambda: unattached.compute_loss({f"layer_{unattached.block_index}": hidden}, {}), RuntimeError),
    }
    sd = reg.predictor.state_dict()
    out["state_keys"] = {"keys": list(sd.keys()), "block_index_dtype": str(sd["block_index"].dtype), "block_index_shape": tuple(sd["block_index"].shape),
                         "block_index": int(sd["block_index"]), "module_name": R.MODULE_NAME,
                         "shapes": {k: tuple(v.shape) for k, v in sd.items()}}
    torch.save(out, OUT)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); linear regime share {share:.3f}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))

"""state_dict() -> load_state_dict() of the four fused optimizers, one contract for all: a freshly built optimizer that loads a saved state continues
bit for bit — parameters, flat state buffers, per-parameter state — and keeps every buffer in the dtype the class declares (never torch's "cast the state
to the parameter's dtype").  The `ops.*` calls are the CPU stand-ins of tests/ops_emulator.py, tests/lion_bounds.py and tests/muon_ref.py."""
import copy

import pytest
import torch

from tests import lion_bounds, muon_ref, ops_emulator

F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(8, 16), (16, 8), (8, 8)]
N = sum(r * c for r, c in SHAPES)
NAMES = ["blocks.0.attn.to_q.lora_A", "blocks.0.attn.to_k.lora_A", "blocks.0.attn.to_v.lora_A"]

# case -> (class name, parameter dtype, constructor keywords, {state key: dtype}, {state key: key in _flat[0]})
CASES = {
    "adamw-fp32": ("St355AdamW", F32, dict(lr=1e-2, weight_decay=1e-2), {"exp_avg": F32, "exp_avg_sq": F32}, {"exp_avg": "m", "exp_avg_sq": "v"}),
    "adamw-bf16": ("St355AdamW", BF16, dict(lr=1e-2, weight_decay=1e-2), {"exp_avg": F32, "exp_avg_sq": F32}, {"exp_avg": "m", "exp_avg_sq": "v"}),
    "adamw_bf16": ("St355AdamWBF16", BF16, dict(lr=1e-3, weight_decay=1.0, seed=3), {"exp_avg": BF16, "exp_avg_sq": BF16, "shift": BF16},
                   {"exp_avg": "m", "exp_avg_sq": "v", "shift": "shift"}),
    "lion-bf16": ("St355Lion", BF16, dict(lr=1e-3, weight_decay=1e-2), {"exp_avg": BF16, "kahan_comp": BF16}, {"exp_avg": "m", "kahan_comp": "comp"}),
    "lion-fp32": ("St355Lion", F32, dict(lr=1e-3, weight_decay=1e-2), {"exp_avg": F32}, {"exp_avg": "m"}),
    "muon-fp32": ("St355Muon", F32, dict(lr=1e-2), {"momentum_buffer": F32}, {"momentum_buffer": "m"}),
}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _arena(dtype, init):
    flat, grad = init.to(dtype).clone(), torch.zeros(N, dtype=dtype)
    ps, off = [], 0
    for s in SHAPES:
        k = s[0] * s[1]
        p = torch.nn.Parameter(flat[off:off + k].view(s))
        p.grad = grad[off:off + k].view(s)
        ps.append(p)
        off += k
    return flat, grad, ps


def _step(opt, grad, step):
    grad.copy_((1e-2 * torch.randn(N, generator=torch.Generator().manual_seed(100 + step))).to(grad.dtype))
    opt.step()


def _same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what
    else:
        assert a == b, what


@pytest.mark.parametrize("case", list(CASES))
def test_a_loaded_optimizer_continues_bit_for_bit_in_the_declared_dtypes(monkeypatch, case):
    from simpletuner_amd.training import optimizer as O
    ops_emulator.install(monkeypatch)
    lion_bounds.install(monkeypatch)
    muon_ref.install(monkeypatch)
    cls_name, dtype, kw, dtypes, flat_keys = CASES[case]
    cls = getattr(O, cls_name)
    init = 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(7))

    a_flat, a_grad, a_ps = _arena(dtype, init)
    a = cls(a_ps, **kw)
    assert not a.state and not a._flat                              # state is created on the first step or on load, not in the constructor
    if cls_name == "St355Muon":
        a.register_attention_params(dict(zip(NAMES, a_ps)))
    for s in (1, 2):
        _step(a, a_grad, s)
    saved = copy.deepcopy(a.state_dict())                           # the live state tensors are views of buffers that the next step overwrites
    assert sorted(saved["state"]) == [0, 1, 2]

    b_flat, b_grad, b_ps = _arena(dtype, a_flat.float())            # the model weights come from the checkpoint
    b = cls(b_ps, **dict(kw, lr=0.5))
    b.load_state_dict(saved)
    assert b.param_groups[0]["lr"] == kw["lr"]                      # saved hyper-parameters replace the live ones
    fb = b._flat[0]
    for p in b_ps:                                                  # loaded buffers: declared dtype, views of the flat buffers
        assert {k for k, v in b.state[p].items() if isinstance(v, torch.Tensor) and v.dim() > 0} == set(dtypes)
        for key, dt in dtypes.items():
            t = b.state[p][key]
            assert t.dtype == dt and t.shape == p.shape, (key, t.dtype)
            assert fb[flat_keys[key]].dtype == dt
            assert t.untyped_storage().data_ptr() == fb[flat_keys[key]].untyped_storage().data_ptr(), key
    if case == "lion-fp32":
        assert fb["comp"] is None

    _step(a, a_grad, 3)
    _step(b, b_grad, 3)
    assert torch.equal(_bits(a_flat), _bits(b_flat))
    fa = a._flat[0]
    assert set(fa) - {"zero_decay"} == set(fb) - {"zero_decay"}         # (zero_decay: a vector cached by the first step that releases no decay)
    for key in set(fa) & set(fb):
        if key not in ("ps", "plan"):
            _same(fa[key], fb[key], f"_flat[0][{key!r}]")
    if "plan" in fa:
        assert fa["plan"].mats == fb["plan"].mats
    for i, (pa, pb) in enumerate(zip(a_ps, b_ps)):
        sa, sb = a.state[pa], b.state[pb]
        assert set(sa) == set(sb), i
        for key in sa:
            _same(sa[key], sb[key], f"state[{i}][{key!r}]")
    if cls_name == "St355AdamW":
        assert all(a.state[p]["step"].dim() == 0 and float(a.state[p]["step"]) == 3.0 for p in a_ps) and fa["step"] == 3
    if cls_name == "St355AdamWBF16":
        assert all(type(b.state[p]["step"]) is float and b.state[p]["step"] == 3.0 and type(b.state[p]["accumulated_decay"]) is float for p in b_ps)
        assert len({b.state[p]["accumulated_decay"] for p in b_ps}) == 3          # one phase per tensor, carried through the checkpoint
    if cls_name == "St355Muon":
        assert all(b.state[p]["factored"] is False for p in b_ps)
        assert b.state_dict()["param_names"] == a.state_dict()["param_names"] == {0: NAMES}

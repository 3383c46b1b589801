"""Muon on the MI355X: the grouped Newton-Schulz kernel and the fused step (simpletuner_amd/csrc/muon.hip) against the fp64 restatement
(tests/muon_ref.py), element-wise, with bounds derived from the fp32 summation error of the kernel (v_mfma_f32_32x32x2_f32 is a k-ordered
fp32 fma chain: |error| <= gamma_K sum |a b|, gamma_K = K u / (1 - K u), u = 2^-24), in the style of tests/gemm_bounds.py."""
import math

import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.training.optimizer import St355Muon
from tests import muon_ref as MR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
F64 = torch.float64


def gamma(k):
    return k * U / (1 - k * U)


def _arena(shapes, gen, scale=None):
    mats = []
    for i, s in enumerate(shapes):
        x = torch.randn(s, generator=gen, dtype=torch.float32)
        if scale is not None and scale[i] is not None:
            x = x * scale[i]
        mats.append(x)
    offs, o = [], 0
    for x in mats:
        offs.append(o)
        o += x.numel()
    flat = torch.cat([x.reshape(-1) for x in mats]).to(DEV)
    return flat, offs


def _views(flat, offs, shapes):
    return [flat[o:o + s[0] * s[1]].view(s) for o, s in zip(offs, shapes)]


def _iter_bound(X, EX, abc, L, nch):
    """element-wise bound on |kernel - fp64| for one iteration X -> a X + (b A + c A A) X in the short x long orientation, given the input's
    own error bound EX (|.| products in fp64)"""
    a, b, c = abc
    R = X.shape[0]
    aX = X.abs()
    A = aX @ aX.T
    EA = aX @ EX.T + EX @ aX.T + gamma(L + nch + 4) * A
    B = abs(b) * A + abs(c) * (A @ A)
    EB = abs(b) * EA + abs(c) * (EA @ A + A @ EA + gamma(R) * (A @ A)) + 2 * U * B
    return abs(a) * EX + EB @ aX + B @ EX + gamma(R + 2) * (abs(a) * aX + B @ aX)


def _short_long(x):
    return x.T if x.shape[0] > x.shape[1] else x


SHORT = (8, 16, 32, 64, 128)
LONG = (3072, 12288, 15360, 1000)


def _shapes():
    out = []
    for r in SHORT:
        for L in LONG:
            if r == 128 and L == 15360:
                out.append((L, r))           # one per (r, L): alternate orientations, both present for every short side
            else:
                out.append((r, L) if (r // 8 + L) % 2 else (L, r))
    out += [(24, 5000), (5000, 24)]
    return out


def test_orthogonalisation_one_iteration_at_a_time_is_bounded_against_fp64():
    shapes = _shapes()
    gen = torch.Generator().manual_seed(0)
    flat, offs = _arena(shapes, gen)
    plan = ops.MuonPlan(offs, shapes, DEV)
    coeffs = MR.coefficients()
    worst = 0.0
    x = flat
    for it, abc in enumerate(coeffs):
        y = ops.muon_orthogonalize(plan, x, [abc], normalize=(it == 0))
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        for xin, yout, s in zip(_views(x, offs, shapes), _views(y, offs, shapes), shapes):
            X = _short_long(xin.to(F64))
            L = max(s)
            nch = (L + 511) // 512
            if it == 0:
                nrm = X.norm().clamp(min=1e-7)
                EX = (2 * U + gamma(X.numel())) * X.abs() / nrm
                X = X / nrm
            else:
                EX = torch.zeros_like(X)
            ref = _short_long(MR.ns_fp64(X if X.shape[0] <= X.shape[1] else X, [abc], normalize=False))
            bound = _iter_bound(X, EX, abc, L, nch)
            err = (_short_long(yout.to(F64)) - ref).abs()
            ratio = (err / bound.clamp(min=1e-300)).max().item()
            worst = max(worst, ratio)
            assert (err <= bound).all(), (it, s, ratio)
        x = y
    print(f"[muon] worst |err| / bound over {len(shapes)} matrices x 5 iterations: {worst:.3f}")


def test_zero_and_tiny_norm_matrices():
    shapes = [(32, 3072), (3072, 32), (16, 1000), (1000, 16)]
    gen = torch.Generator().manual_seed(1)
    flat, offs = _arena(shapes, gen, scale=[0.0, 1e-9, 1e-12, 1e-9])
    plan = ops.MuonPlan(offs, shapes, DEV)
    y = ops.muon_orthogonalize(plan, flat, MR.coefficients(), normalize=True)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    v = _views(y, offs, shapes)
    assert torch.equal(v[0], torch.zeros_like(v[0]))                          # an exact-zero matrix gives zeros, not NaN
    for xin, yout in zip(_views(flat, offs, shapes)[1:], v[1:]):
        ref = MR.ns_fp64(xin, MR.coefficients())
        assert (yout.to(F64) - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())


def _step_bound(m, abc_list, L, nch):
    """bound of the orthogonalised update of one matrix through all iterations (the input normalised in the kernel)"""
    X = _short_long(m.to(F64))
    nrm = X.norm().clamp(min=1e-7)
    EX = (2 * U + gamma(X.numel())) * X.abs() / nrm
    X = X / nrm
    for abc in abc_list:
        EX = _iter_bound(X, EX, abc, L, nch)
        a, b, c = abc
        A = X @ X.T
        X = a * X + (b * A + c * (A @ A)) @ X
    return X, EX


def test_full_step_is_bounded_against_fp64_over_five_steps():
    shapes = [(32, 3072), (3072, 32), (16, 12288), (12288, 16), (64, 1000), (128, 128), (8, 333)]
    gen = torch.Generator().manual_seed(2)
    pflat, offs = _arena(shapes, gen, scale=[0.05] * len(shapes))
    ps = [torch.nn.Parameter(v) for v in _views(pflat, offs, shapes)]
    gflat = torch.zeros_like(pflat)
    for p, g in zip(ps, _views(gflat, offs, shapes)):
        p.grad = g
    lr, wd, mu, rms, sc = 3e-3, 0.1, 0.95, 0.2, 0.5
    opt = St355Muon(ps, lr=lr, weight_decay=wd, momentum=mu, rms_scale_factor=rms)
    opt.grad_scale = sc
    coeffs = MR.coefficients()
    for step in range(5):
        gflat.copy_(torch.randn(pflat.numel(), generator=gen).to(DEV))
        opt._group_flat(0, opt.param_groups[0])
        p_before = [p.detach().to(F64).clone() for p in ps]
        m_before = [opt.state[p]["momentum_buffer"].to(F64).clone() for p in ps]
        opt.step()
        torch.cuda.synchronize()
        for p, p0, m0, g in zip(ps, p_before, m_before, _views(gflat, offs, shapes)):
            m_ref = m0 + (1 - mu) * (sc * g.to(F64) - m0)
            m_k = opt.state[p]["momentum_buffer"].to(F64)
            assert (m_k - m_ref).abs().max().item() <= 4 * U * (m0.abs() + g.to(F64).abs()).max().item() + 1e-30
            L = max(p.shape)
            Xs, EX = _step_bound(m_k, coeffs, L, (L + 511) // 512)     # from the kernel's own momentum
            sf = math.sqrt(L) * rms
            tall = p.shape[0] > p.shape[1]
            O = (Xs.T if tall else Xs) * sf
            EO = (EX.T if tall else EX) * sf + 3 * U * O.abs()
            p_ref = p0 + (-lr * wd) * p0 + (-lr) * O
            bound = lr * EO + 3 * U * (p0.abs() + lr * O.abs())
            err = (p.detach().to(F64) - p_ref).abs()
            assert (err <= bound).all(), (step, tuple(p.shape), (err / bound).max().item())


def test_two_runs_are_bit_identical_and_abi_calls_do_not_grow_with_the_matrix_count(monkeypatch):
    calls = []
    real = ops.muon_step
    monkeypatch.setattr(ops, "muon_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(nmat):
        shapes = [(32, 3072), (3072, 32)] * nmat
        gen = torch.Generator().manual_seed(3)
        pflat, offs = _arena(shapes, gen, scale=[0.05] * len(shapes))
        gflat = torch.randn(pflat.numel(), generator=gen).to(DEV)
        ps = [torch.nn.Parameter(v) for v in _views(pflat, offs, shapes)]
        for p, g in zip(ps, _views(gflat, offs, shapes)):
            p.grad = g
        opt = St355Muon(ps, lr=1e-3)
        calls.clear()
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        return pflat.clone(), opt._flat[0]["m"].clone(), len(calls), opt._flat[0]["plan"].launches(5)

    a = run(3)
    b = run(3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = run(40)
    assert a[2] == c[2] == 3                                 # one ABI call per step
    assert a[3] == c[3] == 2 + 3 * 5                          # launches of a call: independent of the number of matrices


def test_captured_step_equals_eager_step_bit_for_bit():
    shapes = [(32, 3072), (3072, 32), (16, 1000), (64, 12288)]

    def make():
        gen = torch.Generator().manual_seed(4)
        pflat, offs = _arena(shapes, gen, scale=[0.05] * len(shapes))
        gflat = torch.randn(pflat.numel(), generator=gen).to(DEV)
        ps = [torch.nn.Parameter(v) for v in _views(pflat, offs, shapes)]
        for p, g in zip(ps, _views(gflat, offs, shapes)):
            p.grad = g
        opt = St355Muon(ps, lr=1e-3)
        opt.step()                      # plan, workspace and momentum arena are made here, outside any capture
        return pflat, opt

    pe, oe = make()
    pg, og = make()
    oe.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        og.step()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pe, pg)
    assert torch.equal(oe._flat[0]["m"], og._flat[0]["m"])


def test_flux_lora_trajectory_with_muon_matches_the_oracle_and_the_fp64_restatement():
    """20 steps of Flux LoRA at reduced depth with optimizer='muon' through the trainer, against the fp32 oracle model whose adapters are stepped
    by the fp64 Muon restatement.  Stated bounds: |loss difference| <= 2e-3 per step and adapter values within 0.25 lr * steps"""
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU

    steps, lr = 20, 1e-3
    cfg = default_config(lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=lr, optimizer="muon")
    acc = St355Accelerator(DEV)
    plugin = Flux(cfg, acc)
    plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    plugin.add_lora_adapter()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Muon)
    cpu, devt = PU.make_inputs(1, 16, 16, 64, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    model = plugin.get_trained_component()
    P, lora, scale = PU.oracle_state(model)
    ocfg = PU.oracle_cfg(model)
    mom = {k: (torch.zeros_like(a, dtype=F64), torch.zeros_like(b, dtype=F64)) for k, (a, b) in lora.items()}
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    worst = 0.0
    for _ in range(steps):
        loss = trainer.train_step(dict(batch))
        o_loss, _, grads = PU.oracle_step(P, ocfg, lora, scale, cpu)
        worst = max(worst, abs(loss.item() - o_loss.item()))
        new_lora, new_mom = {}, {}
        for k, (a, b) in lora.items():
            (pa, pb), (ma, mb) = MR.muon_step_fp64([a.detach(), b.detach()], [grads[k][0], grads[k][1]], [mom[k][0], mom[k][1]], lr)
            new_lora[k] = (pa.float(), pb.float())
            new_mom[k] = (ma, mb)
        lora, mom = new_lora, new_mom
    torch.cuda.synchronize()
    _, lora_k, _ = PU.oracle_state(model)
    dev_max = max(max((lora_k[k][0] - lora[k][0]).abs().max().item(), (lora_k[k][1] - lora[k][1]).abs().max().item()) for k in lora)
    print(f"[muon] flux lora 20 steps: max |d loss| = {worst:.3e}, max |d adapter| = {dev_max:.3e} (lr {lr})")
    assert worst <= 2e-3
    assert dev_max <= 0.25 * lr * steps

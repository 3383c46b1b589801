"""SOAP on the MI355X (simpletuner_amd/csrc/soap.hip): the fused step bounded element-wise against fp64 (tests/soap_bounds.py), the batched
eigensolver and the refresh against what torch.linalg.eigh reaches in fp32, the recorded reference trajectories (tests/golden/soap_vectors.pt) and
the optimizer's host behaviour through a Flux LoRA train step."""
import copy
import math
from pathlib import Path

import pytest
import torch

from simpletuner_amd import ops
from simpletuner_amd.training.optimizer import St355Soap
from tests import soap_bounds as SB
from tests import soap_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
F32 = torch.float32
GOLD = torch.load(Path(__file__).resolve().parent / "golden" / "soap_vectors.pt")

SHORT = (4, 32, 48, 128)              # padding below 32, an exact class, padding to 64, the LDS maximum
LONG = (129, 200, 513, 1100)          # shorter than a 512 chunk, not a multiple of 4, one past a chunk, three chunks with a tail (spot check of 32-column tiles too)
SHAPES = [s for r in SHORT for L in LONG for s in ((r, L), (L, r))]


def _arena(shapes, seed, scale=0.05, values=None):
    gen = torch.Generator().manual_seed(seed)
    mats = [scale * torch.randn(s, generator=gen) for s in shapes] if values is None else [v.clone() for v in values]
    pflat = torch.cat([x.reshape(-1) for x in mats]).to(DEV)
    gflat = torch.zeros_like(pflat)
    ps, off = [], 0
    for s in shapes:
        k = s[0] * s[1]
        p = torch.nn.Parameter(pflat[off:off + k].view(s))
        p.grad = gflat[off:off + k].view(s)
        ps.append(p)
        off += k
    return pflat, gflat, ps, gen


def _set_grads(gflat, shapes, grads):
    gflat.copy_(torch.cat([g.reshape(-1) for g in grads]).to(DEV))


def _ortho_err(q):
    q = q.to(F64).cpu()
    return float((q.T @ q - torch.eye(q.shape[0], dtype=F64)).norm())


def _resid(a, q, lam):
    a, q, lam = a.to(F64).cpu(), q.to(F64).cpu(), lam.to(F64).cpu()
    na = float(a.norm())
    num = float((a @ q - q * lam).norm())
    return num / na if na > 0 else num


# ---- the fused step, every element bounded ---------------------------------------------------------------------------------------------------------
def test_step_is_bounded_element_wise_against_fp64_and_the_first_call_only_builds_the_basis():
    lr, betas, eps, wd, sb, gs = 3e-3, (0.95, 0.9), 1e-8, 0.01, 0.8, 0.5
    pflat, gflat, ps, gen = _arena(SHAPES, 0)
    opt = St355Soap(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, shampoo_beta=sb, max_precond_dim=128, precondition_frequency=1000)
    opt.grad_scale = gs
    p_start = pflat.clone()
    worst = dict(m=0.0, v=0.0, p=0.0, GG=0.0)
    loose = 0.0
    for call in range(3):
        gflat.copy_(torch.randn(pflat.numel(), generator=gen).to(DEV))
        st = opt._group_flat(0, opt.param_groups[0])
        before = {k: st[k].clone() for k in ("m", "v", "gg", "q")}
        p_before = pflat.clone()
        opt.step()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in (pflat, st["m"], st["v"], st["gg"], st["q"]))
        if call == 0:
            assert torch.equal(pflat, p_start) and not st["m"].any() and not st["v"].any()        # bit-unchanged, exp_avg zero
            assert all(opt.state[p]["step"] == 0 for p in ps) and st["step"] == 0
        t = max(call, 1)
        c = SB.consts(gs, betas[0], betas[1], eps, SB.step_size(lr, betas, t), lr * wd, 1.0 - sb)
        off = 0
        for i, p in enumerate(ps):
            n, r, qo = p.numel(), st["plan"].short[i], st["plan"].q_offsets[i]
            wide = p.shape[0] < p.shape[1]
            view = lambda flat: flat[off:off + n].view(p.shape).cpu()
            blk = lambda flat: flat[qo:qo + r * r].view(r, r).cpu()
            Q = blk(before["q"]) if call else torch.eye(r)
            x = SR.one_step_fp64(view(p_before), view(gflat), view(before["m"]), view(before["v"]), Q, blk(before["gg"]), wide, c)
            b = SB.step_bounds(x, c, max(p.shape))
            name = f"call {call} {tuple(p.shape)}"
            worst["GG"] = SB.check(name + " GG", blk(st["gg"]), x["GG1"], b["GG"], worst["GG"])
            if call:
                loose = max(loose, b["loose"])
                worst["m"] = SB.check(name + " exp_avg", SB.orient(view(st["m"]), wide), x["m1"], b["m"], worst["m"])
                worst["v"] = SB.check(name + " exp_avg_sq", SB.orient(view(st["v"]), wide), x["v1"], b["v"], worst["v"])
                worst["p"] = SB.check(name + " p", SB.orient(view(pflat), wide), x["p2"], b["p"], worst["p"])
            off += n
    print(f"[soap] worst |err| / bound over {len(SHAPES)} matrices x 2 steps: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; largest share of loosely bounded elements {loose:.2e}")
    assert loose <= 1e-3


# ---- the eigensolver ---------------------------------------------------------------------------------------------------------------------------------
def test_eigh_reaches_what_lapack_reaches_in_fp32():
    gen = torch.Generator().manual_seed(1)
    mats, kinds = [], []
    for r in SHORT + (1, 33):
        x = torch.randn(r, r + 7, generator=gen)
        mats.append(x @ x.T); kinds.append("spd")
        k = max(r - 3, 1) if r > 4 else 2
        y = torch.randn(r, k, generator=gen) if r > 1 else torch.zeros(1, 1)
        mats.append(y @ y.T); kinds.append("deficient")                       # a few exactly-zero eigenvalues
        mats.append(torch.zeros(r, r)); kinds.append("zero")
    shapes = [(a.shape[0], a.shape[0] + 1) for a in mats]
    offs, o = [], 0
    for s in shapes:
        offs.append(o)
        o += s[0] * s[1]
    plan = ops.SoapPlan(offs, shapes, DEV)
    gg = torch.cat([a.reshape(-1) for a in mats]).to(DEV)
    q, lam = ops.soap_eigh(plan, gg)
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(lam).all()
    worst = [0.0, 0.0]
    for a, kind, r, qo, ro in zip(mats, kinds, plan.short, plan.q_offsets, plan.r_offsets):
        qk, lk = q[qo:qo + r * r].view(r, r).cpu(), lam[ro:ro + r].cpu()
        l_ref, q_ref = torch.linalg.eigh(a)                                    # fp32 LAPACK on the same input: the yardstick
        l_ref, q_ref = torch.flip(l_ref, [0]), torch.flip(q_ref, [1])
        o_ref, r_ref = _ortho_err(q_ref), _resid(a, q_ref, l_ref)
        o_k, r_k = _ortho_err(qk), _resid(a, qk, lk)
        print(f"[soap] eigh r={r:3d} {kind:9s}: |Q^T Q - I| {o_k:.2e} (lapack {o_ref:.2e}), |A Q - Q L| / |A| {r_k:.2e} (lapack {r_ref:.2e})")
        assert bool((lk[1:] <= lk[:-1]).all()), (r, kind)                      # descending
        assert o_k <= 4 * o_ref, (r, kind, o_k, o_ref)
        assert r_k <= 4 * r_ref, (r, kind, r_k, r_ref)
        if kind == "zero":
            assert torch.equal(qk.abs().sum(0), torch.ones(r)) and torch.equal(qk.abs().sum(1), torch.ones(r))   # a signed permutation
        worst = [max(worst[0], o_k / max(o_ref, 1e-30)) if o_ref else worst[0], max(worst[1], r_k / max(r_ref, 1e-30)) if r_ref else worst[1]]
    print(f"[soap] eigh worst ratio to lapack: orthogonality {worst[0]:.2f}, residual {worst[1]:.2f}")


# ---- the refresh ------------------------------------------------------------------------------------------------------------------------------------
def test_refresh_keeps_the_basis_orthonormal_and_permutes_exp_avg_sq_exactly():
    shapes = [(4, 129), (200, 32), (48, 513), (1100, 128), (32, 200), (129, 48)]

    def run(freq):
        pflat, gflat, ps, gen = _arena(shapes, 2)
        opt = St355Soap(ps, lr=1e-3, max_precond_dim=128, precondition_frequency=freq)
        for call in range(4):                       # the first call, then steps 1 .. 3: step 3 refreshes when freq == 3
            gflat.copy_(torch.randn(pflat.numel(), generator=gen).to(DEV))
            if call == 2:
                gflat[:shapes[0][0] * shapes[0][1]] = 0
            opt.step()
        torch.cuda.synchronize()
        return pflat, opt

    pa, oa = run(3)
    pb, ob = run(1000)
    sa, sb_ = oa._flat[0], ob._flat[0]
    assert torch.equal(pa, pb) and torch.equal(sa["m"], sb_["m"]) and torch.equal(sa["gg"], sb_["gg"])   # the refresh comes after the update
    assert all(torch.isfinite(sa[k]).all() for k in ("m", "v", "gg", "q"))
    for i, (p, q) in enumerate(zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"])):
        r = min(p.shape)
        side = 0 if p.shape[0] < p.shape[1] else 1
        idx = sa["plan"].sort_index(i).long()
        assert sorted(idx.tolist()) == list(range(r))
        want = ob.state[q]["exp_avg_sq"].index_select(side, idx)
        assert torch.equal(oa.state[p]["exp_avg_sq"], want), tuple(p.shape)                             # bit for bit, by the kernel's own index
        Q = oa.state[p]["Q"][side]
        G = oa.state[p]["GG"][side].cpu()
        _, q_ref = torch.linalg.eigh(G)
        o_k, o_ref = _ortho_err(Q), _ortho_err(q_ref)
        print(f"[soap] refresh {tuple(p.shape)}: |Q^T Q - I| {o_k:.2e} (lapack eigh on GG {o_ref:.2e})")
        assert o_k <= 4 * o_ref, (tuple(p.shape), o_k, o_ref)


def test_refresh_of_an_ill_conditioned_preconditioner_reaches_what_lapack_qr_reaches():
    """GG with eigenvalues from 1 down to 1e-6 and a basis rotated away from its eigenvectors: the refresh is Q R = GG Q[:, idx], so Q^T (GG Q[:, idx]) must be
    upper triangular.  Orthogonality and the weight below the diagonal are held to 4 x what torch.linalg.qr reaches in fp32 on the same product (the yardstick
    of the eigensolver test); a column wrongly replaced by the completion would put its whole remainder below the diagonal"""
    gen = torch.Generator().manual_seed(7)
    rs = (4, 32, 48, 128)
    shapes = [(r, 200) for r in rs]
    offs = [sum(a * b for a, b in shapes[:i]) for i in range(len(shapes))]
    plan = ops.SoapPlan(offs, shapes, DEV)
    GGs, Qs = [], []
    for r in rs:
        U, _ = torch.linalg.qr(torch.randn(r, r, generator=gen, dtype=F64))
        lam = torch.logspace(0, -6, r, dtype=F64)
        GGs.append(((U * lam) @ U.T).float())
        Q0, _ = torch.linalg.qr(U + 0.05 * torch.randn(r, r, generator=gen, dtype=F64))
        Qs.append(Q0[:, torch.randperm(r, generator=gen)].float())
    gg = torch.cat([a.reshape(-1) for a in GGs]).to(DEV)
    q = torch.cat([a.reshape(-1) for a in Qs]).to(DEV)
    n = sum(a * b for a, b in shapes)
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    ops.soap_step(plan, p, g, m, v, gg, q, 0.0, 0.95, 0.95, 1e-8, 0.0, 0.0, False, True)      # zero gradient, weight 0: GG stays, the basis is refreshed
    torch.cuda.synchronize()
    assert torch.equal(gg.cpu(), torch.cat([a.reshape(-1) for a in GGs])) and torch.isfinite(q).all()

    def below(Q, M):
        return float(torch.tril(Q.to(F64).T @ M, -1).norm() / M.norm())

    for i, (r, G, Q0) in enumerate(zip(rs, GGs, Qs)):
        idx = plan.sort_index(i).long().cpu()
        est = torch.diag(Q0.to(F64).T @ G.to(F64) @ Q0.to(F64))
        assert sorted(idx.tolist()) == list(range(r)) and bool((est[idx][1:] <= est[idx][:-1] + 1e-5 * est.max()).all())
        M = G.to(F64) @ Q0.to(F64)[:, idx]
        Qk = q[plan.q_offsets[i]:plan.q_offsets[i] + r * r].view(r, r).cpu()
        Ql = torch.linalg.qr(M.float()).Q
        o_k, o_l, b_k, b_l = _ortho_err(Qk), _ortho_err(Ql), below(Qk, M), below(Ql, M)
        print(f"[soap] ill-conditioned refresh r={r:3d}: |Q^T Q - I| {o_k:.2e} (lapack qr {o_l:.2e}), below the diagonal {b_k:.2e} (lapack qr {b_l:.2e})")
        assert o_k <= 4 * o_l, (r, o_k, o_l)
        assert b_k <= 4 * b_l, (r, b_k, b_l)


def test_all_zero_gradients_across_a_refresh_leave_finite_state_and_only_decay_the_parameters():
    shapes = [(4, 129), (513, 48), (128, 200)]
    pflat, gflat, ps, _ = _arena(shapes, 3)
    lr, wd = 1e-2, 0.1
    opt = St355Soap(ps, lr=lr, weight_decay=wd, max_precond_dim=128, precondition_frequency=3)
    want = pflat.clone()
    for call in range(8):
        opt.step()
        if call:
            want = torch.addcmul(want, want, torch.tensor(-SB.f32(lr * wd), device=DEV))               # fma(-lr wd, p, p)
    torch.cuda.synchronize()
    st = opt._flat[0]
    assert all(torch.isfinite(st[k]).all() for k in ("m", "v", "gg", "q")) and torch.isfinite(pflat).all()
    assert not st["m"].any() and not st["v"].any() and not st["gg"].any()
    for p in ps:
        side = 0 if p.shape[0] < p.shape[1] else 1
        assert _ortho_err(opt.state[p]["Q"][side]) == 0.0                    # a permutation: the completion of a zero matrix
    assert (pflat - want).abs().max().item() <= 8 * 2.0 ** -24 * want.abs().max().item()


# ---- the recorded reference ---------------------------------------------------------------------------------------------------------------------------
def _ulp_of_max(t):
    return 2.0 ** (math.floor(math.log2(float(t.abs().max()))) - 23)


def _follow(name, start=0, state_dict=None):
    """drive St355Soap over the recorded gradients of a fixture run; per call the distance to the recorded fp32 reference and its tolerance:
    4 x the reference's own fp32-vs-fp64-decomposition distance at that call, at least 8 fp32 ulps of max |p|"""
    run = GOLD[name]
    shapes = run["shapes"]
    p0 = run["p0"] if start == 0 else run["traj"][start - 1]
    pflat, gflat, ps, _ = _arena(shapes, 0, values=p0)
    opt = St355Soap(ps, **run["settings"])
    if state_dict is not None:
        opt.load_state_dict(copy.deepcopy(state_dict))
    rows = []
    for k in range(start, len(run["grads"])):
        _set_grads(gflat, shapes, run["grads"][k])
        opt.step()
        for i, (p, ref) in enumerate(zip(ps, run["traj"][k])):
            dist = (p.detach().cpu() - ref).abs().max().item()
            tol = max(4.0 * run["dist_f64dec"][k][i], 8 * _ulp_of_max(ref))
            rows.append((k, i, dist, tol))
    return rows, opt, pflat


@pytest.mark.parametrize("name", ["one_sided_f3", "one_sided_f10", "zero_first_grad", "wd0", "nobias", "sb09"])
def test_trajectory_follows_the_recorded_reference(name):
    rows, _, _ = _follow(name)
    worst = max(rows, key=lambda t: t[2] / t[3])
    print(f"[soap] {name}: worst call {worst[0]} matrix {worst[1]}: |p - reference| {worst[2]:.3e}, tolerance {worst[3]:.3e}; "
          + "per call " + " ".join(f"{max(d for k, _, d, _ in rows if k == kk):.1e}" for kk in sorted({k for k, *_ in rows})))
    for k, i, dist, tol in rows:
        assert dist <= tol, (name, k, i, dist, tol)


def test_reference_state_dict_loads_and_the_continuation_stays_within_the_trajectory_tolerance():
    run = GOLD["one_sided_f3"]
    rows, opt, _ = _follow("one_sided_f3", start=run["state_at"] + 1, state_dict=run["state_dict"])
    assert opt._flat[0]["step"] == len(run["grads"]) - 1
    for k, i, dist, tol in rows:
        assert dist <= tol, (k, i, dist, tol)


def test_save_load_continue_is_bit_equal_to_the_uninterrupted_run():
    shapes = [(32, 200), (513, 4), (48, 129)]

    def grads(k):
        return torch.randn(sum(a * b for a, b in shapes), generator=torch.Generator().manual_seed(100 + k)).to(DEV)

    pflat, gflat, ps, _ = _arena(shapes, 4)
    opt = St355Soap(ps, lr=1e-3, max_precond_dim=128, precondition_frequency=3)
    for k in range(5):
        gflat.copy_(grads(k)); opt.step()
    saved, p_mid = copy.deepcopy(opt.state_dict()), pflat.clone()
    for k in range(5, 8):
        gflat.copy_(grads(k)); opt.step()
    off, vals = 0, []
    for s in shapes:
        vals.append(p_mid[off:off + s[0] * s[1]].view(s).cpu()); off += s[0] * s[1]
    pflat2, gflat2, ps2, _ = _arena(shapes, 0, values=vals)
    opt2 = St355Soap(ps2, lr=0.5, max_precond_dim=128, precondition_frequency=7)        # the saved hyper-parameters replace these
    opt2.load_state_dict(saved)
    for k in range(5, 8):
        gflat2.copy_(grads(k)); opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(pflat, pflat2)
    for key in ("m", "v", "gg", "q"):
        assert torch.equal(opt._flat[0][key], opt2._flat[0][key]), key
    assert all(opt2.state[p]["step"] == 7 for p in ps2)


def test_two_runs_are_bit_identical_and_abi_calls_do_not_grow_with_the_matrix_count():
    def run(nmat):
        shapes = [(32, 1100), (513, 32), (48, 200)] * (nmat // 3) + [(129, 128)] * (nmat % 3)
        pflat, gflat, ps, gen = _arena(shapes, 5)
        opt = St355Soap(ps, lr=1e-3, max_precond_dim=128, precondition_frequency=2)
        for _ in range(4):
            gflat.copy_(torch.randn(pflat.numel(), generator=gen).to(DEV))
            opt.step()
        torch.cuda.synchronize()
        st = opt._flat[0]
        return pflat.clone(), st["m"].clone(), st["v"].clone(), st["gg"].clone(), st["q"].clone(), opt.abi_calls, st["plan"].launches(refresh=True)

    a, b = run(3), run(3)
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    c = run(40)
    assert a[5] == c[5] == 4                                 # one ABI call per group and step, with 3 and with 40 matrices
    assert a[6] == 2 + 1 + 1 + 2 and c[6] == 3 + 1 + 1 + 3    # launches depend on the short-side classes present, not on the matrix count


# ---- through the trainer ------------------------------------------------------------------------------------------------------------------------------
def test_flux_lora_train_step_with_soap():
    from simpletuner_amd.flux.model import Flux
    from simpletuner_amd.training.trainer import St355Accelerator, Trainer, default_config
    from tests import parity_utils as PU

    cfg = default_config(lora_rank=16, seed=5, lora_init_b_std=0.02, learning_rate=1e-3, optimizer="soap", optimizer_config="max_precond_dim=128")
    acc = St355Accelerator(DEV)
    plugin = Flux(cfg, acc)
    plugin.load_model(**PU.small_flux_cfg(layers=1, single=1))
    plugin.add_lora_adapter()
    trainer = Trainer(cfg, plugin, acc)
    assert isinstance(trainer.optimizer, St355Soap)
    _, devt = PU.make_inputs(1, 16, 16, 64, 128, 64, DEV, seed=5)
    sig = devt["sigmas"]
    plugin.sample_flow_sigmas = lambda batch, state: (sig, sig * 1000.0)
    batch = {"latent_batch": devt["latents"], "prompt_embeds": devt["prompt"], "add_text_embeds": devt["pooled"], "noise": devt["noise"]}
    flat = plugin.get_trained_component().lora_flat
    snaps = [flat.clone()]
    for _ in range(3):
        loss = trainer.train_step(dict(batch))
        assert math.isfinite(float(loss))
        snaps.append(flat.clone())
    assert torch.equal(snaps[0], snaps[1])                    # the first call only builds the preconditioner
    assert not torch.equal(snaps[1], snaps[2]) and not torch.equal(snaps[2], snaps[3])      # the adapters change from step 2 on
    assert torch.isfinite(flat).all() and trainer.optimizer.abi_calls == 3

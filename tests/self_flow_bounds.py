"""Element-wise error bounds for the Self-Flow kernels (simpletuner_amd/csrc/self_flow.hip) against the fp64 restatement (tests/self_flow_ref.py) — derived, not
fitted, in the manner of tests/nextlat_bounds.py.  u = 2^-24 (fp32 unit roundoff); one round-to-nearest-even to bf16 costs half a bf16 ulp:
`_rounded(ref, e)` = 1/2 ulp_bf16(|ref| + e) + e for a stored bf16 value whose fp32 pre-image is within e of ref.  An fp32 sum of K terms, in any fixed order, is
off by at most K u sum|terms| (recursive summation; products of two bf16 values are exact in fp32, + 8 absorbs the adds of fixed-order partials).

Stored intermediates are chained: xhat, proj, G, g and P each cost their one bf16 rounding where they are stored, and every stage is bounded against the fp64 value
of ITS OWN stored operands, so a one-ulp tie in an intermediate cannot leak into the next stage.  The cosine pass (st355_layersync_fwd) is held to
tests/layersync_bounds.py, the LayerNorm backward (st355_nextlat_ln_bwd_add) to tests/nextlat_bounds.ln_bwd_add_bounds.  The unchained end-to-end agreement with the
executed reference is the fixture's and the engine tests' business.

views.  out = fma(s, n, fl(fl(1 - s) x)) with s, x, n exact inputs (s an fp32 the kernel selects, never computes): fl(1 - s) carries u (1 - s), the product one more u,
the fma one: the fp32 pre-image is within e = 3 u |(1 - s) x| + u |s n| of (1 - s) x + s n (4 u (|(1 - s) x| + |s n|) is used).  A bf16 output is `_rounded(ref, e)`, an
fp32 output ref within e (the fma's own rounding is the last u).  The token timesteps, the teacher's sigma and timestep and the sigma grid are SELECTIONS of input
values (a < compare in fp32, fminf): exact, tolerance 0.

fold.  Wf = bf16(fl(gamma W)): e = u |gamma W|.  c = bf16(fl(sum_d W beta) + b): a D-term fmaf chain in lane-strided partials and a butterfly:
e = (D + 8) u (sum_d |W beta| + |b|).  WfT holds the same values transposed.

rows.  tests/internal_guidance_bounds.fwd_bounds' derivation with nn.LayerNorm's eps 1e-5 in s = sqrt(var + eps): per row with A = max_j |x_j|,
e_mean = (D + 2) u A, e_d = e_mean + u |d|, delta_v = 2 e_mean / s + (e_mean / s)^2 + (D + 8) u (refused beyond 1/4), delta_r = 0.77 delta_v + 8 u,
    |xhat - xhat64| <= 1/2 ulp_bf16 + (e_d / s + |xhat64| (delta_r + 2 u)),      |rstd - rstd64| <= delta_r / s.

gemm steps (proj = xhat Wf^T + c, g = G Wf, P = G^T xhat), from the stored operands: e = (K + 8) u (|A| |B|^T + |bias|), tol = `_rounded(ref, e)`.

wgrad, from the stored P (bf16) and db (fp32), N = D rows:
    dW     = s fma(P, gamma, fl(db beta)):              e = 4 u |s| (|P gamma| + |db beta|)
    db     = s db:                                      e = u |s db|
    dgamma = s sum_n W P (32-row chains, 32 row lanes, ceil(D / 256) chunks: D + 8 terms at most):    e = (D + 10) u |s| sum_n |W P|
    dbeta  = s sum_n W db:                              e = (D + 10) u |s| sum_n |W db|
accumulate adds one fp32 addition to what is there: + u |previous + ref|.
"""
import torch

from tests import self_flow_ref as SF
from tests.gemm_bounds import ulp_bf16

F64 = torch.float64
U = 2.0 ** -24


def _rounded(ref, e):
    """one RNE to bf16 of an fp32 value within e of ref"""
    return 0.5 * ulp_bf16(ref.abs() + e) + e


def views_bounds(latents, noise, sigma, sigma_alt, t, t_alt, uniforms, ratio: float, p: int):
    """the exact input values -> {name: (ref64, tol)}; bf16 inputs give bf16 views (one rounding), fp32 inputs fp32 views"""
    v = SF.views64(latents, noise, sigma, sigma_alt, t, t_alt, uniforms, ratio, p)
    lat, n = latents.to(F64), noise.to(F64)
    out = {}
    for name, s in (("noisy_student", v["sigma_grid"]), ("noisy_teacher", v["sigma_teacher"].view(-1, 1, 1, 1))):
        e = 4 * U * (((1 - s) * lat).abs() + (s * n).abs())
        out[name] = (v[name], _rounded(v[name], e) if latents.dtype == torch.bfloat16 else e)
    for name in ("token_timesteps", "sigma_teacher", "timestep_teacher", "sigma_grid"):
        out[name] = (v[name], torch.zeros_like(v[name]))
    return out


def fold_bounds(gamma, beta, W, b):
    """-> {name: (ref64, tol)} for Wf and c"""
    ga, be, Wd, bd = (t.to(F64) for t in (gamma, beta, W, b))
    D = Wd.shape[1]
    Wf, c = Wd * ga[None, :], Wd @ be + bd
    e_c = (D + 8) * U * ((Wd * be[None, :]).abs().sum(dim=1) + bd.abs())
    return {"Wf": (Wf, _rounded(Wf, U * Wf.abs())), "c": (c, _rounded(c, e_c))}


def rows_bounds(h):
    """h [M, D] (the exact bf16 input values) -> (xhat64, tol_xhat [M, D], rstd64, tol_rstd [M])"""
    x = h.to(F64)
    D = x.shape[1]
    mean = x.mean(dim=1, keepdim=True)
    d = x - mean
    s = torch.sqrt((d * d).mean(dim=1, keepdim=True) + SF.EPS)
    xhat = d / s
    e_mean = (D + 2) * U * x.abs().amax(dim=1, keepdim=True)
    delta_v = 2 * e_mean / s + (e_mean / s) ** 2 + (D + 8) * U
    assert float(delta_v.max()) <= 0.25, "rows_bounds: a row outside the regime of the derivation (delta_v > 1/4)"
    delta_r = 0.77 * delta_v + 8 * U
    e_x = (e_mean + U * d.abs()) / s + xhat.abs() * (delta_r + 2 * U)
    return xhat, _rounded(xhat, e_x), (1.0 / s)[:, 0], (delta_r / s)[:, 0]


def gemm_bounds(A, Bm, bias=None):
    """the stored operands A [M, K], Bm [N, K] (out = A Bm^T + bias) -> (ref64, tol) of the bf16 output"""
    a, b = A.to(F64), Bm.to(F64)
    K = a.shape[1]
    ref, mag = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        ref, mag = ref + bias.to(F64)[None, :], mag + bias.to(F64).abs()[None, :]
    return ref, _rounded(ref, (K + 8) * U * mag)


def wgrad_bounds(P, db, gamma, beta, W, scale: float, prev=None):
    """-> {name: (ref64, tol)} for g_gamma, g_beta, g_W, g_b; prev: {name: what the gradients held} under accumulate"""
    Pd, d, ga, be, Wd = P.to(F64), db.to(F64).reshape(-1), gamma.to(F64), beta.to(F64), W.to(F64)
    D = Wd.shape[0]
    s, a = float(scale), abs(float(scale))
    out = {
        "g_W": (s * (Pd * ga[None, :] + d[:, None] * be[None, :]), 4 * U * a * ((Pd * ga[None, :]).abs() + (d[:, None] * be[None, :]).abs())),
        "g_b": (s * d, U * a * d.abs()),
        "g_gamma": (s * (Wd * Pd).sum(dim=0), (D + 10) * U * a * (Wd * Pd).abs().sum(dim=0)),
        "g_beta": (s * (Wd * d[:, None]).sum(dim=0), (D + 10) * U * a * (Wd * d[:, None]).abs().sum(dim=0)),
    }
    if prev is not None:
        out = {k: (prev[k].to(F64) + ref, e + U * (prev[k].to(F64) + ref).abs() + U * ref.abs()) for k, (ref, e) in out.items()}
    return out


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the elements (0 / 0 counts as 0: an exact value with tolerance 0), and whether every element is inside"""
    err = (got.to(F64) - ref).abs()
    ok = bool((err <= tol).all())
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()), ok


# ---- the cases the stand-ins (CPU) and the kernels (GPU) are both held to ----
GUARD = 64                      # elements in front of and behind every operand carved from a guard buffer (>= 128 bytes: the operands stay 16-byte aligned)
SENTINEL = 12345.0
VIEW_SHAPES = ((1, 16, 2, 2), (3, 16, 6, 10))          # a single token; rows of 10 elements (no multiple of the 8- / 4-element vector), 15 tokens per sample
VIEW_RATIOS = (0.0, 0.25, 0.5)
HEAD_CASES = ((128, 3, 10, False), (128, 1, 64, False), (1536, 3, 10, True), (1536, 2, 32, True))          # (D, B, S, strided teacher): M = 30 (no multiple of 4 / 16 / 64) and 64


def _guarded(shape, dtype, device, fill=None, stride0=None):
    """-> (whole, view): a 1-D buffer of sentinels with `view` (contiguous, or with batch stride stride0) carved out GUARD elements in"""
    n0 = shape[0]
    per = 1
    for d in shape[1:]:
        per *= d
    s0 = per if stride0 is None else stride0
    whole = torch.full((GUARD + n0 * s0 + GUARD,), SENTINEL, dtype=dtype)
    view = torch.as_strided(whole, shape, (s0, *torch.empty(shape[1:]).stride()) if len(shape) > 1 else (1,), GUARD)
    if fill is not None:
        view.copy_(fill.to(dtype))
    whole = whole.to(device)
    view = torch.as_strided(whole, shape, (s0, *torch.empty(shape[1:]).stride()) if len(shape) > 1 else (1,), GUARD)
    return whole, view


def _outside_intact(whole, shape, stride0=None):
    """every element of the guard buffer outside the carved view still holds the sentinel"""
    w = whole.detach().cpu().float().clone()
    sent = float(torch.tensor(SENTINEL).to(whole.dtype))          # (as the buffer's dtype holds it)
    per = 1
    for d in shape[1:]:
        per *= d
    s0 = per if stride0 is None else stride0
    for b in range(shape[0]):
        w[GUARD + b * s0:GUARD + b * s0 + per] = sent
    return bool((w == sent).all())


def check_views_case(ops, dev, shape, ratio: float, dtype, strided: bool, seed: int = 0):
    """one call of ops.self_flow_views (p = 2) on seeded inputs inside guard buffers: every output inside its bound, a second call bit-identical, inputs and guards
    untouched.  Returns {name: worst ratio to the bound}."""
    B, C, H, W = shape
    p, per = 2, C * H * W
    g = torch.Generator().manual_seed(500 + seed)
    lat, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    sig = torch.tensor([0.30, 0.70, 0.55][:B])
    alt = torch.tensor([0.65, 0.20, 0.55][:B])                     # above, below, equal
    u = torch.rand(B, H // p, W // p, generator=g)
    if B > 1 and 0.0 < ratio:
        assert 0 < int((u < ratio).sum()) < u.numel()
    s0 = per + 24 if strided else None
    w_lat, v_lat = _guarded(shape, dtype, dev, lat, s0)
    w_noise, v_noise = _guarded(shape, dtype, dev, noise, s0)
    outs, wholes = [], []
    for shp, dt in ((shape, dtype), (shape, dtype), ((B, (H // p) * (W // p)), torch.float32), ((B,), torch.float32), ((B,), torch.float32)):
        w_, v_ = _guarded(shp, dt, dev)
        wholes.append((w_, shp)); outs.append(v_)
    before = (w_lat.clone(), w_noise.clone())
    args = (v_lat, v_noise, sig.to(dev), alt.to(dev), (sig * 1000.0).to(dev), (alt * 1000.0).to(dev), u.to(dev), ratio, p)
    res = ops.self_flow_views(*args, out=tuple(outs))
    first = [t.detach().cpu().clone() for t in res[:5]]
    fresh = ops.self_flow_views(*args, want_sigma_grid=True)          # a second launch, outputs allocated by the wrapper, the sigma grid written
    names = ("noisy_student", "noisy_teacher", "token_timesteps", "sigma_teacher", "timestep_teacher")
    bounds = views_bounds(v_lat.detach().cpu(), v_noise.detach().cpu(), sig, alt, sig * 1000.0, alt * 1000.0, u, ratio, p)
    worst = {}
    for nm, a, b2 in zip(names, first, fresh[:5]):
        assert a.dtype == b2.dtype and torch.equal(a, b2.detach().cpu()), f"{nm}: two launches differ"
        ref, tol = bounds[nm]
        worst[nm], ok = worst_ratio(a, ref.reshape(a.shape), tol.reshape(a.shape))
        assert ok, f"{nm}: outside the bound, worst ratio {worst[nm]:.3f} ({shape}, ratio {ratio}, {dtype})"
    ref, tol = bounds["sigma_grid"]
    worst["sigma_grid"], ok = worst_ratio(fresh[5].detach().cpu(), ref.reshape(fresh[5].shape), tol.reshape(fresh[5].shape))
    assert ok, "sigma_grid"
    assert torch.equal(before[0], w_lat) and torch.equal(before[1], w_noise), "an input buffer was written"
    for (w_, shp) in wholes:
        assert _outside_intact(w_, shp), "guard bytes around an output were written"
    return worst


def head_inputs(D: int, B: int, S: int, strided: bool, dev, seed: int = 0):
    """seeded projector parameters (fp32), a [B, S, D] bf16 block-output view inside a joint [B, S + 7, D] buffer, teacher features (compact, or a [B, S, D] view of
    a [B, S + 5, D] buffer: one row stride, another batch stride), dx to add into (a view like h)"""
    g = torch.Generator().manual_seed(900 + seed)
    params = (1.0 + 0.25 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), torch.randn(D, D, generator=g) / D ** 0.5, 0.05 * torch.randn(D, generator=g))
    joint = (torch.randn(B, S + 7, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(dev)
    tbuf = torch.randn(B, S + 5 if strided else S, D, generator=g).to(torch.bfloat16).to(dev)
    dxj = (0.01 * torch.randn(B, S + 7, D, generator=g)).to(torch.bfloat16).to(dev)
    return tuple(q.to(dev) for q in params), joint, joint[:, 3:3 + S], tbuf[:, 2:2 + S] if strided else tbuf, dxj, dxj[:, 3:3 + S]


def check_head_case(ops, dev, D: int, B: int, S: int, strided: bool, dsim: float = -0.37, seed: int = 0):
    """the fold, the row pass, the projection, the cosine and the whole backward of the alignment path on one case, every stage held to its bound on its own stored
    operands; the chain is run twice and compared bit for bit.  Returns {stage: worst ratio to the bound}."""
    from simpletuner_amd.engine import pad64, pad64_empty
    from tests import layersync_bounds as LB
    from tests import layersync_ref as LS
    from tests import nextlat_bounds as NB
    BF16, F32 = torch.bfloat16, torch.float32
    M = B * S
    dsim = float(torch.tensor(dsim, dtype=F32))          # the scalar as the kernels read it: one fp32 on the device

    def run():
        params, joint, h, teacher, dxj, dx = head_inputs(D, B, S, strided, dev, seed)
        ga, be, W, b = params
        Wf, WfT, c = (torch.empty(D, D, dtype=BF16, device=dev), torch.empty(D, D, dtype=BF16, device=dev), torch.empty(D, dtype=BF16, device=dev))
        ops.self_flow_fold(ga, be, W, b, Wf, WfT, c)
        xhat, rstd = pad64_empty(M, D, dev), torch.empty(M, dtype=F32, device=dev)
        ops.self_flow_rows(h, xhat, rstd)
        G = pad64_empty(M, D, dev)
        ops.gemm(xhat, Wf, bias=c, out=G)
        proj = G.detach().clone()
        cos, sim = torch.empty(M, dtype=F32, device=dev), torch.empty((), dtype=F32, device=dev)
        ops.layersync_fwd(G.view(B, S, D), teacher, G, cos, sim)
        s = torch.tensor([dsim], dtype=F32, device=dev)
        db = torch.empty(1, D, dtype=F32, device=dev)
        ops.colsum_prod(G, db)
        P = ops.gemm_tn(pad64(G), pad64(xhat))
        grads = tuple(torch.full(q.shape, 0.5, dtype=F32, device=dev) for q in params)
        ops.self_flow_wgrad(P, db.view(D), ga, be, W, s, *grads, accumulate=False)
        acc = tuple(torch.full(q.shape, 0.5, dtype=F32, device=dev) for q in params)
        ops.self_flow_wgrad(P, db.view(D), ga, be, W, s, *acc, accumulate=True)
        gg = torch.empty(M, D, dtype=BF16, device=dev)
        ops.gemm(G, WfT, out=gg)
        dx_in = dx.detach().clone()
        joint_before, dxj_before = joint.detach().clone(), dxj.detach().clone()
        ops.nextlat_ln_bwd_add(gg, xhat, rstd, s, dx)
        assert torch.equal(joint_before, joint), "the block output was written"
        outside = torch.ones(dxj.shape[:2], dtype=torch.bool)
        outside[:, 3:3 + S] = False
        assert torch.equal(dxj_before.cpu()[outside], dxj.cpu()[outside]), "rows outside the dx view were written"
        cpu = lambda t: t.detach().cpu().clone()
        return dict(params=tuple(cpu(q) for q in params), h=cpu(h), teacher=cpu(teacher), Wf=cpu(Wf), WfT=cpu(WfT), c=cpu(c), xhat=cpu(xhat), rstd=cpu(rstd), proj=cpu(proj),
                    G=cpu(G), cos=cpu(cos), sim=cpu(sim), db=cpu(db.view(D)), P=cpu(P), grads=tuple(cpu(q) for q in grads), acc=tuple(cpu(q) for q in acc), g=cpu(gg),
                    dx_in=cpu(dx_in), dx=cpu(dx))

    r, r2 = run(), run()
    for k in r:
        a, b_ = (r[k], r2[k]) if not isinstance(r[k], tuple) else (torch.cat([q.reshape(-1) for q in r[k]]), torch.cat([q.reshape(-1) for q in r2[k]]))
        assert torch.equal(a, b_), f"{k}: two runs differ"
    ga, be, W, b = r["params"]
    worst = {}

    def hold(name, got, ref, tol):
        worst[name], ok = worst_ratio(got, ref.reshape(got.shape), tol.reshape(got.shape) if torch.is_tensor(tol) else torch.full(got.shape, float(tol), dtype=F64))
        assert ok, f"{name}: outside the bound, worst ratio {worst[name]:.3f} (D {D}, M {M})"

    fb = fold_bounds(ga, be, W, b)
    hold("Wf", r["Wf"], *fb["Wf"]); hold("c", r["c"], *fb["c"])
    assert torch.equal(r["WfT"], r["Wf"].t()), "WfT is not Wf transposed"
    xh, tx, rs, tr = rows_bounds(r["h"].reshape(M, D))
    hold("xhat", r["xhat"], xh, tx); hold("rstd", r["rstd"], rs, tr)
    hold("proj", r["proj"], *gemm_bounds(r["xhat"], r["Wf"], r["c"]))
    c64, sim64, G64, sn = LS.reference64(r["proj"].view(B, S, D), r["teacher"])
    hold("cos", r["cos"], c64, LB.cos_bound(D)); hold("sim", r["sim"].reshape(1), sim64.reshape(1), LB.sim_bound(D, M))
    hold("G", r["G"], G64, LB.grad_bound(G64, sn, D))
    Gd = r["G"].to(F64)
    hold("db", r["db"], Gd.sum(dim=0), (M + 8) * U * Gd.abs().sum(dim=0))
    hold("P", r["P"], *gemm_bounds(r["G"].t(), r["xhat"].t()))
    wb = wgrad_bounds(r["P"], r["db"], ga, be, W, dsim)
    wa = wgrad_bounds(r["P"], r["db"], ga, be, W, dsim, prev={k: torch.full(v[0].shape, 0.5, dtype=F64) for k, v in wb.items()})
    for i, k in enumerate(("g_gamma", "g_beta", "g_W", "g_b")):
        hold(k, r["grads"][i], *wb[k]); hold(k + "+", r["acc"][i], *wa[k])
    hold("g", r["g"], *gemm_bounds(r["G"], r["WfT"]))
    hold("dx", r["dx"].reshape(M, D), *NB.ln_bwd_add_bounds(r["g"], r["xhat"], r["rstd"], dsim, r["dx_in"].reshape(M, D)))
    return worst, r


# the flag-off launch-trace selection of tests/test_self_flow_cpu.py (tools/launch_trace.py -k): the SD3 tokenwise step and the LoRA steps with a tap and a head
TRACE_SELECTION = "(test_sd3_host_sequencing_cpu and tokenwise_timesteps_through_the_emulator) or (test_sd3_engine_with_nextlat_matches_autograd_through_the_oracle and lora and plain)"

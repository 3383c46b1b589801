"""Element-wise error bounds of the Flow-DPO kernels (csrc/flow_dpo.hip) against fp64 on the SAME bf16 / fp32 operands — TEST INFRASTRUCTURE ONLY.

Every bound is derived from the kernels' arithmetic, never from what they return.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16), gamma(n) = n u / (1 - n u): the
relative error of an fp32 sum of n terms in ANY order.  A bf16 number is an fp32 number; a sum or difference of two of them is ONE fp32 rounding (their exponents
may lie more than 16 apart).  The fp32 division is correctly rounded; expf and log1pf are taken as accurate to 2 ulp (MATH = 2: ROCm's device library documents 1).
The counts hold with or without fused multiply-adds (a fused pair rounds once instead of twice); SLACK = 1 + 2^-10 covers the second-order terms.  The scalar
parameters are compared as the fp32 numbers the kernels receive (flow_dpo_ref.f32).

st355_flow_dpo_stats   each of the N terms takes part in at most DEPTH = 8 runs + 6 + 4 + parts additions — the lane's strided run of `runs` 8-element vectors, 6
    butterfly steps, 4 wave partials in wave order, the `parts` stage-2 partials in index order (stats_depth restates the kernel's grid rule) — and the error of a
    summation tree is bounded by gamma(depth) sum |term| whatever its shape:
    errors      m (x - t)^2:  x - t: u, the square: 2 u + u, the mask: u  ->  4 u |term|
    anchor      (p - r)^2:  3 u |term|
    mask sum    exact terms
    advantage   m d q,  d = r - p (u |d|),  s = r + p (u |s|),  q = s - 2 t (2 t exact; the difference: u |q|, and it carries s's error u |s| ABSOLUTELY: this is the
                cancellation the form has, where p + r ~ 2 t, and it is counted, not assumed away):
                |term - term64| <= |m| [ |d| u |s| + 4 u |d q| ]
    |S_k - S_k64| <= sum e_term + gamma(DEPTH) sum |term|

st355_flow_dpo_head    against fp64 ON THE GIVEN fp32 STATS.  nu: 1 / n or 1 / max(S_m, 1): 2 u.  margin = nu (a + b): 4 u |nu| (|a| + |b|) =: e_m  (the sum a + b is one
    rounding of |a + b| <= |a| + |b|).  absmean: (sum e_m + gamma(B + 1) sum |margin|) / B.  ema = decay ema + (1 - decay) absmean: 4 u (|decay ema| + |(1 - decay)
    absmean|) + (1 - decay) e_absmean.  beta = clamp(num / max(ema, eps)): the clamps are 1-Lipschitz; relative e_ema / max(ema, eps) + 2 u.
    logit = beta margin / 2: |logit| (rel_beta + 2 u) + |beta| e_m / 2 =: e_x.   E = exp(-|x|): relative e_x + (MATH + 1) u.   log sigma = min(x, 0) - log1p(E):
    e_x + E rel_E + MATH u log1p(E) + u |log sigma|.   sigma(-x) = {E, 1} / (1 + E): relative rel_E + 3 u.   c = lw beta sigma(-x) / (2 B): relative rel_beta + rel_sig + 5 u.
    The means over B pairs run in pair order: gamma(B + 1).  The anchor (all terms >= 0): gamma(B + 12) relative.
    negative_margin_pct is exact when every |margin_b| > e_m (check_margins: the input condition, zero undecided samples).

st355_flow_dpo_grad    against fp64 ON THE GIVEN fp32 pair coefficients.  k = +-2 c nu s (s = grad_scale [* upstream]: u): 4 u.  a = alpha / (B n) s: 5 u.
    k (m (p - t)): 3 u more;  a (p - r): 2 u more;  the sum: u.   e32 = 8 u (|k m (p - t)| + |a (p - r)|);  then ONE bf16 rounding:  tol = e32 + ub (|g64| + e32)
"""
import torch

from tests import flow_dpo_ref as FR
from tests import reflexflow_ref as RR

F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 1e-38
SLACK = 1.0 + 2.0 ** -10
MATH = 2.0


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def stats_depth(B: int, N: int) -> int:
    """the most additions any term takes part in: csrc/flow_dpo.hip's grid rule (sample_parts of feature_common.h: 256 lanes of 8 elements per partial workgroup, at most 2048 / B of them
    per pair), restated"""
    vecs = N // 8
    parts = max(1, min(-(-vecs // 256), 2048 // B))
    runs = -(-vecs // (256 * parts))
    return 8 * runs + 6 + 4 + parts


def stats_ref(policy, ref, tw, tl, emask=None, depth=None):
    """(reference [B, 9], bound [B, 9]); depth: the summation tree's depth, the kernel's by default"""
    B = tw.shape[0]
    p, r, t1, t2 = FR._flat(policy, 2 * B), FR._flat(ref, 2 * B), FR._flat(tw, B), FR._flat(tl, B)
    N = t1.shape[1]
    m = RR._mask_full(None if emask is None else emask.cpu(), B, N)
    m = torch.ones_like(t1) if m is None else m
    pw, pl, rw, rl = p[:B], p[B:], r[:B], r[B:]
    out = FR.stats64(policy, ref, tw, tl, emask)
    g = gamma(stats_depth(B, N) if depth is None else depth)
    bounds = []
    for x, t in ((pw, t1), (pl, t2), (rw, t1), (rl, t2)):
        mag = (m * (x - t) ** 2).sum(1)
        bounds.append((4 * U + g) * mag)
    for a, b in ((pw, rw), (pl, rl)):
        mag = ((a - b) ** 2).sum(1)
        bounds.append((3 * U + g) * mag)
    bounds.append(g * m.sum(1))
    for d, s, t in ((rw - pw, rw + pw, t1), (pl - rl, pl + rl, t2)):
        q = s - 2 * t
        bounds.append((m.abs() * (d.abs() * U * s.abs() + 4 * U * (d * q).abs())).sum(1) + g * (m * d * q).abs().sum(1))
    return out, SLACK * torch.stack(bounds, dim=1) + TINY


def head_ref(stats, n, norm_type="sum", has_mask=False, beta=1.0, loss_weight=1.0, anchor_alpha=0.0, ema_state=None, auto_num=0.0, decay=0.99, beta_min=None,
             beta_max=None, eps=1e-6, original_loss=None, sft_weight=0.0, absmean=None):
    """fp64 on the given fp32 stats and the fp32 values of the scalars: {name: (reference, bound)} for loss, pair (margin, logit, c, nu columns), logs, ema"""
    f = FR.f32
    kw = dict(norm_type=norm_type, has_mask=has_mask, beta=f(beta), loss_weight=f(loss_weight), anchor_alpha=f(anchor_alpha), auto_num_=f(auto_num), decay=f(decay),
              beta_min=None if beta_min is None else f(beta_min), beta_max=None if beta_max is None else f(beta_max), eps=f(eps),
              original_loss=None if original_loss is None else float(original_loss), sft_weight=f(sft_weight))
    r = FR.head64(stats, n, ema_state=ema_state, absmean=absmean, **kw)
    st = stats.detach().to(F64).cpu()
    B = st.shape[0]
    margin, logit, c, nu = r["pair"].unbind(1)
    e_m = 4 * U * nu.abs() * (st[:, 7].abs() + st[:, 8].abs())
    gB = gamma(B + 1)
    e_abs = (e_m.sum() + gB * margin.abs().sum()) / B + U * r["absmean"].abs() if absmean is None else torch.zeros((), dtype=F64)
    bt = float(r["beta"])
    rel_beta, e_ema = 0.0, torch.zeros((), dtype=F64)
    if ema_state is not None:
        d, am = kw["decay"], float(r["absmean"])
        prev = float(ema_state[0]) if float(ema_state[1]) != 0.0 else 0.0
        e_ema = (4 * U * (abs(d * prev) + abs((1 - d) * am)) + (1 - d) * e_abs) if float(ema_state[1]) != 0.0 else e_abs
        rel_beta = float(e_ema) / max(r["ema_state"][0], kw["eps"]) + 2 * U
    e_x = logit.abs() * (rel_beta + 2 * U) + abs(bt) * e_m / 2
    E = torch.exp(-logit.abs())
    rel_E = e_x + (MATH + 1) * U
    ls, sn = FR.logsig64(logit)
    e_ls = e_x + E * rel_E + MATH * U * torch.log1p(E) + U * ls.abs()
    rel_sn = rel_E + 3 * U
    e_sn = sn * rel_sn
    e_c = c.abs() * (rel_beta + rel_sn + 5 * U)
    e_dpo = e_ls.sum() / B + gB * ls.abs().sum() / B
    anchor = r["logs"][12]
    e_anchor = gamma(B + 12) * anchor.abs()
    lw = abs(kw["loss_weight"])
    dpo = r["logs"][0]
    e_loss = e_dpo * lw + e_anchor + 2 * U * ((dpo * lw).abs() + anchor.abs())

    def mean_of(k):          # mean_b nu_b stats[b, k]: nu 2 u, the product u, the sum in pair order, the division
        return (3 * U + gB + U) * (nu * st[:, k]).abs().sum() / B

    orig = abs(float(original_loss)) if original_loss is not None else 0.0
    e_logs = torch.stack([e_dpo, torch.tensor(abs(bt) * rel_beta + U * abs(bt), dtype=F64), e_m.sum() / B + gB * margin.abs().sum() / B, mean_of(7), mean_of(8),
                          mean_of(0), mean_of(1), mean_of(2), mean_of(3), torch.zeros((), dtype=F64), e_sn.sum() / B + gB * sn.sum() / B,
                          e_loss + 3 * U * abs(kw["sft_weight"]) * orig + U * r["logs"][11].abs(), e_anchor, e_abs, e_ema, torch.zeros((), dtype=F64)])
    e_pair = torch.stack([e_m, e_x + U * logit.abs(), e_c, 2 * U * nu.abs()], dim=1)
    return {"loss": (r["loss"], SLACK * e_loss + TINY), "pair": (r["pair"], SLACK * e_pair + TINY), "logs": (r["logs"], SLACK * e_logs + TINY),
            "ema": (None if r["ema_state"] is None else torch.tensor(r["ema_state"][0], dtype=F64), SLACK * e_ema + TINY), "margin_bound": SLACK * e_m + TINY}


def grad_ref(policy, ref, tw, tl, pair, emask=None, anchor_alpha=0.0, grad_scale=1.0):
    """(reference [2B, N], bound [2B, N]); grad_scale: the product of the host scale and the upstream device scalar, as one number"""
    B = tw.shape[0]
    a_ = FR.f32(anchor_alpha)
    g = FR.grad64(policy, ref, tw, tl, pair, emask, a_, grad_scale)
    main = FR.grad64(policy, ref, tw, tl, pair, emask, 0.0, grad_scale)
    e32 = SLACK * 8 * U * (main.abs() + (g - main).abs())
    return g, e32 + UB * (g.abs() + e32) + TINY


def margin_forms(policy, ref, tw, tl, emask=None):
    """fp32 arithmetic on the CPU, both ways, per pair and unnormalised (norm_type sum): (the margin from the element-wise advantages, the margin as the
    difference of the four fp32 sums) — why the kernel is shaped as it is.  Every sum is an explicit pairwise tree of depth log2(N) (N a power of two), one fp32
    addition per level, so that the depth the bound counts is the depth that ran"""
    F32 = torch.float32
    B = tw.shape[0]
    f = lambda t, rows: t.detach().to(F32).cpu().reshape(rows, -1)
    p, r, t1, t2 = f(policy, 2 * B), f(ref, 2 * B), f(tw, B), f(tl, B)
    m = RR._mask_full(None if emask is None else emask.cpu(), B, t1.shape[1], dtype=F32)
    m = torch.ones_like(t1) if m is None else m
    pw, pl, rw, rl = p[:B], p[B:], r[:B], r[B:]
    def tree(x):
        assert x.shape[1] & (x.shape[1] - 1) == 0
        while x.shape[1] > 1:
            x = x[:, 0::2] + x[:, 1::2]
        return x[:, 0]

    adv = tree(m * ((rw - pw) * ((rw + pw) - 2 * t1))) + tree(m * ((pl - rl) * ((pl + rl) - 2 * t2)))
    E = lambda x, t: tree(m * (x - t) ** 2)
    four = (E(rw, t1) - E(pw, t1)) + (E(pl, t2) - E(rl, t2))
    return adv, four


def check_margins(stats, n, norm_type="sum", has_mask=False):
    """the input condition: every |margin_b| lies above its bound (zero undecided samples for negative_margin_pct).  Returns (ok, min |margin| / bound)"""
    r = head_ref(stats, n, norm_type=norm_type, has_mask=has_mask)
    ratio = r["pair"][0][:, 0].abs() / r["margin_bound"]
    return bool((ratio > 1.0).all()), float(ratio.min())


def inside(got, ref, tol):
    """(ok, worst |got - ref| / tol)"""
    err = (got.detach().to(F64).cpu().reshape(ref.shape) - ref).abs()
    return bool((err <= tol).all()), float((err / tol).max())

"""Element-wise error bounds for the Self-Transcendence kernels (simpletuner_amd/csrc/self_transcendence.hip) against the fp64 restatement
(tests/self_transcendence_ref.py) — derived, not fitted, in the manner of tests/nextlat_bounds.py — and the cases both the CPU stand-ins and the GPU kernels are
held to.  u = 2^-24 (fp32 unit roundoff); one round-to-nearest-even to bf16 costs half a bf16 ulp: `_rounded(ref, e)` = 1/2 ulp_bf16(|ref| + e) + e for a stored
bf16 value whose fp32 pre-image is within e of ref.  Every kernel is bounded against the fp64 value of ITS OWN stored operands.

fold.  bf16(W), bf16(b) of fp32 masters: e = 0, one rounding.  The transposes hold the same values.  Rows >= P3 of W3h and elements >= P3 of b3h keep their bytes.

target.  vae: the stored value, read as it is: e_t = 0.  cfg: t = fma(s32, fl(c - u), u) with s32 = fl(cfg_scale): the scale's own rounding u |s| |c - u|, the
difference's u |c - u| carried through the factor, the fma's u |t|:   e_t = 2 u |s| |c - u| + u |t|.
d = fl(pred - t): e_d = e_t + u |d|.   G = bf16(2 d) of an active sample (2 d is exact): tol = _rounded(2 d, 2 e_d); of an inactive one exactly 0.

per-sample mean.  A lane's fmaf chain runs over at most 8 ceil(n8 / (nch 256)) squares (n8 = S P / 8 chunks, nch = min(ceil(n8 / 256), 256) workgroups per
sample), then 6 butterfly steps, 2 wave adds, the nch partials in order and the scale by fl(1 / (S P)):  L = 8 ceil(n8 / (nch 256)) + nch + 10.  Each square
carries (2 |d| e_d + e_d^2):
    |per - per64| <= [sum (2 |d| e_d + e_d^2) + L u sum d^2] / (S P) + 2 u per64
loss = (sum of the active means in sample order) / n:   tol = mean_active tol_per + (n + 2) u loss64.   count exact;  stats[2] = fl(fl(1 / (S P)) / n): 3 u relative.

wgrad.  g_W = fl(s P) (P bf16, s fp32: one rounding) or fma(s, P, g_W): e = u |ref| (accumulate: of the sum, + u |s P| for an unfused product).
g_b = s db (+ g_b): the same.
dx_add.  bf16(fma(s, g, dx)): tol = _rounded(ref, u |ref|).
"""
import torch

from tests import self_transcendence_ref as ST
from tests.gemm_bounds import ulp_bf16

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
GUARD = 64          # guard elements on either side of every output

TRACE_SELECTION = ("(test_sd3_host_sequencing_cpu and tokenwise_timesteps_through_the_emulator) or (test_sd3_engine_with_nextlat_matches_autograd_through_the_oracle "
                   "and lora and plain) or (test_sd3_engine_with_self_flow_matches_autograd_through_the_oracle and plain)")


def _rounded(ref, e):
    return 0.5 * ulp_bf16(ref.abs() + e) + e


def inside(got, ref, tol, what=""):
    err = (got.detach().to(F64).cpu() - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst error / bound = {float((err / tol.clamp_min(1e-300)).max()):.3f}"


class Guarded:
    """an output tensor inside a buffer with GUARD sentinel elements on either side"""

    def __init__(self, shape, dtype, dev, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.sent = 7.0 if dtype != torch.uint8 else 7
        self.buf.fill_(self.sent)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())


# ---- the masked loss ----
def loss_chain(S: int, Pc: int) -> int:
    n8 = S * Pc // 8
    nch = min((n8 + 255) // 256, 256)
    return 8 * ((n8 + nch * 256 - 1) // (nch * 256)) + nch + 10


def loss_bounds(pred, t64, e_t, sigmas, tmin, tmax):
    """pred [B, S, Pc] (stored bf16), t64 / e_t [B, S, Pc] fp64 -> dict of (ref, tol) for G, per_sample, loss, and the exact count / inv"""
    p = pred.to(F64)
    B, S, Pc = p.shape
    d = p - t64
    e_d = e_t + U * d.abs()
    m = ST.mask64(sigmas, tmin, tmax)
    G = 2.0 * d * m.to(F64)[:, None, None]
    tol_G = torch.where(m[:, None, None].expand_as(d), _rounded(2.0 * d, 2.0 * e_d), torch.zeros_like(d))
    per = (d * d).flatten(1).mean(1)
    L = loss_chain(S, Pc)
    tol_per = ((2 * d.abs() * e_d + e_d * e_d).flatten(1).sum(1) + L * U * (d * d).flatten(1).sum(1)) / (S * Pc) + 2 * U * per
    n = int(m.sum())
    loss = per[m].mean() if n else torch.zeros((), dtype=F64)
    tol_loss = (tol_per[m].mean() + (n + 2) * U * loss) if n else torch.zeros((), dtype=F64)
    inv = 1.0 / (n * S * Pc) if n else 0.0
    return dict(G=(G, tol_G), per=(per, tol_per), loss=(loss, tol_loss), n=n, inv=inv, mask=m)


def _check_loss_outputs(b, G, per_sample, stats, what):
    inside(G.t.float().view(b["G"][0].shape), *b["G"], what + " G")
    inside(per_sample.t, *b["per"], what + " per_sample")
    inside(stats.t[0], *b["loss"], what + " loss")
    assert float(stats.t[1]) == float(b["n"]), what
    assert abs(float(stats.t[2]) - b["inv"]) <= 3 * U * b["inv"], what
    assert G.intact() and per_sample.intact() and stats.intact(), what + ": guard bytes"
    assert not bool(torch.isnan(G.t.float()).any()) and not bool(torch.isnan(stats.t).any())
    if b["n"] == 0:
        assert float(stats.t[0]) == 0.0 and float(stats.t[2]) == 0.0 and float(G.t.float().abs().max()) == 0.0, what


_lat = lambda B, H, W: (B, 16, H, W)
VAE_CASES = [
    dict(id="D64-in-out", shape=_lat(2, 10, 14), S=35, D=64, sigmas=[0.55, 0.9], tmin=0.4, tmax=0.7, dtype=BF16),
    dict(id="D1536-slice-in-out", shape=_lat(2, 10, 14), S=35, D=1536, sigmas=[0.55, 0.9], tmin=0.4, tmax=0.7, dtype=BF16),
    dict(id="fp32-target", shape=_lat(2, 10, 14), S=35, D=64, sigmas=[0.55, 0.9], tmin=0.4, tmax=0.7, dtype=F32),
    dict(id="none-active", shape=_lat(2, 10, 14), S=35, D=64, sigmas=[0.1, 0.9], tmin=0.4, tmax=0.7, dtype=BF16),
    dict(id="B1", shape=_lat(1, 10, 14), S=35, D=64, sigmas=[0.5], tmin=0.4, tmax=0.7, dtype=BF16),
    dict(id="square-patch1", shape=_lat(2, 6, 6), S=36, D=64, sigmas=[0.55, 0.9], tmin=0.4, tmax=0.7, dtype=BF16),
    dict(id="inclusive-ends", shape=_lat(2, 10, 14), S=35, D=64, sigmas=[0.5, 0.75], tmin=0.5, tmax=0.75, dtype=BF16),
    dict(id="strided-target", shape=_lat(2, 10, 14), S=35, D=64, sigmas=[0.55, 0.6], tmin=0.4, tmax=0.7, dtype=BF16, strided=True),
]


def check_vae_loss(fn, case, dev):
    """fn(pred, target, grid, sigmas, tmin, tmax, per_sample, stats): element-wise inside the bound, guard bytes intact, two launches bit-identical"""
    g = torch.Generator().manual_seed(101)
    B, C, H, W = case["shape"]
    S, D = case["S"], case["D"]
    gh, gw = ST.factor_grid64((H, W), S)
    P = C * (H // gh) * (W // gw)
    proj = torch.randn(B * S, D, generator=g).to(BF16)                      # the projection's D columns: the kernel is handed the P that are read, compact
    pred0 = proj[:, :P].contiguous()
    target = torch.randn(B, C, H, W, generator=g).to(case["dtype"])
    if case.get("strided"):                                                  # samples further apart than C H W
        big = torch.zeros(B, C * H * W + 16, dtype=case["dtype"])
        big[:, :C * H * W] = target.view(B, -1)
        target_dev = big.to(dev)[:, :C * H * W].view(B, C, H, W)
    else:
        target_dev = target.to(dev)
    sig = torch.tensor(case["sigmas"], dtype=F32)
    tokens = ST.vae_target_tokens64(target, S)
    b = loss_bounds(pred0.view(B, S, P), tokens, torch.zeros_like(tokens), sig, case["tmin"], case["tmax"])
    runs = []
    for _ in range(2):
        G, per, st = Guarded((B * S, P), BF16, dev, pred0), Guarded((B,), F32, dev), Guarded((3,), F32, dev)
        fn(G.t, target_dev, (gh, gw), sig.to(dev), case["tmin"], case["tmax"], per.t, st.t)
        _check_loss_outputs(b, G, per, st, f"st_vae_loss[{case['id']}]")
        runs.append((G.t.clone(), per.t.clone(), st.t.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*runs)), "two launches differ"
    if case["id"] == "inclusive-ends":
        assert b["n"] == 2
    return b


CFG_CASES = [dict(id=f"D{D}-cfg{s:g}", D=D, scale=s, S=35, sigmas=[0.55, 0.9], tmin=0.4, tmax=0.7) for D in (64, 1536) for s in (1.0, 30.0)] + \
            [dict(id="D64-both-active", D=64, scale=30.0, S=35, sigmas=[0.4, 0.7], tmin=0.4, tmax=0.7)]


def check_cfg_loss(fn, case, dev):
    """fn(pred, capture, cfg_scale, sigmas, tmin, tmax, per_sample, stats) on the [2B, S, D] capture as a VIEW (row stride D + 8)"""
    g = torch.Generator().manual_seed(103)
    B, S, D, s = 2, case["S"], case["D"], case["scale"]
    pred0 = torch.randn(B * S, D, generator=g).to(BF16)
    big = torch.randn(2 * B, S, D + 8, generator=g).to(BF16)
    cap = big[:, :, :D]
    c, u = cap[:B].to(F64), cap[B:].to(F64)
    s32 = float(torch.tensor(s, dtype=F32))
    t = u + s32 * (c - u)
    e_t = 2 * U * abs(s) * (c - u).abs() + U * t.abs()
    sig = torch.tensor(case["sigmas"], dtype=F32)
    b = loss_bounds(pred0.view(B, S, D), t, e_t, sig, case["tmin"], case["tmax"])
    cap_dev = big.to(dev)[:, :, :D]
    runs = []
    for _ in range(2):
        G, per, st = Guarded((B * S, D), BF16, dev, pred0), Guarded((B,), F32, dev), Guarded((3,), F32, dev)
        fn(G.t, cap_dev, s, sig.to(dev), case["tmin"], case["tmax"], per.t, st.t)
        _check_loss_outputs(b, G, per, st, f"st_cfg_loss[{case['id']}]")
        runs.append((G.t.clone(), per.t.clone(), st.t.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*runs)), "two launches differ"
    if s == 1.0:          # target = c up to the derived bound
        assert float(((t - c).abs() - e_t).max()) <= 0
    return b


# ---- fold ----
FOLD_CASES = [dict(id=f"D{D}-Hp{Hp}-{stage}", D=D, Hp=Hp, P3=(64 if stage == "vae" else D), stage=stage) for (D, Hp) in ((64, 128), (1536, 128)) for stage in ("vae", "self")]


def check_fold(fn, case, dev):
    g = torch.Generator().manual_seed(107)
    D, Hp, P3 = case["D"], case["Hp"], case["P3"]
    shapes = ((Hp, D), (Hp,), (Hp, Hp), (Hp,), (D, Hp), (D,))
    params = [torch.randn(*s, generator=g) / 8 for s in shapes]
    z = torch.zeros((), dtype=F64)
    runs = []
    for _ in range(2):
        outs = [Guarded(s, BF16, dev) for s in ((Hp, D), (D, Hp), (Hp,), (Hp, Hp), (Hp, Hp), (Hp,), (D, Hp), (Hp, P3), (D,))]
        fn(*(p.to(dev) for p in params), *(o.t for o in outs))
        W1h, W1T, b1h, W2h, W2T, b2h, W3h, W3T, b3h = (o.t.float().cpu() for o in outs)
        W1, b1, W2, b2, W3, b3 = (p.to(F64) for p in params)
        for got, ref, nm in ((W1h, W1, "W1h"), (W1T, W1.t(), "W1T"), (b1h, b1, "b1h"), (W2h, W2, "W2h"), (W2T, W2.t(), "W2T"), (b2h, b2, "b2h"),
                             (W3h[:P3], W3[:P3], "W3h"), (W3T, W3[:P3].t(), "W3T"), (b3h[:P3], b3[:P3], "b3h")):
            inside(got, ref, _rounded(ref, z), f"st_fold[{case['id']}] {nm}")
        assert torch.equal(W1h.t(), W1T) and torch.equal(W2h.t(), W2T) and torch.equal(W3h[:P3].t(), W3T)
        # the P3-row form leaves the rest of its output buffers untouched
        assert bool((W3h[P3:] == 7.0).all()) and bool((b3h[P3:] == 7.0).all()) and all(o.intact() for o in outs), f"st_fold[{case['id']}]: guard bytes"
        runs.append([o.t.clone() for o in outs])
    assert all(torch.equal(a, c) for a, c in zip(*runs)), "two launches differ"


# ---- wgrad / dx_add ----
WGRAD_CASES = [dict(id=f"{R}x{Cc}-{'acc' if acc else 'write'}", R=R, Cc=Cc, acc=acc) for (R, Cc) in ((72, 136), (128, 1536)) for acc in (False, True)]


def check_wgrad(fn, case, dev):
    """(72 x 136: 1224 chunks of 8 — the last workgroup of 256 lanes is ragged, and so is the bias workgroup)"""
    g = torch.Generator().manual_seed(109)
    R, Cc, acc = case["R"], case["Cc"], case["acc"]
    P = torch.randn(R, Cc, generator=g).to(BF16)
    db = torch.randn(R, generator=g)
    prevW, prevb = torch.randn(R, Cc, generator=g), torch.randn(R, generator=g)
    s = torch.tensor([0.37], dtype=F32)
    s64 = float(s)
    refW = s64 * P.to(F64) + (prevW.to(F64) if acc else 0)
    refb = s64 * db.to(F64) + (prevb.to(F64) if acc else 0)
    tolW = U * refW.abs() + (U * (s64 * P.to(F64)).abs() if acc else 0)
    tolb = U * refb.abs() + (U * (s64 * db.to(F64)).abs() if acc else 0)
    runs = []
    for _ in range(2):
        gW, gb = Guarded((R, Cc), F32, dev, prevW), Guarded((R,), F32, dev, prevb)
        fn(P.to(dev), db.to(dev), s.to(dev), gW.t, gb.t, accumulate=acc)
        inside(gW.t, refW, tolW, f"st_wgrad[{case['id']}] g_W")
        inside(gb.t, refb, tolb, f"st_wgrad[{case['id']}] g_b")
        assert gW.intact() and gb.intact()
        runs.append((gW.t.clone(), gb.t.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*runs))


DX_CASES = [dict(id=f"D{D}", D=D, rows=35, extra=9) for D in (64, 1536)]


def check_dx_add(fn, case, dev):
    """dx: rows [extra, extra + rows) of every sample of a joint [B, extra + rows, D] buffer; the other rows keep their bytes"""
    g = torch.Generator().manual_seed(113)
    B, rows, D, extra = 2, case["rows"], case["D"], case["extra"]
    joint = torch.randn(B, extra + rows, D, generator=g).to(BF16)
    add = torch.randn(B * rows, D, generator=g).to(BF16)
    s = torch.tensor([-0.61], dtype=F32)
    ref = joint[:, extra:].to(F64) + float(s) * add.to(F64).view(B, rows, D)
    runs = []
    for _ in range(2):
        J = Guarded((B, extra + rows, D), BF16, dev, joint)
        fn(add.to(dev), s.to(dev), J.t[:, extra:])
        inside(J.t[:, extra:].float(), ref, _rounded(ref, U * ref.abs()), f"st_dx_add[{case['id']}]")
        assert torch.equal(J.t[:, :extra].cpu(), joint[:, :extra]) and J.intact()
        runs.append(J.t.clone())
    assert torch.equal(*runs)

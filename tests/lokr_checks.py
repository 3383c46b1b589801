"""Checkers shared by the CPU and GPU LoKr tests — TEST INFRASTRUCTURE ONLY: each runs one op of a namespace `fns` (the wrappers of simpletuner_amd.ops on the GPU, or
the stand-ins of tests/lokr_ref.py on the CPU) on seeded operands, with guard elements behind every output, and holds the result to the derived bound of
tests/lokr_bounds.py around the fp64 reference on the same operands."""
from types import SimpleNamespace

import torch

from tests import lokr_bounds as LB

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
W1_SIDES = [(2, 2), (8, 4), (16, 16)]
ROWS = [("compact", 1, 37), ("compact", 1, 154), ("view", 2, 64)]          # ragged; the text rows; a [B, rows, C] view of a joint buffer


def _guarded(shape, dtype, dev, sentinel=-7.0):
    """a contiguous tensor of `shape` at the head of a larger buffer whose tail holds a sentinel: (tensor, tail)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device=dev)
    return buf[:n].view(*shape), buf[n:]


def _layout(kind, B, rows, C, dev, g):
    """B * rows logical rows of C columns: a compact [B * rows, C] tensor, or the [B, rows, C] view of a taller, wider joint buffer; (operand, logical rows)"""
    vals = torch.randn(B * rows, C, generator=g).to(BF16)
    if kind == "compact":
        t = vals.to(dev)
        return t, t
    joint = torch.full((B, rows + 9, C + 16), 3.0, dtype=BF16, device=dev)
    view = joint[:, 4:4 + rows, 8:8 + C]
    view.copy_(vals.view(B, rows, C).to(dev))
    return view, vals.to(dev)


def run_fold(fns, dev, ol, im, ok, in_, G, s, seed=0, gap=0):
    """G targets of ol * ok rows each (+ `gap` rows without an adapter behind them) over one input of im * in columns"""
    g = torch.Generator().manual_seed(seed)
    N, K = ol * ok, im * in_
    Nt = G * N + gap
    W = (torch.randn(Nt, K, generator=g) / K ** 0.5).to(BF16).to(dev)
    facs = [((torch.rand(ol, im, generator=g) * 2 - 1).to(dev), (0.05 * torch.randn(ok, in_, generator=g)).to(dev)) for _ in range(G)]
    Wf, WfT = _guarded((Nt, K), BF16, dev), _guarded((K, Nt), BF16, dev)
    w2b = [_guarded((ok, in_), BF16, dev) for _ in range(G)]
    fns.lokr_fold(W, [(i * N, N, w1, w2, w2b[i][0]) for i, (w1, w2) in enumerate(facs)], s, Wf[0], WfT[0])
    return SimpleNamespace(W=W, facs=facs, N=N, Wf=Wf, WfT=WfT, w2b=w2b, s=s)


def check_fold(fns, dev, ol, im, ok, in_, G, s=0.7, seed=0, gap=0):
    r = run_fold(fns, dev, ol, im, ok, in_, G, s, seed, gap)
    ok_, worst = LB.inside(r.Wf[0], *LB.fold_ref(r.W, [(i * r.N, r.N, w1, w2) for i, (w1, w2) in enumerate(r.facs)], s))
    print(f"[lokr_fold w1 {ol}x{im} w2 {ok}x{in_} G={G} gap={gap}] Wf: worst error / bound = {worst:.3f}")
    assert ok_, worst
    assert torch.equal(r.WfT[0], r.Wf[0].t())                                      # bitwise the transpose
    for (w1, w2), (b, tail) in zip(r.facs, r.w2b):
        assert LB.inside(b, *LB.w2b_ref(w2))[0] and bool((tail.float() == -7.0).all())
    assert bool((r.Wf[1].float() == -7.0).all()) and bool((r.WfT[1].float() == -7.0).all()), "guard elements written"
    return r


def check_mix(fns, dev, kind, B, rows, ol, im, ok, G, seed=0):
    g = torch.Generator().manual_seed(seed)
    N, n_off = ol * ok, (G - 1) * ol * ok                                           # G = 3: the last slab of a fused q / k / v gradient
    dy, logical = _layout(kind, B, rows, G * N, dev, g)
    w1 = (torch.rand(ol, im, generator=g) * 2 - 1).to(dev)
    out, tail = _guarded((B * rows, im * ok), BF16, dev)
    fns.lokr_mix(dy, n_off, w1, ok, out)
    ok_, worst = LB.inside(out, *LB.mix_ref(logical, n_off, w1, ok))
    print(f"[lokr_mix {kind} {B} x {rows} w1 {ol}x{im} ok={ok} n_off={n_off}] worst error / bound = {worst:.3f}")
    assert ok_, worst
    assert bool((tail.float() == -7.0).all())
    return out.clone()


def check_dw2(fns, dev, kind, B, rows, im, ok, in_, accumulate, seed=0):
    g = torch.Generator().manual_seed(seed)
    M = B * rows
    x, logical = _layout(kind, B, rows, im * in_, dev, g)
    dP = torch.randn(M, im * ok, generator=g).to(BF16).to(dev)
    prev = torch.randn(ok, in_, generator=g).to(dev)
    out, tail = _guarded((ok, in_), F32, dev)
    out.copy_(prev)
    fns.lokr_dw2(dP, x, im, out, alpha=0.7, accumulate=accumulate)
    ok_, worst = LB.inside(out, *LB.dw2_ref(dP, logical, im, ok, 0.7, prev if accumulate else None))
    print(f"[lokr_dw2 {kind} {B} x {rows} im={im} w2 {ok}x{in_} acc={accumulate}] worst error / bound = {worst:.3f}")
    assert ok_, worst
    assert bool((tail == -7.0).all())
    return out.clone()


def check_dw1(fns, dev, kind, B, rows, ol, im, ok, G, accumulate, seed=0):
    g = torch.Generator().manual_seed(seed)
    M, N, n_off = B * rows, ol * ok, (G - 1) * ol * ok
    dy, logical = _layout(kind, B, rows, G * N, dev, g)
    P = torch.randn(M, im * ok, generator=g).to(BF16).to(dev)
    prev = torch.randn(ol, im, generator=g).to(dev)
    out, tail = _guarded((ol, im), F32, dev)
    out.copy_(prev)
    fns.lokr_dw1(dy, n_off, P, out, ok, alpha=0.7, accumulate=accumulate)
    ok_, worst = LB.inside(out, *LB.dw1_ref(logical, n_off, P, ol, im, ok, 0.7, prev if accumulate else None))
    print(f"[lokr_dw1 {kind} {B} x {rows} w1 {ol}x{im} ok={ok} n_off={n_off} acc={accumulate}] worst error / bound = {worst:.3f}")
    assert ok_, worst
    assert bool((tail == -7.0).all())
    return out.clone()

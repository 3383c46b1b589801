"""GPU parity of every HIP kernel, called through the C ABI (simpletuner_amd.ops -> libst355.so), against a
plain fp32 PyTorch statement of the same op on the same seeded inputs.

Tolerances (stated per test): bf16 outputs carry one rounding (2^-8 relative); a contraction of length K in
bf16 inputs / fp32 accumulation adds ~sqrt(K)*2^-9 relative noise on top.  Integer/index work (pack/unpack) is bit-exact.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def rel(a, ref):
    a = a.float(); ref = ref.float()
    return ((a - ref).norm() / (ref.norm() + 1e-30)).item()


def maxabs(a, ref):
    return (a.float() - ref.float()).abs().max().item()


def report(name, a, ref):
    r, m = rel(a, ref), maxabs(a, ref)
    print(f"[parity] {name}: rel_l2={r:.3e} max_abs={m:.3e} ref_max={ref.float().abs().max().item():.3e}")
    return r, m


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


@pytest.fixture(scope="module")
def ops():
    from simpletuner_amd import ops as o

    return o


# ------------------------------------------------------------------------------------------------
# library / streaming
# ------------------------------------------------------------------------------------------------
def test_library_identity():
    from simpletuner_amd import lib

    L = lib.load()
    assert L.st355_arch() == b"gfx950"
    assert L.st355_version() >= 1


def test_flow_noise_mix_given_noise(ops):
    torch.manual_seed(0)
    x = torch.randn(3, 16, 32, 32, device=dev()).to(BF16)
    n = torch.randn_like(x.float()).to(BF16)
    sig = torch.tensor([0.25, 0.5, 0.9], device=dev())
    xt, tg, n_out = ops.flow_noise_mix(x, sig, noise=n)
    s = sig.view(-1, 1, 1, 1)
    ref_xt = ((1 - s) * x.float() + s * n.float())
    ref_tg = n.float() - x.float()
    r1, _ = report("flow x_t", xt, ref_xt)
    r2, _ = report("flow target", tg, ref_tg)
    assert r1 < 4e-3 and r2 < 4e-3  # one bf16 rounding
    assert n_out is n or torch.equal(n_out, n)


def test_flow_noise_mix_generated_noise_statistics(ops):
    x = torch.zeros(4, 16, 128, 128, device=dev(), dtype=BF16)
    sig = torch.ones(4, device=dev())
    xt, tg, n = ops.flow_noise_mix(x, sig, noise=None, seed=1234, offset=0)
    nf = n.float()
    print(f"[parity] philox normal: mean={nf.mean().item():.4f} std={nf.std().item():.4f} kurt={(nf**4).mean().item():.3f}")
    assert abs(nf.mean().item()) < 5e-3 and abs(nf.std().item() - 1.0) < 5e-3 and abs((nf ** 4).mean().item() - 3.0) < 0.1
    assert torch.equal(xt, n) and torch.equal(tg, n)  # sigma=1, x=0
    _, _, n2 = ops.flow_noise_mix(x, sig, noise=None, seed=1234, offset=0)
    assert torch.equal(n, n2)  # counter-based: reproducible
    _, _, n3 = ops.flow_noise_mix(x, sig, noise=None, seed=1234, offset=x.numel() // 4)
    assert not torch.equal(n, n3)


def test_ddpm_noise_mix(ops):
    torch.manual_seed(1)
    x = torch.randn(2, 4, 64, 64, device=dev()).to(BF16)
    n = torch.randn(2, 4, 64, 64, device=dev()).to(BF16)
    acp = torch.tensor([0.9, 0.2], device=dev())
    a, s = acp.sqrt(), (1 - acp).sqrt()
    xt, v = ops.ddpm_noise_mix(x, n, a, s)
    av, sv = a.view(-1, 1, 1, 1), s.view(-1, 1, 1, 1)
    assert report("ddpm x_t", xt, av * x.float() + sv * n.float())[0] < 4e-3
    assert report("ddpm v", v, av * n.float() - sv * x.float())[0] < 4e-3


def test_mse_loss_and_grad(ops):
    torch.manual_seed(2)
    p = torch.randn(4, 16, 32, 32, device=dev()).to(BF16)
    t = torch.randn(4, 16, 32, 32, device=dev()).to(BF16)
    w = torch.tensor([1.0, 0.5, 2.0, 0.25], device=dev())
    for weight in (None, w):
        pf = p.float().requires_grad_(True)
        l = ((pf - t.float()) ** 2)
        if weight is not None:
            l = l * weight.view(-1, 1, 1, 1)
        per = l.mean(dim=(1, 2, 3))
        ref = per.mean()
        ref.backward()
        loss, per_s, dp = ops.mse_loss(p, t, weight=weight)
        print(f"[parity] mse loss={loss.item():.7f} ref={ref.item():.7f}")
        assert abs(loss.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
        assert torch.allclose(per_s, per.detach(), rtol=1e-5, atol=1e-6)
        assert report("mse dpred", dp, pf.grad)[0] < 4e-3


def test_flux_pack_unpack_bit_exact(ops):
    torch.manual_seed(3)
    lat = torch.randn(2, 16, 24, 40, device=dev()).to(BF16)
    B, Cc, H, W = lat.shape
    # reference: flux/__init__.py:25-45
    ref = lat.view(B, Cc, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), Cc * 4)
    packed = ops.flux_pack(lat)
    assert torch.equal(packed, ref)
    back = ops.flux_unpack(packed, Cc, H, W)
    assert torch.equal(back, lat)


def test_timestep_proj_silu_add_scale(ops):
    t = torch.tensor([0.0, 0.1234, 0.5, 1.0], device=dev())
    out = ops.timestep_proj(t, 256, 1000.0)
    half = 128
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, device=dev(), dtype=torch.float32) / half)
    ang = (t * 1000.0)[:, None] * freqs[None]
    ref = torch.cat([ang.cos(), ang.sin()], dim=-1)
    # fp32 cos/sin of arguments up to 1000 rad: allow 2e-3 absolute (bf16 output rounding is 4e-3 relative)
    assert report("timestep_proj", out, ref)[1] < 8e-3
    x = torch.randn(5, 3072, device=dev()).to(BF16)
    y = torch.randn(5, 3072, device=dev()).to(BF16)
    assert report("silu", ops.silu(x), torch.nn.functional.silu(x.float()))[0] < 4e-3
    assert report("add", ops.add(x, y), x.float() + y.float())[0] < 4e-3
    big = torch.randn(2 * 96, 512, device=dev()).to(BF16)
    gate = torch.randn(2, 6 * 512, device=dev()).to(BF16)[:, 1024:1536]
    ref = big.float().view(2, 96, 512) * gate.float()[:, None, :]
    assert report("scale_cols", ops.scale_cols(big, gate, 96), ref.view(-1, 512))[0] < 4e-3


# ------------------------------------------------------------------------------------------------
# GEMM family
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 200, 256), (1, 3072, 256), (4608, 3072, 3072), (512, 64, 3072),
                                   (4608, 128, 9216), (2000, 96, 3072), (4096, 64, 3072)])   # last three: split-K (thin N) path
def test_gemm_plain(ops, M, N, K):
    torch.manual_seed(10)
    a = torch.randn(M, K, device=dev()).to(BF16)
    w = (torch.randn(N, K, device=dev()) * 0.05).to(BF16)
    out = ops.gemm(a, w)
    ref = a.float() @ w.float().t()
    r, _ = report(f"gemm {M}x{N}x{K}", out, ref)
    assert r < 5e-3
    # transpose detector: asymmetric operands -> out^T must NOT match
    if M == N:
        assert rel(out.t(), ref) > 0.1


@pytest.mark.parametrize("M,P,Q", [(64, 256, 256), (192, 512, 264), (4096, 1536, 1536), (960, 136, 3072), (4352, 3072, 768), (8640, 640, 640), (8704, 320, 640)])
def test_gemm_tn_weight_gradient(ops, M, P, Q):
    """dW[P,Q] = dY[M,P]^T X[M,Q] (+ accumulate): contraction over the slow axis of both operands (transposing LDS reads)"""
    torch.manual_seed(21)
    dy = (torch.randn(M, P, device=dev()) * 0.5).to(BF16)
    x = torch.randn(M, Q, device=dev()).to(BF16)
    out = ops.gemm_tn(dy, x)
    ref = dy.float().t() @ x.float()
    r, _ = report(f"gemm_tn {P}x{Q} over {M}", out, ref)
    assert r < 5e-3
    if P == Q:
        assert rel(out.t(), ref) > 0.1                      # transpose detector
    acc0 = torch.randn(P, Q, device=dev()).to(BF16)
    acc = acc0.clone()
    ops.gemm_tn(dy, x, out=acc, accumulate=True)
    assert report("gemm_tn accumulate", acc, ref + acc0.float())[0] < 6e-3
    # strided operands: column slices of wider buffers (how the engine hands per-projection dY blocks)
    wide = torch.randn(M, P + 64, device=dev()).to(BF16)
    o2 = ops.gemm_tn(wide[:, 32:32 + P] if False else wide[:, 64:], x)
    assert report("gemm_tn strided L", o2, wide[:, 64:].float().t() @ x.float())[0] < 5e-3


def test_colsum_prod_and_transpose(ops):
    """token-axis reductions of the full fine-tune backward + the bf16 transpose that refreshes W^T"""
    torch.manual_seed(31)
    B, S, N = 3, 231, 1536
    dy = torch.randn(B * S, N, device=dev()).to(BF16); y = torch.randn(B * S, N, device=dev()).to(BF16)
    out = torch.zeros(B, 2 * N, device=dev(), dtype=torch.float32)[:, N:]                 # strided fp32 destination (a slice of dmod)
    ops.colsum_prod(dy, out, rows_per_batch=S)
    assert report("colsum per batch", out, dy.float().view(B, S, N).sum(1))[0] < 1e-5
    ops.colsum_prod(dy, out, b=y, rows_per_batch=S, accumulate=True)
    assert report("colsum prod accumulate", out, dy.float().view(B, S, N).sum(1) + (dy.float() * y.float()).view(B, S, N).sum(1))[0] < 1e-5
    bias = torch.zeros(1, N, device=dev(), dtype=torch.float32)
    ops.colsum_prod(dy, bias)
    assert report("bias grad", bias[0], dy.float().sum(0))[0] < 1e-5
    # modulation-scale gradient from the saved LN output (mode 1)
    x = torch.randn(B * S, N, device=dev()).to(BF16)
    mod = (torch.randn(B, 2 * N, device=dev()) * 0.3).to(BF16)
    shift, scale = mod[:, :N], mod[:, N:]
    n = ops.ln_modulate_fwd(x, scale, shift, S)
    dsh = torch.zeros(B, N, device=dev(), dtype=torch.float32); dsc = torch.zeros_like(dsh)
    ops.colsum_prod(dy, dsh, rows_per_batch=S)
    ops.colsum_prod(dy, dsc, b=n, rows_per_batch=S, mode=1, prev=dsh, shift=shift, scale=scale)
    xh = torch.nn.functional.layer_norm(x.float(), (N,), eps=1e-6)
    ref = (dy.float() * xh).view(B, S, N).sum(1)
    assert report("dscale via saved n", dsc, ref)[0] < 2e-2
    w = torch.randn(1536, 4608, device=dev()).to(BF16)
    assert torch.equal(ops.transpose(w), w.t().contiguous())
    assert torch.equal(ops.transpose(w[:, 512:1536]), w[:, 512:1536].t().contiguous())


def test_gemm_gate_residual_keeps_branch_output(ops):
    torch.manual_seed(32)
    B, S, D, K = 2, 300, 512, 256
    a = torch.randn(B * S, K, device=dev()).to(BF16); w = (torch.randn(D, K, device=dev()) * 0.1).to(BF16)
    bias = torch.randn(D, device=dev()).to(BF16); gate = torch.randn(B, D, device=dev()).to(BF16); res = torch.randn(B * S, D, device=dev()).to(BF16)
    ybr = torch.empty(B * S, D, device=dev(), dtype=BF16)
    out = ops.gemm(a, w, bias=bias, epilogue=ops.EPI_GATE_RESIDUAL, aux_in=res, gate=gate, rows_per_batch=S, aux_out=ybr)
    y = a.float() @ w.float().t() + bias.float()
    assert report("un-gated branch output", ybr, y)[0] < 5e-3
    assert report("gated residual", out, res.float() + (gate.float()[:, None, :] * y.view(B, S, D)).view(B * S, D))[0] < 5e-3


def test_gemm_ring_race_screen(ops):
    """the LDS-DMA ring (counted vmcnt + raw barriers, two wave groups one barrier apart) is only correct if every read sits behind
    the wait + barrier that retires its region: screen for rare early reads — many runs over shapes with different K-tile counts
    (1, 2, 3 tiles exercise the prologue / tail counts), uneven M, concurrent launches; results must be bit-identical run to run and
    match the fp32 reference."""
    torch.manual_seed(77)
    for (M, N, K) in [(4608, 3072, 64), (4608, 3072, 128), (4608, 3072, 192), (4352, 4608, 1536), (8192, 8192, 2048)]:
        a = torch.randn(M, K, device=dev()).to(BF16); w = (torch.randn(N, K, device=dev()) * 0.05).to(BF16)
        ref = a.float() @ w.float().t()
        first = ops.gemm(a, w)
        assert report(f"race-screen gemm {M}x{N}x{K}", first, ref)[0] < 5e-3
        for _ in range(12):
            assert torch.equal(ops.gemm(a, w), first)
    for (M, P, Q) in [(64, 3072, 1536), (128, 1536, 3072), (4096, 3072, 3072)]:
        l = torch.randn(M, P, device=dev()).to(BF16); r = torch.randn(M, Q, device=dev()).to(BF16)
        first = ops.gemm_tn(l, r)
        assert report(f"race-screen gemm_tn {P}x{Q} over {M}", first, l.float().t() @ r.float())[0] < 5e-3
        for _ in range(12):
            assert torch.equal(ops.gemm_tn(l, r), first)


def test_gemm_identity_asymmetric(ops):
    # A = I (padded), asymmetric B: catches row/col swaps in the C write (cdna guide §3 "A=I-check")
    K = 128
    a = torch.eye(K, device=dev()).to(BF16)
    w = (torch.arange(200 * K, device=dev(), dtype=torch.float32).view(200, K) % 251 - 125).to(BF16)
    out = ops.gemm(a, w)
    assert torch.equal(out.float(), w.float().t())


def test_gemm_bias_gelu_aux(ops):
    torch.manual_seed(11)
    M, N, K = 260, 384, 192
    a = torch.randn(M, K, device=dev()).to(BF16)
    w = (torch.randn(N, K, device=dev()) * 0.1).to(BF16)
    b = torch.randn(N, device=dev()).to(BF16)
    pre = torch.empty(M, N, device=dev(), dtype=BF16)
    out = ops.gemm(a, w, bias=b, epilogue=ops.EPI_GELU, aux_out=pre)
    ref_pre = a.float() @ w.float().t() + b.float()
    assert report("gemm+bias pre-act", pre, ref_pre)[0] < 5e-3
    assert report("gemm+bias+gelu", out, gelu_tanh(pre.float()))[0] < 5e-3
    out2 = ops.gemm(a, w, bias=b)
    assert report("gemm+bias", out2, ref_pre)[0] < 5e-3


def test_gemm_gate_residual_strided(ops):
    torch.manual_seed(12)
    B, S, D, K = 2, 150, 256, 320
    a = torch.randn(B * S, K, device=dev()).to(BF16)
    w = (torch.randn(D, K, device=dev()) * 0.1).to(BF16)
    bias = torch.randn(D, device=dev()).to(BF16)
    mod = torch.randn(B, 6 * D, device=dev()).to(BF16)
    gate = mod[:, 2 * D:3 * D]
    resid_full = torch.randn(B * S, 2 * D, device=dev()).to(BF16)
    resid = resid_full[:, D:]            # strided residual view
    out_full = torch.zeros(B * S, 3 * D, device=dev(), dtype=BF16)
    out = out_full[:, D:2 * D]           # strided output view
    ops.gemm(a, w, bias=bias, out=out, epilogue=ops.EPI_GATE_RESIDUAL, aux_in=resid, gate=gate, rows_per_batch=S)
    ref = resid.float().view(B, S, D) + gate.float()[:, None, :] * (a.float() @ w.float().t() + bias.float()).view(B, S, D)
    assert report("gemm gate+residual", out, ref.view(B * S, D))[0] < 5e-3
    assert out_full[:, :D].abs().max().item() == 0 and out_full[:, 2 * D:].abs().max().item() == 0


def test_gemm_mul_gelu_grad(ops):
    torch.manual_seed(13)
    M, N, K = 200, 512, 128
    dy = torch.randn(M, K, device=dev()).to(BF16)
    wT = (torch.randn(N, K, device=dev()) * 0.1).to(BF16)
    pre = torch.randn(M, N, device=dev()).to(BF16)
    out = ops.gemm(dy, wT, epilogue=ops.EPI_MUL_GELU_GRAD, aux_in=pre)
    pf = pre.float().requires_grad_(True)
    gelu_tanh(pf).backward(dy.float() @ wT.float().t())
    assert report("gemm * gelu'", out, pf.grad)[0] < 6e-3


def test_gemm_lora_extension(ops):
    """fused base + low-rank: y = x W^T + b + (x A^T)(sB)^T  (peft LoraLayer; common.py:1094-1117)"""
    torch.manual_seed(14)
    M, N, K, r, s = 384, 256, 512, 32, 0.5
    x = torch.randn(M, K, device=dev()).to(BF16)
    W = (torch.randn(N, K, device=dev()) * 0.05).to(BF16)
    bias = torch.randn(N, device=dev()).to(BF16)
    A = torch.randn(r, K, device=dev()) * 0.05
    Bm = torch.randn(N, r, device=dev()) * 0.05
    A_pad = torch.zeros(64, K, device=dev(), dtype=BF16); A_T = torch.zeros(K, 64, device=dev(), dtype=BF16)
    Bs_pad = torch.zeros(N, 64, device=dev(), dtype=BF16); Bs_T = torch.zeros(64, N, device=dev(), dtype=BF16)
    ops.lora_pack(A, Bm, s, A_pad, A_T, Bs_pad, Bs_T)
    assert torch.equal(A_pad[:r], A.to(BF16)) and A_pad[r:].abs().max().item() == 0
    assert torch.equal(A_T, A_pad.t()) and torch.equal(Bs_T, Bs_pad.t())
    assert torch.equal(Bs_pad[:, :r], (s * Bm).to(BF16)) and Bs_pad[:, r:].abs().max().item() == 0
    t = ops.gemm(x, A_pad)                       # x A^T  [M,64]
    y = ops.gemm(x, W, bias=bias, a2=t, b2=Bs_pad)
    ref = x.float() @ W.float().t() + bias.float() + (x.float() @ A_pad.float().t()).to(BF16).float() @ Bs_pad.float().t()
    assert report("lora fused fwd", y, ref)[0] < 5e-3
    exact = x.float() @ W.float().t() + bias.float() + s * (x.float() @ A.t()) @ Bm.t()
    assert report("lora fused fwd vs fp32 LoRA", y, exact)[0] < 8e-3


@pytest.mark.parametrize("M,P,Rn,r", [(300, 256, 64, 32), (4608, 3072, 64, 32), (1000, 136, 32, 16)])
def test_skinny_tn(ops, M, P, Rn, r):
    torch.manual_seed(15)
    Lm = torch.randn(M, P, device=dev()).to(BF16)
    R = torch.randn(M, Rn, device=dev()).to(BF16)
    out = torch.zeros(P, r, device=dev())
    ops.skinny_tn(Lm, R, out, r, 1, r, alpha=0.5)
    ref = 0.5 * Lm.float().t() @ R.float()[:, :r]
    assert report(f"skinny_tn {M}x{P}x{Rn}", out, ref)[0] < 1e-5 * math.sqrt(M) + 1e-6
    # transposed output + accumulate
    outT = torch.ones(r, P, device=dev())
    ops.skinny_tn(Lm, R, outT, 1, P, r, alpha=1.0, accumulate=True)
    assert report("skinny_tn^T acc", outT, 1.0 + (Lm.float().t() @ R.float()[:, :r]).t())[0] < 1e-4


def test_skinny_tn_multi_equals_separate_products(ops):
    """st355_skinny_tn_multi: the dA products of the q / k / v adapters that share x in one pass over x — bit-equal to three st355_skinny_tn calls"""
    torch.manual_seed(16)
    M, P, r = 4608, 3072, 32
    x = torch.randn(M, P, device=dev()).to(BF16)
    U = torch.randn(M, 128, device=dev()).to(BF16)
    outs = [torch.zeros(r, P, device=dev()) for _ in range(3)]
    ops.skinny_tn_multi(x, U, outs, 1, P, r, alpha=0.75)
    for g in range(3):
        ref = torch.zeros(r, P, device=dev())
        ops.skinny_tn(x, U[:, 32 * g:32 * g + 32], ref, 1, P, r, alpha=0.75)
        assert torch.equal(outs[g], ref)
        assert report(f"skinny multi block {g}", outs[g], 0.75 * (x.float().t() @ U.float()[:, 32 * g:32 * g + 32]).t())[0] < 1e-4
    acc = [o.clone() for o in outs]
    ops.skinny_tn_multi(x, U, acc, 1, P, r, alpha=0.75, accumulate=True)
    assert all(torch.equal(a, 2 * o) for a, o in zip(acc, outs))


def test_captured_skinny_tn_survives_growth_of_its_scratch(ops, monkeypatch):
    """a hipGraph bakes in the scratch address it was captured with: when a later, larger shape outgrows that scratch, the old buffer must stay allocated
    (ops._scratch retires it), so that replaying the graph neither writes into memory the allocator has handed to someone else nor computes anything else"""
    from simpletuner_amd import lib

    monkeypatch.setattr(ops, "_scratch_bufs", {})           # a table of this test's own: what ran before in this process must not have grown the scratch already
    monkeypatch.setattr(ops, "_scratch_retired", [])
    L = lib.load()
    P, Rn, r, M_small, M_large = 64, 32, 32, 256, 4096
    need_small, need_large = L.st355_skinny_tn_workspace(M_small, P, Rn), L.st355_skinny_tn_workspace(M_large, P, Rn)
    assert 0 < need_small < need_large
    torch.manual_seed(17)
    Ls, Rs = torch.randn(M_small, P, device=dev()).to(BF16), torch.randn(M_small, Rn, device=dev()).to(BF16)
    Ll, Rl = torch.randn(M_large, P, device=dev()).to(BF16), torch.randn(M_large, Rn, device=dev()).to(BF16)
    out_g, out_l, out_e = (torch.zeros(P, r, device=dev()) for _ in range(3))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.skinny_tn(Ls, Rs, out_g, r, 1, r)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.skinny_tn(Ls, Rs, out_g, r, 1, r)
    torch.cuda.current_stream().wait_stream(side)
    captured = ops._scratch("skinny", dev(), need_small)
    captured_ptr, captured_bytes = captured.data_ptr(), captured.numel()
    assert captured_bytes < need_large
    del captured

    ops.skinny_tn(Ll, Rl, out_l, r, 1, r)                 # outgrows the scratch
    assert ops._scratch("skinny", dev(), need_small).data_ptr() != captured_ptr
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    squatters = [torch.full((captured_bytes,), 0xFF, dtype=torch.uint8, device=dev()) for _ in range(4)]
    out_g.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()

    assert [t.data_ptr() for t in ops._scratch_retired] == [captured_ptr]
    assert all(t.data_ptr() != captured_ptr and bool((t == 0xFF).all()) for t in squatters)
    ops.skinny_tn(Ls, Rs, out_e, r, 1, r)
    assert torch.equal(out_g, out_e)
    assert report("skinny_tn replayed", out_g, Ls.float().t() @ Rs.float())[0] < 1e-5 * math.sqrt(M_small) + 1e-6


@pytest.mark.parametrize("B,rows,lo,S,N,K", [(3, 256, 256, 768, 512, 256), (8, 512, 0, 4608, 256, 192), (2, 4096, 512, 4608, 768, 256)])
def test_gemm_segmented_rows_bit_equal_to_per_sample_problems(ops, B, rows, lo, S, N, K):
    """st355_gemm_args.seg_rows: the per-sample row blocks [lo, lo + rows) of joint [B, S, *] buffers as ONE problem (3-D strided views), on the A side, the
    C side, the LoRA extension and the residual — bit-identical to one GEMM per sample on the same tiles, with a gated-residual epilogue on top
    (flux/transformer.py:1332 `torch.cat` / the per-stream projections of a double block)."""
    torch.manual_seed(41)
    d = dev()
    A_joint = torch.randn(B, S, K, device=d).to(BF16)                  # A rows taken out of a joint buffer
    W = (torch.randn(N, K, device=d) * 0.05).to(BF16); bias = torch.randn(N, device=d).to(BF16)
    T = torch.randn(B * rows, 64, device=d).to(BF16)                   # compact LoRA down-projection
    Bs = (torch.randn(N, 64, device=d) * 0.05).to(BF16)
    res = torch.randn(B, S, N, device=d).to(BF16)                      # residual in a joint buffer
    gate = torch.randn(B, N, device=d).to(BF16)
    out_joint = torch.full((B, S, N), 7.0, device=d, dtype=BF16)
    ops.gemm(A_joint[:, lo:lo + rows], W, bias=bias, a2=T, b2=Bs, out=out_joint[:, lo:lo + rows], epilogue=ops.EPI_GATE_RESIDUAL,
             aux_in=res[:, lo:lo + rows], gate=gate, rows_per_batch=rows)
    ref = torch.full((B, S, N), 7.0, device=d, dtype=BF16)
    for b in range(B):
        ops.gemm(A_joint[b, lo:lo + rows], W, bias=bias, a2=T[b * rows:(b + 1) * rows], b2=Bs, out=ref[b, lo:lo + rows], epilogue=ops.EPI_GATE_RESIDUAL,
                 aux_in=res[b, lo:lo + rows], gate=gate[b:b + 1], rows_per_batch=rows)
    assert torch.equal(out_joint, ref)                                 # rows outside the blocks untouched (7.0), rows inside bit-equal
    exact = res[:, lo:lo + rows].float() + gate.float()[:, None] * (A_joint[:, lo:lo + rows].float() @ W.float().t() + bias.float()
                                                                    + (T.float() @ Bs.float().t()).view(B, rows, N))
    assert report("segmented gemm vs fp32", out_joint[:, lo:lo + rows], exact)[0] < 6e-3
    # grouped form: a segmented problem next to a plain one
    o1 = torch.empty(B * rows, N, device=d, dtype=BF16); x2 = torch.randn(512, K, device=d).to(BF16)
    o1b, o2 = ops.gemm_grouped([dict(a=A_joint[:, lo:lo + rows], w=W, out=o1), dict(a=x2, w=W)])
    assert torch.equal(o1b.view(B, rows, N), torch.stack([ops.gemm(A_joint[b, lo:lo + rows], W) for b in range(B)]))
    assert torch.equal(o2, ops.gemm(x2, W))
    # rank-space gradients over the same segmented rows
    dy = torch.randn(B, S, N, device=d).to(BF16)
    g_seg = torch.zeros(N, 32, device=d); g_ref = torch.zeros(N, 32, device=d)
    ops.skinny_tn(dy[:, lo:lo + rows], T, g_seg, 32, 1, 32, alpha=0.5)
    ops.skinny_tn(dy[:, lo:lo + rows].reshape(B * rows, N), T, g_ref, 32, 1, 32, alpha=0.5)
    assert torch.equal(g_seg, g_ref)
    with pytest.raises(Exception):
        ops.gemm(A_joint[:, 1:1 + 200], W)                              # 200-row segments: not a multiple of the 256-row tile


@pytest.mark.parametrize("epi", ["none", "gelu", "gate_residual", "add", "mul_gelu_grad", "segmented_gate_residual_lora"])
def test_gemm_persistent_schedule_is_bit_equal_to_one_tile_per_workgroup(ops, epi):
    """k_gemm_pz (persistent workgroups, LDS ring running across tile seams, epilogue staged in the ring's idle regions, residual rows prefetched a
    sub-pass ahead) against k_gemm_pq on problems of more than one round of 256x256 tiles: every output BIT-identical, three launches each (a seam race
    would show as a non-repeatable difference), odd and even K-tile counts (the ring parity flips per tile when odd), and against fp32 torch."""
    torch.manual_seed(77)
    d = dev()
    M, N, K = (5 * 256 * 4, 18 * 256, 320) if epi != "segmented_gate_residual_lora" else (4 * 1024, 20 * 256, 448)       # 360 / 320 tiles, 5 / 7(+1) K-tiles
    x = torch.randn(M, K, device=d).to(BF16)
    W = (torch.randn(N, K, device=d) * 0.05).to(BF16)
    bias = torch.randn(N, device=d).to(BF16)
    aux = torch.randn(M, N, device=d).to(BF16)
    gate = torch.randn(4, N, device=d).to(BF16)
    kw, ref = dict(bias=bias), x.float() @ W.float().t() + bias.float()
    outs = {}
    if epi == "gelu":
        kw.update(epilogue=ops.EPI_GELU)
        ref = torch.nn.functional.gelu(ref.to(BF16).float(), approximate="tanh")
    elif epi == "gate_residual":
        kw.update(epilogue=ops.EPI_GATE_RESIDUAL, aux_in=aux, gate=gate, rows_per_batch=M // 4)
        ref = aux.float() + gate.float().repeat_interleave(M // 4, dim=0) * ref
    elif epi == "add":
        kw.update(epilogue=ops.EPI_ADD, aux_in=aux)
        ref = ref + aux.float()
    elif epi == "mul_gelu_grad":
        kw.update(epilogue=ops.EPI_MUL_GELU_GRAD, aux_in=aux)
        h = aux.float().requires_grad_(True)
        torch.nn.functional.gelu(h, approximate="tanh").sum().backward()
        ref = ref * h.grad
    elif epi == "segmented_gate_residual_lora":
        B, rows, S, lo = 4, 1024, 1536, 256
        xj = torch.randn(B, S, K, device=d).to(BF16)
        T = torch.randn(B * rows, 64, device=d).to(BF16); Bs = (torch.randn(N, 64, device=d) * 0.05).to(BF16)
        resj = torch.randn(B, S, N, device=d).to(BF16)
    for mode in (0, 1):
        prev = ops.gemm_set_persistent(mode)
        try:
            got = []
            for rep in range(3):
                if epi == "segmented_gate_residual_lora":
                    o = torch.full((B, S, N), 7.0, device=d, dtype=BF16)
                    ops.gemm(xj[:, lo:lo + rows], W, bias=bias, a2=T, b2=Bs, out=o[:, lo:lo + rows], epilogue=ops.EPI_GATE_RESIDUAL,
                             aux_in=resj[:, lo:lo + rows], gate=gate, rows_per_batch=rows)
                    got.append((o, None))
                elif epi == "gelu":
                    pre = torch.empty(M, N, device=d, dtype=BF16)
                    got.append((ops.gemm(x, W, aux_out=pre, **kw), pre))
                else:
                    got.append((ops.gemm(x, W, **kw), None))
            for o, pre in got[1:]:
                assert torch.equal(o, got[0][0]) and (pre is None or torch.equal(pre, got[0][1]))
            outs[mode] = got[0]
        finally:
            ops.gemm_set_persistent(prev)
    assert torch.equal(outs[0][0], outs[1][0]), "persistent schedule differs from the one-tile-per-workgroup schedule"
    if outs[0][1] is not None:
        assert torch.equal(outs[0][1], outs[1][1])
    if epi == "segmented_gate_residual_lora":
        exact = resj[:, lo:lo + rows].float() + gate.float()[:, None] * (xj[:, lo:lo + rows].float() @ W.float().t() + bias.float()
                                                                        + (T.float() @ Bs.float().t()).view(B, rows, N))
        assert report("persistent segmented gemm vs fp32", outs[1][0][:, lo:lo + rows], exact)[0] < 6e-3
        assert (outs[1][0][:, :lo] == 7.0).all() and (outs[1][0][:, lo + rows:] == 7.0).all()
    else:
        assert report(f"persistent gemm [{epi}] vs fp32", outs[1][0], ref)[0] < 8e-3


def test_gemm_grouped_launches_under_the_persistent_schedule(ops):
    """two problems that share one grid (st355_gemm_bf16_grouped) must never be handed to the single-problem persistent kernel as one tile list; pairs whose
    members each fill the chip run one after the other on it.  (r03: the first build walked problem 0 over both problems' tiles — a memory fault.)"""
    torch.manual_seed(78)
    d = dev()
    K, N = 320, 12 * 256
    W = (torch.randn(N, K, device=d) * 0.05).to(BF16)
    big, big2, small = (torch.randn(m, K, device=d).to(BF16) for m in (24 * 256, 23 * 256, 512))
    res = {}
    for mode in (0, 1):
        prev = ops.gemm_set_persistent(mode)
        try:
            res[mode] = ops.gemm_grouped([dict(a=big, w=W), dict(a=small, w=W)]) + ops.gemm_grouped([dict(a=big, w=W), dict(a=big2, w=W)])
        finally:
            ops.gemm_set_persistent(prev)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    for o, x in zip(res[1], (big, small, big, big2)):
        assert report("grouped gemm vs fp32", o, x.float() @ W.float().t())[0] < 5e-3


@pytest.mark.parametrize("S,with_bias", [(512, False), (300, False), (448, True)])
def test_attention_forward_row_major_v_is_bit_equal(ops, S, with_bias):
    """st355_attn_fwd_vrows: V read row-major (token rows of a [B*S, ld] projection buffer) through transposing LDS reads — the same fragments as the
    head-major V^T form, so O and the LSE are bit-identical; ragged last tile and the key-bias variant included"""
    torch.manual_seed(92)
    d_ = dev()
    B, H, hd = 2, 3, 128
    D = H * hd
    Sp = (S + 63) // 64 * 64
    scale = 1.0 / math.sqrt(hd)
    Q = torch.randn(B, H, S, hd, device=d_).to(BF16); K = torch.randn(B, H, S, hd, device=d_).to(BF16)
    qkv = torch.randn(B * S, 3 * D, device=d_).to(BF16)                    # V = the last third of a projection buffer: ld = 3 D
    V = qkv[:, 2 * D:]
    Vt = torch.zeros(B, H, hd, Sp, device=d_, dtype=BF16)
    Vt[..., :S] = V.reshape(B, S, H, hd).permute(0, 2, 3, 1)
    kb = (torch.rand(B, S, device=d_) > 0.25).float() if with_bias else None
    O1 = torch.empty(B * S, D, device=d_, dtype=BF16); l1 = torch.empty(B, H, S, device=d_)
    O2 = torch.empty_like(O1); l2 = torch.empty_like(l1)
    prev = ops.attn_set_impl(fwd=32)                                       # the row-major-V kernel is a form of the 32-query kernel: compare with that one
    try:
        ops.attn_fwd(Q, K, Vt, O1, l1, B, H, S, Sp, hd, scale, key_bias=kb)
    finally:
        ops.attn_set_impl(fwd=prev[0])
    ops.attn_fwd_vrows(Q, K, V, O2, l2, B, H, S, hd, scale, key_bias=kb)
    assert torch.equal(O1, O2) and torch.equal(l1, l2)


@pytest.mark.parametrize("B,H,S", [(2, 4, 512), (1, 8, 320), (1, 3, 64), (1, 2, 1152)])
def test_attention_64_row_kernels_against_the_32_row_kernels(ops, B, H, S):
    """k_attn_fwd64 / k_attn_bwd_dq64 (one wave per SIMD, 64 queries per wave, hand-scheduled bodies from tools/kgen) against k_attn_fwd4 / k_attn_bwd_dq on the
    shapes they take over (head_dim 128, no bias, S % 64 == 0; query counts that leave the last 256-query workgroup ragged; one to eighteen key tiles, odd and
    even: prologue-only, loop and both tail paths).  dQ is BIT-identical (same arithmetic, same accumulation order), with and without the fused RoPE epilogue;
    O agrees to bf16 rounding (the 64-row forward takes exponentials against a reference maximum that may lag by up to 2^8), lse2 to 1e-4.  One row of Q is
    spiked against one key in a late tile so that the forward's out-of-line re-reference runs after the first tile as well."""
    torch.manual_seed(93)
    d_ = dev()
    hd = 128
    D = H * hd
    scale = 1.0 / math.sqrt(hd)
    Q = torch.randn(B, H, S, hd, device=d_).to(BF16); K = torch.randn(B, H, S, hd, device=d_).to(BF16)
    if S >= 192:
        Q[0, 0, 5] = (K[0, 0, S - 40].float() * 6).to(BF16)               # a score ~ 6 * 128 / sqrt(128) = 68 nats in the last tile: far beyond the bound
    V = torch.randn(B * S, D, device=d_).to(BF16)
    Vt = V.view(B, S, H, hd).permute(0, 2, 3, 1).contiguous()
    dO = torch.randn(B * S, D, device=d_).to(BF16)
    res = {}
    prev = ops.attn_set_impl()
    try:
        for impl in (32, 64):
            ops.attn_set_impl(fwd=impl, dq=impl)
            O = torch.empty(B * S, D, device=d_, dtype=BF16); lse2 = torch.empty(B, H, S, device=d_)
            ops.attn_fwd(Q, K, Vt, O, lse2, B, H, S, S, hd, scale)
            res[impl] = [O, lse2]
        O, lse2 = res[32]                                                  # one forward state for both backward kernels
        cos, sin = _rope_tables(S, hd, d_)
        cos_p, sin_p = cos[:, 0::2].contiguous(), sin[:, 0::2].contiguous()
        rrms = (0.5 + torch.rand(B * S, 2 * H, device=d_)).contiguous()
        w = [(1 + 0.2 * torch.randn(hd, device=d_)).to(BF16) for _ in range(2)]
        for impl in (32, 64):
            ops.attn_set_impl(fwd=impl, dq=impl, dkv=3 if impl == 32 else 4)
            dQ = torch.empty_like(Q); dK = torch.empty_like(K); dqkv = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
            ops.attn_bwd(Q, K, None, None, V, O, dO, lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, S, hd, scale)
            fused = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
            ops.attn_bwd_rope(Q, K, V, O, dO, lse2, rrms, w[0], w[1], w[0], w[1], 0, cos_p, sin_p, fused, B, H, S, S, hd, scale)
            res[impl] += [dQ, fused, dK, dqkv]
    finally:
        ops.attn_set_impl(fwd=prev[0], dq=prev[1], dkv=prev[2])
    assert report("fwd64 O vs fwd4", res[64][0], res[32][0])[0] < 5e-3
    # the scores are the same fp32 sums of bf16 products in both kernels (the 64-row chains start from -m_ref / scale2 instead of subtracting afterwards):
    # lse2 agrees to fp32 rounding
    assert float((res[64][1] - res[32][1]).abs().max()) < 1e-4
    assert torch.equal(res[64][2], res[32][2]), "dq64 is not bit-identical to dq"
    D3 = res[32][3].shape[1] // 3
    assert torch.equal(res[64][3][:, :D3], res[32][3][:, :D3]), "dq64 with the fused RoPE epilogue is not bit-identical to dq"
    # k_attn_bwd_dkv4 folds the statistics into the MFMA chains and pre-scales K (re-rounded to bf16): dK / dV (head-major, and through the fused RoPE epilogue /
    # as projection-gradient rows) agree with k_attn_bwd_dkv3 to bf16 rounding
    assert report("dkv4 dK vs dkv3", res[64][4], res[32][4])[0] < 6e-3
    assert report("dkv4 dV vs dkv3", res[64][5][:, 2 * D3:], res[32][5][:, 2 * D3:])[0] < 6e-3
    assert report("dkv4 fused-rope dK vs dkv3", res[64][3][:, D3:2 * D3], res[32][3][:, D3:2 * D3])[0] < 6e-3
    assert report("dkv4 fused-rope dV vs dkv3", res[64][3][:, 2 * D3:], res[32][3][:, 2 * D3:])[0] < 6e-3


@pytest.mark.parametrize("with_norm,split,with_bias", [(True, 256, False), (True, 0, False), (False, 0, False), (True, 256, True)])
def test_attention_backward_with_fused_rope_norm_backward(ops, with_norm, split, with_bias):
    """st355_attn_bwd_rope: dq / dk / dv straight into the projection-gradient rows, the RoPE + RMSNorm backward running in the dQ / dK kernels' epilogues,
    against the two-step chain (st355_attn_bwd -> head-major dQ, dK -> st355_qk_rope_norm_bwd).  The fused form skips the bf16 rounding of dQ / dK in between,
    so it is compared with a tolerance; dV is bit-equal."""
    torch.manual_seed(91)
    d_ = dev()
    B, H, S, hd = 2, 2, 512, 128
    D = H * hd
    scale = 1.0 / math.sqrt(hd)
    cos, sin = _rope_tables(S, hd, d_)
    cos_p, sin_p = cos[:, 0::2].contiguous(), sin[:, 0::2].contiguous()
    Q = torch.randn(B, H, S, hd, device=d_).to(BF16); K = torch.randn(B, H, S, hd, device=d_).to(BF16)      # roped head-major activations (z)
    V = torch.randn(B * S, D, device=d_).to(BF16)
    Vt = V.view(B, S, H, hd).permute(0, 2, 3, 1).contiguous()
    rrms = (0.5 + torch.rand(B * S, 2 * H, device=d_)).contiguous()
    mk = lambda: (1 + 0.2 * torch.randn(hd, device=d_)).to(BF16) if with_norm else None
    wq_lo, wk_lo, wq_hi, wk_hi = mk(), mk(), mk(), mk()
    if split == 0:
        wq_lo, wk_lo = wq_hi, wk_hi
    O = torch.empty(B * S, D, device=d_, dtype=BF16); lse2 = torch.empty(B, H, S, device=d_)
    kb = None
    if with_bias:            # the attention-masked training form: an additive per-key bias (flux/transformer.py:170-173)
        kb = torch.zeros(B, S, device=d_); kb[:, :split] = (torch.rand(B, split, device=d_) > 0.3).float()
        kb[:, split:] = 1.0
    ops.attn_fwd(Q, K, Vt, O, lse2, B, H, S, S, hd, scale, key_bias=kb)
    dO = torch.randn(B * S, D, device=d_).to(BF16)
    # two-step chain
    dQ = torch.empty_like(Q); dK = torch.empty_like(K)
    ref = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
    ops.attn_bwd(Q, K, None, None, V, O, dO, lse2, dQ, dK, ref[:, 2 * D:], B, H, S, S, hd, scale, key_bias=kb)
    if split > 0:
        ops.qk_rope_norm_bwd(dQ, dK, Q, K, rrms, wq_lo, wk_lo, cos, sin, ref, B, H, hd, split, 0, S)
    ops.qk_rope_norm_bwd(dQ, dK, Q, K, rrms, wq_hi, wk_hi, cos, sin, ref, B, H, hd, S - split, split, S)
    # fused
    out = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
    ops.attn_bwd_rope(Q, K, V, O, dO, lse2, rrms, wq_lo, wk_lo, wq_hi, wk_hi, split, cos_p, sin_p, out, B, H, S, S, hd, scale, key_bias=kb)
    assert torch.equal(out[:, 2 * D:], ref[:, 2 * D:])
    assert report("fused rope-bwd dq", out[:, :D], ref[:, :D])[0] < 6e-3
    assert report("fused rope-bwd dk", out[:, D:2 * D], ref[:, D:2 * D])[0] < 6e-3


# ------------------------------------------------------------------------------------------------
# AdaLN, RMSNorm + RoPE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3072, 1536, 1152, 256])
def test_ln_modulate_fwd_bwd(ops, D):
    torch.manual_seed(20)
    B, S = 2, 70
    x = (torch.randn(B * S, D, device=dev()) * 2 + 0.3).to(BF16)
    mod = (torch.randn(B, 6 * D, device=dev()) * 0.5).to(BF16)
    shift, scale, gate = mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    y = ops.ln_modulate_fwd(x, scale, shift, S)
    xf = x.float().view(B, S, D).requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xf, (D,), eps=1e-6) * (1 + scale.float()[:, None]) + shift.float()[:, None]
    assert report(f"ln_mod fwd D={D}", y, ref.view(B * S, D))[0] < 4e-3
    dy = torch.randn(B * S, D, device=dev()).to(BF16)
    dres = torch.randn(B * S, D, device=dev()).to(BF16)
    ref.backward(dy.float().view(B, S, D))
    dx, dxg = ops.ln_modulate_bwd(dy, x, scale, S, dres=dres, gate=gate, want_gated=True)
    ref_dx = xf.grad.view(B * S, D) + dres.float()
    assert report(f"ln_mod bwd D={D}", dx, ref_dx)[0] < 6e-3
    assert report("ln_mod bwd gated", dxg, (dx.float().view(B, S, D) * gate.float()[:, None]).view(B * S, D))[0] < 4e-3
    dx2, none = ops.ln_modulate_bwd(dy, x, scale, S)
    assert none is None and report("ln_mod bwd (no dres)", dx2, xf.grad.view(B * S, D))[0] < 6e-3


def _rope_tables(S, d, device):
    # FluxPosEmbed-like interleave-repeated tables with arbitrary (non-trivial) angles
    ang = torch.rand(S, d // 2, device=device, dtype=torch.float64) * 6.0
    cos = ang.cos().repeat_interleave(2, dim=1).float().contiguous()
    sin = ang.sin().repeat_interleave(2, dim=1).float().contiguous()
    return cos, sin


def _ref_norm_rope(x, w, cos, sin, eps=1e-6):
    # x [B,H,S,d] fp32; diffusers RMSNorm then flux/transformer.py:73-98
    if w is not None:
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    xr, xi = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack([-xi, xr], dim=-1).flatten(3)
    return x * cos[None, None] + rot * sin[None, None]


@pytest.mark.parametrize("d,H,S_txt,S_img", [(128, 3, 64, 128), (128, 2, 40, 100), (64, 4, 77, 150)])
def test_qk_norm_rope_fwd_bwd(ops, d, H, S_txt, S_img):
    torch.manual_seed(21)
    B = 2
    S = S_txt + S_img
    Sp = (S + 63) // 64 * 64
    D = H * d
    cos, sin = _rope_tables(S, d, dev())
    wq = (1 + 0.2 * torch.randn(d, device=dev())).to(BF16)
    wk = (1 + 0.2 * torch.randn(d, device=dev())).to(BF16)
    Q = torch.zeros(B, H, S, d, device=dev(), dtype=BF16); K = torch.zeros_like(Q)
    Qt = torch.zeros(B, H, d, Sp, device=dev(), dtype=BF16); Kt = torch.zeros_like(Qt); Vt = torch.zeros_like(Qt)
    parts = [("txt", S_txt, 0), ("img", S_img, S_txt)]
    wq2 = (1 + 0.2 * torch.randn(d, device=dev())).to(BF16)   # the txt stream has its own norm weights (norm_added_q/k)
    wk2 = (1 + 0.2 * torch.randn(d, device=dev())).to(BF16)
    wts = {"txt": (wq2, wk2), "img": (wq, wk)}
    qkv = torch.randn(B * S, 3 * D, device=dev()).to(BF16)       # JOINT buffer, row b*S + pos
    for name, Sp_, pos0 in parts:
        ops.qk_norm_rope_fwd(qkv, wts[name][0], wts[name][1], cos, sin, Q, K, Qt, Kt, Vt, B, H, d, Sp_, pos0, S, Sp)
    q, k, v = qkv.float().view(B, S, 3, H, d).permute(2, 0, 3, 1, 4)
    q = q.contiguous().requires_grad_(True); k = k.contiguous().requires_grad_(True)
    wq_full = torch.cat([wq2.float().expand(S_txt, d), wq.float().expand(S_img, d)], 0)   # per-position weights
    wk_full = torch.cat([wk2.float().expand(S_txt, d), wk.float().expand(S_img, d)], 0)
    Qr = _ref_norm_rope(q, wq_full, cos, sin); Kr = _ref_norm_rope(k, wk_full, cos, sin)
    assert report("rope Q", Q, Qr)[0] < 4e-3 and report("rope K", K, Kr)[0] < 4e-3
    assert torch.equal(Qt[..., :S], Q.transpose(2, 3)) and torch.equal(Kt[..., :S], K.transpose(2, 3))
    assert torch.equal(Vt[..., :S], v.to(BF16).transpose(2, 3))
    if Sp > S:
        assert Qt[..., S:].abs().max().item() == 0 and Vt[..., S:].abs().max().item() == 0
    # Qt / Kt are optional outputs (head_dim 128 backward without transposed copies): the other three outputs are unchanged
    Q2 = torch.zeros_like(Q); K2 = torch.zeros_like(K); Vt2 = torch.zeros_like(Vt)
    for name, Sp_, pos0 in parts:
        ops.qk_norm_rope_fwd(qkv, wts[name][0], wts[name][1], cos, sin, Q2, K2, None, None, Vt2, B, H, d, Sp_, pos0, S, Sp)
    assert torch.equal(Q2, Q) and torch.equal(K2, K) and torch.equal(Vt2, Vt)
    # backward
    dQ = torch.randn(B, H, S, d, device=dev()).to(BF16); dK = torch.randn(B, H, S, d, device=dev()).to(BF16)
    (Qr * dQ.float()).sum().backward(retain_graph=True)
    (Kr * dK.float()).sum().backward()
    dqkv = torch.zeros(B * S, 3 * D, device=dev(), dtype=BF16)
    for name, Sp_, pos0 in parts:
        ops.qk_norm_rope_bwd(dQ, dK, qkv, wts[name][0], wts[name][1], cos, sin, dqkv, B, H, d, Sp_, pos0, S)
    ref_dq = q.grad.permute(0, 2, 1, 3).reshape(B * S, D)
    ref_dk = k.grad.permute(0, 2, 1, 3).reshape(B * S, D)
    assert report("rope bwd dq", dqkv[:, :D], ref_dq)[0] < 6e-3
    assert report("rope bwd dk", dqkv[:, D:2 * D], ref_dk)[0] < 6e-3
    assert dqkv[:, 2 * D:].abs().max().item() == 0


@pytest.mark.parametrize("lora", [False, True])
def test_fused_qkv_projection_epilogue(ops, lora):
    """ST355_EPI_QK_NORM_ROPE: the QKV projection with RMSNorm(q), RMSNorm(k), RoPE and the head-major re-layout in the GEMM epilogue
    (FluxAttnProcessor2_0, flux/transformer.py:140-207) and its backward from the roped Q / K + 1/rms, for both streams of a double block written into the
    joint buffers (segmented V rows).  Checked against fp32 autograd of the same maths and against the unfused kernel chain; V is bit-equal to it."""
    torch.manual_seed(77)
    d_ = dev()
    B, H, hd, St, Si, Kin = 2, 2, 128, 256, 512, 192
    S, D = St + Si, H * hd
    cos, sin = _rope_tables(S, hd, d_)
    cos_p, sin_p = cos[:, 0::2].contiguous(), sin[:, 0::2].contiguous()        # one angle per interleaved pair: what the fused epilogue reads
    streams = {}
    for name, rows, pos0 in (("txt", St, 0), ("img", Si, St)):
        streams[name] = dict(rows=rows, pos0=pos0, x=torch.randn(B * rows, Kin, device=d_).to(BF16), W=(torch.randn(3 * D, Kin, device=d_) * 0.08).to(BF16),
                             bias=(0.1 * torch.randn(3 * D, device=d_)).to(BF16), wq=(1 + 0.2 * torch.randn(hd, device=d_)).to(BF16),
                             wk=(1 + 0.2 * torch.randn(hd, device=d_)).to(BF16), T=torch.randn(B * rows, 64, device=d_).to(BF16),
                             Bs=(torch.randn(3 * D, 64, device=d_) * 0.05).to(BF16))
    Q = torch.zeros(B, H, S, hd, device=d_, dtype=BF16); K = torch.zeros_like(Q)
    rrms = torch.zeros(B * S, 2 * H, device=d_)
    V = torch.zeros(B * S, D, device=d_, dtype=BF16)
    Vt = torch.zeros(B, H, hd, S, device=d_, dtype=BF16)
    probs = []
    for name, st in streams.items():
        kw = dict(a2=st["T"], b2=st["Bs"]) if lora else {}
        probs.append(dict(a=st["x"], w=st["W"], bias=st["bias"], out=V.view(B, S, D)[:, st["pos0"]:st["pos0"] + st["rows"]], epilogue=ops.EPI_QK_NORM_ROPE,
                          rope=ops.qk_rope(Q, K, rrms, st["wq"], st["wk"], cos_p, sin_p, H, S, st["pos0"], Vt=Vt), rows_per_batch=st["rows"], **kw))
    ops.gemm_grouped(probs)
    assert torch.equal(Vt, V.view(B, S, H, hd).permute(0, 2, 3, 1))           # the head-major V^T copy of the same launch
    # the unfused chain: projection rounded to bf16, then the separate norm + rope + re-layout pass
    qkv_u = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
    Sp = (S + 63) // 64 * 64
    Qu = torch.zeros_like(Q); Ku = torch.zeros_like(K); Vtu = torch.zeros(B, H, hd, Sp, device=d_, dtype=BF16)
    x_refs = {}
    for name, st in streams.items():
        kw = dict(a2=st["T"], b2=st["Bs"]) if lora else {}
        ops.gemm(st["x"], st["W"], bias=st["bias"], out=qkv_u.view(B, S, 3 * D)[:, st["pos0"]:st["pos0"] + st["rows"]], **kw)
        ops.qk_norm_rope_fwd(qkv_u, st["wq"], st["wk"], cos, sin, Qu, Ku, None, None, Vtu, B, H, hd, st["rows"], st["pos0"], S, Sp)
        pre = st["x"].float() @ st["W"].float().t() + st["bias"].float()
        if lora:
            pre = pre + st["T"].float() @ st["Bs"].float().t()
        x_refs[name] = pre.view(B, st["rows"], 3, H, hd)
    assert torch.equal(V, qkv_u[:, 2 * D:])                                   # same accumulators, same single rounding
    # fp32 reference of the fused maths (joint order: txt rows then img rows)
    pre = torch.cat([x_refs["txt"], x_refs["img"]], 1)                        # [B, S, 3, H, hd]
    q = pre[:, :, 0].permute(0, 2, 1, 3).contiguous().requires_grad_(True); k = pre[:, :, 1].permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    wq_full = torch.cat([streams["txt"]["wq"].float().expand(St, hd), streams["img"]["wq"].float().expand(Si, hd)], 0)
    wk_full = torch.cat([streams["txt"]["wk"].float().expand(St, hd), streams["img"]["wk"].float().expand(Si, hd)], 0)
    Qr = _ref_norm_rope(q, wq_full, cos, sin); Kr = _ref_norm_rope(k, wk_full, cos, sin)
    eq, ek = report("fused Q vs fp32", Q, Qr)[0], report("fused K vs fp32", K, Kr)[0]
    uq = report("unfused Q vs fp32", Qu, Qr)[0]
    assert eq < 3e-3 and ek < 3e-3 and eq <= uq * 1.02                         # one rounding instead of two: at least as close as the unfused chain
    rr_ref = torch.cat([torch.rsqrt(q.detach().pow(2).mean(-1) + 1e-6), torch.rsqrt(k.detach().pow(2).mean(-1) + 1e-6)], 1)   # [B, 2H, S]
    assert report("rrms", rrms.view(B, S, 2 * H).permute(0, 2, 1), rr_ref)[0] < 1e-5
    # backward from (Q, K, rrms)
    dQ = torch.randn(B, H, S, hd, device=d_).to(BF16); dK = torch.randn(B, H, S, hd, device=d_).to(BF16)
    (Qr * dQ.float()).sum().backward(retain_graph=True); (Kr * dK.float()).sum().backward()
    dqkv = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
    for name, st in streams.items():
        ops.qk_rope_norm_bwd(dQ, dK, Q, K, rrms, st["wq"], st["wk"], cos, sin, dqkv, B, H, hd, st["rows"], st["pos0"], S)
    ref_dq = q.grad.permute(0, 2, 1, 3).reshape(B * S, D); ref_dk = k.grad.permute(0, 2, 1, 3).reshape(B * S, D)
    assert report("fused-form bwd dq", dqkv[:, :D], ref_dq)[0] < 8e-3
    assert report("fused-form bwd dk", dqkv[:, D:2 * D], ref_dk)[0] < 8e-3
    assert dqkv[:, 2 * D:].abs().max().item() == 0
    # no norm weights (RoPE only): rrms is 1, the backward is the transposed rotation
    Q2 = torch.zeros_like(Q); K2 = torch.zeros_like(K); rr2 = torch.zeros_like(rrms); V2 = torch.zeros_like(V)
    st = streams["img"]
    ops.gemm(st["x"], st["W"], out=V2.view(B, S, D)[:, St:], epilogue=ops.EPI_QK_NORM_ROPE, rope=ops.qk_rope(Q2, K2, rr2, None, None, cos_p, sin_p, H, S, St),
             rows_per_batch=Si)
    pre2 = (st["x"].float() @ st["W"].float().t()).view(B, Si, 3, H, hd)
    q2 = pre2[:, :, 0].permute(0, 2, 1, 3)
    assert report("rope only Q", Q2[:, :, St:], _ref_norm_rope(q2, None, cos[St:], sin[St:]))[0] < 3e-3
    assert torch.all(rr2.view(B, S, 2 * H)[:, St:] == 1.0) and Q2[:, :, :St].abs().max().item() == 0


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _attn_case(ops, B, H, S, d, bias=False, spike=False, seed=30):
    torch.manual_seed(seed)
    Sp = (S + 63) // 64 * 64
    D = H * d
    scale = 1.0 / math.sqrt(d)
    q = torch.randn(B, H, S, d, device=dev()).to(BF16)
    k = torch.randn(B, H, S, d, device=dev()).to(BF16)
    qkv_rows = torch.randn(B * S, 3 * D, device=dev()).to(BF16)   # V lives token-major in the qkv buffer
    if d == 96:      # include/st355.h: head_dim 96 is a zero-padded narrower head (<= 80 valid channels; the 64-row kernels contract over 80)
        q[..., 80:] = 0; k[..., 80:] = 0
        qkv_rows.view(B * S, 3, H, d)[..., 80:] = 0
    v_rows = qkv_rows[:, 2 * D:]
    v = v_rows.float().view(B, S, H, d).permute(0, 2, 1, 3)
    if spike:  # force the online-softmax rescale branch: one key dominates late in the sequence
        k[:, :, S - 3] = (q[:, :, 5] * 4.0).to(BF16)
    kb = None
    if bias:
        kb = torch.zeros(B, S, device=dev())
        kb[:, S // 3: S // 2] = -10000.0   # PixArt-style additive mask (pixart/controlnet.py:224-232)
        kb[:, 0] = 0.5
    Qt = torch.zeros(B, H, d, Sp, device=dev(), dtype=BF16); Kt = torch.zeros_like(Qt); Vt = torch.zeros_like(Qt)
    Qt[..., :S] = q.transpose(2, 3); Kt[..., :S] = k.transpose(2, 3); Vt[..., :S] = v.to(BF16).transpose(2, 3)
    O = torch.zeros(B * S, D, device=dev(), dtype=BF16)
    lse2 = torch.zeros(B, H, S, device=dev())
    ops.attn_fwd(q, k, Vt, O, lse2, B, H, S, Sp, d, scale, key_bias=kb)
    qf = q.float().requires_grad_(True); kf = k.float().requires_grad_(True); vf = v.clone().requires_grad_(True)
    s = (qf @ kf.transpose(2, 3)) * scale
    if kb is not None:
        s = s + kb[:, None, None, :]
    p = s.softmax(-1)
    o_ref = p @ vf
    r, m = report(f"attn fwd B{B} H{H} S{S} d{d} bias={bias} spike={spike}", O.view(B, S, H, d).permute(0, 2, 1, 3), o_ref)
    lse_ref = torch.logsumexp(s, -1) / math.log(2.0)
    ml = maxabs(lse2, lse_ref)
    print(f"[parity] lse2 max_abs={ml:.3e}")
    assert r < 8e-3 and ml < 2e-2
    # backward
    dO = torch.randn(B * S, D, device=dev()).to(BF16)
    if d == 96:
        dO.view(B * S, H, d)[..., 80:] = 0
    o_ref.backward(dO.float().view(B, S, H, d).permute(0, 2, 1, 3))
    dQ = torch.zeros(B, H, S, d, device=dev(), dtype=BF16); dK = torch.zeros_like(dQ)
    dqkv = torch.zeros(B * S, 3 * D, device=dev(), dtype=BF16)
    ops.attn_bwd(q, k, Qt, Kt, v_rows, O, dO, lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, Sp, d, scale, key_bias=kb)
    r1, _ = report("attn bwd dQ", dQ, qf.grad)
    r2, _ = report("attn bwd dK", dK, kf.grad)
    r3, _ = report("attn bwd dV", dqkv[:, 2 * D:].reshape(B, S, H, d).permute(0, 2, 1, 3), vf.grad)
    assert r1 < 2e-2 and r2 < 2e-2 and r3 < 2e-2
    assert dqkv[:, :2 * D].abs().max().item() == 0
    if d in (64, 96, 128):
        # without the pre-transposed Q^T / K^T / dO^T copies (dkv3 + dq<TR>: transposing LDS reads on the row-major tiles; r3: head_dim 64 / 96 too, on
        # tile images that keep the 256-byte row pitch): same math, same summation order per accumulator -> bit-identical to the kernels that read the copies
        dQ2 = torch.zeros_like(dQ); dK2 = torch.zeros_like(dK); dqkv2 = torch.zeros_like(dqkv)
        ops.attn_bwd(q, k, None, None, v_rows, O, dO, lse2, dQ2, dK2, dqkv2[:, 2 * D:], B, H, S, Sp, d, scale, key_bias=kb)
        if S % 64 == 0 or kb is not None:
            assert torch.equal(dQ2, dQ)                                   # (k_attn_bwd_dq64, where it applies, is bit-identical as well)
        else:                                                             # ragged key tail: dq64 + the general kernel on the last tile (r6): one extra bf16 rounding of the sum
            assert report("dq64 + tail vs dq", dQ2, dQ)[0] < 3e-3
        if kb is None:
            # every head_dim without a key bias takes the hand-scheduled k_attn_bwd_dkv4 (same scores; the statistics ride in the MFMA chains: another
            # summation order): fp32-rounding agreement; dkv3 itself stays bit-identical to the copy-reading kernel
            assert report("dkv4 dK vs dkv2", dK2, dK)[0] < 2e-3 and report("dkv4 dV vs dkv2", dqkv2[:, 2 * D:], dqkv[:, 2 * D:])[0] < 2e-3
            prev = ops.attn_set_impl(dkv=3)
            try:
                dK3 = torch.zeros_like(dK); dqkv3 = torch.zeros_like(dqkv)
                ops.attn_bwd(q, k, None, None, v_rows, O, dO, lse2, dQ2, dK3, dqkv3[:, 2 * D:], B, H, S, Sp, d, scale, key_bias=kb)
            finally:
                ops.attn_set_impl(dkv=prev[2])
            assert torch.equal(dK3, dK) and torch.equal(dqkv3, dqkv)
        else:
            assert torch.equal(dK2, dK) and torch.equal(dqkv2, dqkv)


@pytest.mark.parametrize("B,H,S,d,cross", [(1, 20, 1024, 64, False), (2, 4, 320, 128, False), (1, 8, 1024, 64, True)])
def test_attention_backward_with_the_output_residual_cancels_the_common_component(ops, B, H, S, d, cross):
    """st355_attn_fwd_res / st355_attn_bwd_res.  k and v carry a component common to all tokens several times larger than their per-token part (projections of a
    LayerNorm output with a dominant mean pattern: the UNet families' attn1 — SDXL's 32^2 level, 20 heads of 64).  Exact arithmetic cancels the common component of k in
    dQ = dS K (sum_j dS_ij = 0); with delta read from the bf16 O every dS row carries P_ij * dO_i.(O_fp32 - O)_i instead — O ~ the common component of v, so its
    rounding error is large against the differences dS is made of — and the cancellation fails (fp64 emulation of this data: dQ rel-L2 ~2 with the bf16 O, 3e-3 with
    O + O_res).  Asserted: O is bit-identical with and without the residual, dV (which does not read delta) too; O + O_res is closer to the exact output than O; dQ
    with the residual <= 0.2 rel-L2 and at least 4 x closer than without; dK <= 2e-2 either way.  fp64 reference on the device."""
    torch.manual_seed(5)
    dv = dev()
    Sk = 77 if cross else S
    Sp, Skp = (S + 63) // 64 * 64, (Sk + 63) // 64 * 64
    D = H * d
    scale = 1.0 / math.sqrt(d)
    cq, ck, cv = torch.randn(1, H, 1, d, device=dv), torch.randn(1, H, 1, d, device=dv) * 2.0, torch.randn(1, H, 1, d, device=dv) * 4.0
    q = (torch.randn(B, H, S, d, device=dv) + cq).to(BF16)
    k = (torch.randn(B, H, Sk, d, device=dv) * 0.2 + ck).to(BF16)
    v = (torch.randn(B, H, Sk, d, device=dv) + cv).to(BF16)
    v_rows = v.permute(0, 2, 1, 3).reshape(B * Sk, D).contiguous()
    Vt = torch.zeros(B, H, d, Skp, device=dv, dtype=BF16); Vt[..., :Sk] = v.transpose(2, 3)
    dO = torch.randn(B * S, D, device=dv).to(BF16)
    q64, k64, v64 = q.double().requires_grad_(True), k.double().requires_grad_(True), v.double().requires_grad_(True)
    o64 = torch.softmax(q64 @ k64.transpose(2, 3) * scale, -1) @ v64
    o64.backward(dO.double().view(B, S, H, d).permute(0, 2, 1, 3))
    out = {}
    for res in (False, True):
        O = torch.empty(B * S, D, device=dv, dtype=BF16); lse2 = torch.empty(B, H, S, device=dv)
        Ores = torch.empty_like(O) if res else None
        dQ = torch.empty(B, H, S, d, device=dv, dtype=BF16); dK = torch.empty(B, H, Sk, d, device=dv, dtype=BF16); dV = torch.empty(B * Sk, D, device=dv, dtype=BF16)
        if cross:
            ops.attn_cross_fwd(q, k, Vt, O, lse2, B, H, S, Sk, Skp, d, scale, O_res=Ores)
            ops.attn_cross_bwd(q, k, None, None, v_rows, O, dO, lse2, dQ, dK, dV, B, H, S, Sp, Sk, Skp, d, scale, O_res=Ores)
        else:
            prev = ops.attn_set_impl(fwd=32)                 # the residual form runs k_attn_fwd4: compare O against the same kernel
            try:
                ops.attn_fwd(q, k, Vt, O, lse2, B, H, S, Sp, d, scale, O_res=Ores)
            finally:
                ops.attn_set_impl(fwd=prev[0])
            ops.attn_bwd(q, k, None, None, v_rows, O, dO, lse2, dQ, dK, dV, B, H, S, Sp, d, scale, O_res=Ores)
        rq, rk = PU_rel(dQ, q64.grad), PU_rel(dK, k64.grad)
        rv = PU_rel(dV.view(B, Sk, H, d).permute(0, 2, 1, 3), v64.grad)
        out[res] = (O, Ores, rq, rk, rv, dV)
        print(f"[parity] attention backward, common component in k and v, residual={res} cross={cross} B{B} H{H} S{S} d{d}: dQ {rq:.3e} dK {rk:.3e} dV {rv:.3e}")
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][5], out[True][5])     # the same O; dV does not read delta
    o_t = o64.detach().permute(0, 2, 1, 3).reshape(B * S, D)
    r_hi, r_both = PU_rel(out[True][0], o_t), PU_rel(out[True][0].double() + out[True][1].double(), o_t)
    print(f"[parity]   O vs exact {r_hi:.3e}, O + O_res vs exact {r_both:.3e}")
    assert r_both < 0.6 * r_hi
    assert out[True][2] < 0.2 and out[True][2] * 4 < out[False][2], (out[False][2], out[True][2])    # what the residual buys on dQ
    assert out[True][3] < 2e-2 and out[False][3] < 5e-2 and out[True][4] < 1e-2


def PU_rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,H,S,hd,dv_", [(1, 16, 1024, 96, 72), (2, 4, 320, 96, 72), (2, 10, 1024, 64, 64), (1, 5, 4096, 64, 64), (2, 3, 192, 64, 64)])
def test_attention_64_row_kernels_narrow_heads(ops, B, H, S, hd, dv_):
    """the head_dim-96 (PixArt-Sigma's 72, zero padded: 5 contraction k-steps in the 64-row forward / dQ bodies — 80 channels —, 6 in the 32-row kernels; 3 d tiles) and head_dim-64 (SDXL / SD3 / SD 1.x: 4 k-steps, 2 d tiles; SDXL's two self-attention
    shapes) builds of the 64-row kernels — tile images at the 256-byte pitch — against the 32-row kernels: O to bf16 rounding, lse2 to fp32 rounding, dQ
    bit-identical, dK / dV to fp32 summation order; padded channels stay zero.  One row of Q is spiked against a key of a late tile (the forward's out-of-line
    re-reference)."""
    torch.manual_seed(94)
    d_ = dev()
    D = H * hd
    scale = 1.0 / math.sqrt(dv_)
    mk = lambda *sh: torch.randn(*sh, device=d_)
    Q, K = mk(B, H, S, hd), mk(B, H, S, hd)
    Q[..., dv_:] = 0; K[..., dv_:] = 0
    if S >= 192:
        Q[0, 0, 5] = K[0, 0, S - 40] * 6
    Q, K = Q.to(BF16), K.to(BF16)
    V = mk(B * S, H, hd); V[..., dv_:] = 0
    V = V.reshape(B * S, D).to(BF16)
    Vt = V.view(B, S, H, hd).permute(0, 2, 3, 1).contiguous()
    dO = mk(B * S, H, hd); dO[..., dv_:] = 0
    dO = dO.reshape(B * S, D).to(BF16)
    res = {}
    prev = ops.attn_set_impl()
    try:
        for impl in (32, 64):
            ops.attn_set_impl(fwd=impl, dq=impl, dkv=3 if impl == 32 else 4)
            O = torch.empty(B * S, D, device=d_, dtype=BF16); lse2 = torch.empty(B, H, S, device=d_)
            ops.attn_fwd(Q, K, Vt, O, lse2, B, H, S, S, hd, scale)
            res[impl] = [O, lse2]
        O, lse2 = res[32]
        for impl in (32, 64):
            ops.attn_set_impl(fwd=impl, dq=impl, dkv=3 if impl == 32 else 4)
            dQ = torch.empty_like(Q); dK = torch.empty_like(K); dqkv = torch.zeros(B * S, 3 * D, device=d_, dtype=BF16)
            ops.attn_bwd(Q, K, None, None, V, O, dO, lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, S, hd, scale)
            res[impl] += [dQ, dK, dqkv]
    finally:
        ops.attn_set_impl(fwd=prev[0], dq=prev[1], dkv=prev[2])
    if hd == 64:             # head_dim 64 keeps the 32-row forward (the generated 64-row body measured slower): the same kernel either way
        assert torch.equal(res[64][0], res[32][0]) and torch.equal(res[64][1], res[32][1])
    assert report(f"fwd64<{hd}> O vs fwd4", res[64][0], res[32][0])[0] < 5e-3
    assert float((res[64][1] - res[32][1]).abs().max()) < 1e-4
    assert torch.equal(res[64][2], res[32][2]), f"dq64<{hd}> is not bit-identical to dq"
    assert report(f"dkv4<{hd}> dK vs dkv3", res[64][3], res[32][3])[0] < 2e-3
    assert report(f"dkv4<{hd}> dV vs dkv3", res[64][4][:, 2 * D:], res[32][4][:, 2 * D:])[0] < 2e-3
    if dv_ < hd:
        for t in (res[64][2], res[64][3]):
            assert t[..., dv_:].abs().max().item() == 0
        assert res[64][0].view(B * S, H, hd)[..., dv_:].abs().max().item() == 0


@pytest.mark.parametrize("B,H,S,d", [(1, 2, 128, 128), (2, 3, 300, 128), (1, 2, 1024, 128), (2, 2, 231, 64), (1, 4, 640, 64), (1, 2, 333, 96), (2, 2, 512, 96)])
def test_attention_fwd_bwd(ops, B, H, S, d):
    _attn_case(ops, B, H, S, d)


def test_attention_key_bias_and_rescale_branch(ops):
    _attn_case(ops, 1, 2, 320, 128, bias=True)
    _attn_case(ops, 1, 2, 448, 128, spike=True)
    _attn_case(ops, 1, 2, 200, 64, bias=True, spike=True)
    _attn_case(ops, 1, 2, 300, 96, bias=True)


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_sum_chunks_bf16(ops, W):
    """st355_sum_chunks_bf16 (the local half of GradSync's fp32-accumulating reduce-scatter): out[i] = bf16(sum over w, in rank order, of float(chunk_w[i]))
    against float-sum-then-round, bit for bit; chunk lengths from one 8-element vector to a few MiB incl. lengths that leave the last workgroup ragged"""
    torch.manual_seed(55 + W)
    for n in (8, 264, 8 * 1000 + 8, 1 << 20, (1 << 21) + 8 * 37):
        chunks = (torch.randn(W * n, device=dev()) * 3).to(BF16)
        out = torch.empty(n, device=dev(), dtype=BF16)
        ops.sum_chunks_bf16(chunks, W, out)
        acc = torch.zeros(n, device=dev(), dtype=torch.float32)
        for w in range(W):                                              # rank order, fp32 accumulation, ONE rounding
            acc += chunks[w * n:(w + 1) * n].float()
        assert torch.equal(out, acc.to(BF16)), (W, n)


# ------------------------------------------------------------------------------------------------
# optimiser / EMA
# ------------------------------------------------------------------------------------------------
def test_adamw_matches_torch_and_ema(ops):
    torch.manual_seed(40)
    n = 100003
    p0 = torch.randn(n, device=dev())
    p = p0.clone(); m = torch.zeros(n, device=dev()); v = torch.zeros(n, device=dev())
    ema = p0.clone(); pb = torch.empty(n, device=dev(), dtype=BF16)
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ema_ref = p0.clone()
    for step in range(1, 6):
        g = torch.randn(n, device=dev()) * (0.1 * step)
        tp.grad = g.clone()
        opt.step()
        ops.adamw_ema_step(p, g, m, v, step, 1e-3, ema=ema, ema_decay=0.99, p_bf16=pb)
        ema_ref.sub_((1 - 0.99) * (ema_ref - tp.data))
    d = maxabs(p, tp.data)
    print(f"[parity] adamw vs torch.optim.AdamW after 5 steps: max_abs={d:.3e}")
    # |p| ~ 4 -> fp32 ulp 4.8e-7; torch's foreach/fused kernels order the same ops differently: allow 8 ulp
    assert d < 4e-6
    assert maxabs(ema, ema_ref) < 4e-6
    assert torch.equal(pb, p.to(BF16))


def test_adamw_bf16_arena(ops):
    torch.manual_seed(41)
    n = 8 * 4099
    p0 = torch.randn(n, device=dev()).to(BF16)
    p = p0.clone(); m = torch.zeros(n, device=dev()); v = torch.zeros(n, device=dev()); ema = p0.clone()
    pr = p0.float(); mr = torch.zeros(n, device=dev()); vr = torch.zeros(n, device=dev())
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    for step in range(1, 4):
        g = (torch.randn(n, device=dev()) * 0.1).to(BF16)
        ops.adamw_ema_step(p, g, m, v, step, lr, ema=ema, ema_decay=0.9)
        gf = g.float()
        pr = pr * (1 - lr * wd)
        mr = mr + (gf - mr) * (1 - b1)
        vr = vr * b2 + (1 - b2) * gf * gf
        pr = pr - (lr / (1 - b1 ** step)) * (mr / (vr.sqrt() / math.sqrt(1 - b2 ** step) + eps))
        pr = pr.to(BF16).float()
    assert report("adamw bf16 arena", p, pr)[1] < 2e-2
    assert maxabs(m, mr) < 1e-6


def test_ema_update_and_grad_norm(ops):
    torch.manual_seed(42)
    s = torch.randn(1000, device=dev()); p = torch.randn(1000, device=dev())
    ref = s - (1 - 0.999) * (s - p)
    ops.ema_update(s, p, 0.999)
    assert maxabs(s, ref) < 1e-6                      # tests/test_ema.py:39-105 tolerance (atol 1e-6)
    g = torch.randn(12345, device=dev())
    out = ops.grad_norm(g)
    assert abs(out[0].item() - (g * g).sum().item()) < 1e-3 * (g * g).sum().item()
    assert out[1].item() == g.abs().max().item()


# ------------------------------------------------------------------------------------------------
# deep-pipelined GEMM schedule (k_gemm_p3: 3-stage LDS-DMA ring, counted vmcnt) + grouped launches
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(4608, 3072, 64), (4608, 3072, 128), (4608, 3072, 192), (2000, 2200, 320), (4608, 9216, 3072),
                                   (18432, 3072, 3072), (4100, 3076, 1024)])
def test_gemm_p3_shapes_and_race_screen(ops, M, N, K):
    torch.manual_seed(50)
    a = torch.randn(M, K, device=dev()).to(BF16)
    w = (torch.randn(N, K, device=dev()) * 0.05).to(BF16)
    out = ops.gemm(a, w)
    ref = a.float() @ w.float().t()
    assert report(f"gemm(p3) {M}x{N}x{K}", out, ref)[0] < 5e-3
    # race screen: the schedule keeps LDS-DMA in flight across barriers; a misplaced wait shows up as run-to-run differences
    for _ in range(10):
        assert torch.equal(ops.gemm(a, w), out)


def test_gemm_p3_lora_extension_and_epilogues(ops):
    torch.manual_seed(51)
    M, N, K, K2 = 4608, 3072, 1024, 128
    x = torch.randn(M, K, device=dev()).to(BF16)
    W = (torch.randn(N, K, device=dev()) * 0.05).to(BF16)
    t = torch.randn(M, K2, device=dev()).to(BF16)
    b2 = (torch.randn(N, K2, device=dev()) * 0.05).to(BF16)
    bias = torch.randn(N, device=dev()).to(BF16)
    resid = torch.randn(M, N, device=dev()).to(BF16)
    gate = torch.randn(2, N, device=dev()).to(BF16)
    out = ops.gemm(x, W, bias=bias, a2=t, b2=b2, epilogue=ops.EPI_GATE_RESIDUAL, aux_in=resid, gate=gate, rows_per_batch=M // 2)
    core = x.float() @ W.float().t() + t.float() @ b2.float().t() + bias.float()
    ref = resid.float() + gate.float().repeat_interleave(M // 2, dim=0) * core
    assert report("gemm(p3) K-ext + gate/residual", out, ref)[0] < 5e-3
    out2 = ops.gemm(x, W, epilogue=ops.EPI_ADD, aux_in=resid)
    assert report("gemm(p3) add", out2, x.float() @ W.float().t() + resid.float())[0] < 5e-3


def test_gemm_grouped_two_streams(ops):
    """img (4096 rows) + txt (512 rows) projections of an MMDiT block in one launch, different weights / outputs"""
    torch.manual_seed(52)
    D = 1024
    xi = torch.randn(4096, D, device=dev()).to(BF16); xt = torch.randn(512, D, device=dev()).to(BF16)
    Wi = (torch.randn(3 * D, D, device=dev()) * 0.03).to(BF16); Wt = (torch.randn(3 * D, D, device=dev()) * 0.03).to(BF16)
    bi = torch.randn(3 * D, device=dev()).to(BF16); bt = torch.randn(3 * D, device=dev()).to(BF16)
    joint = torch.zeros(4608, 3 * D, device=dev(), dtype=BF16)
    outs = ops.gemm_grouped([dict(a=xi, w=Wi, bias=bi, out=joint[512:]), dict(a=xt, w=Wt, bias=bt, out=joint[:512])])
    assert report("grouped img", joint[512:], xi.float() @ Wi.float().t() + bi.float())[0] < 5e-3
    assert report("grouped txt", joint[:512], xt.float() @ Wt.float().t() + bt.float())[0] < 5e-3
    assert outs[0].data_ptr() == joint[512:].data_ptr()
    # three problems (odd count) incl. a tiny one, GELU epilogue with pre-activation store
    pre = [torch.empty(r, D, device=dev(), dtype=BF16) for r in (4096, 512, 40)]
    xs = [xi, xt, xt[:40]]
    W1 = (torch.randn(D, D, device=dev()) * 0.03).to(BF16)
    outs = ops.gemm_grouped([dict(a=x_, w=W1, epilogue=ops.EPI_GELU, aux_out=p_) for x_, p_ in zip(xs, pre)])
    for x_, p_, o_ in zip(xs, pre, outs):
        assert rel(p_, x_.float() @ W1.float().t()) < 5e-3
        assert rel(o_, gelu_tanh(p_.float())) < 5e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_clamp_value_clipping(ops, dtype):
    """clip_grad_value_ (trainer.py:7209-7213): in-place clamp of the flat gradient arena"""
    torch.manual_seed(31)
    g = (torch.randn(100003, device=dev()) * 3).to(dtype)
    ref = g.clone().clamp_(-1.5, 1.5)
    ops.grad_clamp_(g, 1.5)
    assert torch.equal(g, ref)

"""Plain torch restatement of the numerics of csrc/attention_sage.hip (include/st355.h states them): the quantisers in fp32 exactly as the kernels order them
(bit for bit), everything after the quantisers in fp64.  CPU tensors in, CPU tensors out.

The bound of the main kernel against `attention(dequantised operands)` (used by tests/test_attn_sage_gpu.py), u = 2^-24.  For one query row let
p_k = exp2(s2_k - m) with m the row maximum, so max_k p_k = 1 and l = sum_k p_k >= 1, and O_c = sum_k p_k v_kc / l.  The kernel differs by
  * e_k = exp2(fma(int, f, -(m - 8))) in fp32: f = fl(fl(sq sk) c) carries 5 u relative (two products, c = fl(scale log2 e) from fp32 factors), the fma
    rounds u (|s2| + |m| + 8) absolutely, v_exp_f32 is good to 1 ulp (2 u): relative error of e_k <= eps_e = u (5 S2 + 8) with S2 = max_k |s2_k| of the row
    (ln 2 (5 S2 + 2 S2 + 8) + 2 <= 5 S2 + 8);
  * the e4m3 rounding of e_k = p_k 2^8: relative <= 2^-4 where e_k >= 2^-6 (normal: 3 mantissa bits, half an ulp), absolute <= 2^-10 below (half the
    subnormal step 2^-9), i.e. 2^-18 in units of p;
  * l accumulated in fp32 from the unquantised e_k: at most S + 2 steps + 4 additions / rescalings, relative <= eps_l = eps_e + u (2 S + 8);
  * the products e4m3 x e4m3 are exact in fp32 and accumulate in fp32 with the per-step rescaling: relative to sum_k p_k |v_kc| <= eps_acc = 2 u (2 S + 8).
Hence |num~ - num| <= l vmax_c (2^-4 + eps_e + eps_acc) + S 2^-18 vmax_c with vmax_c = max_k |v_kc|, and dividing by l~ = l (1 + eps), |eps| <= eps_l,
with |num / l| <= vmax_c and l >= 1:
  |dO_c| <= vmax_c (2^-4 + 2 eps_e + eps_acc + 3 eps_l + S 2^-18) =: b_c          (products of the small terms are covered by the doubled eps_e and eps_l)
The two fp32 operations of the epilogue (acc sv, / l) add 2 u |O_c|, inside the slack of 3 eps_l >= 24 u.  Rounding to bf16 adds half an ulp of the
kernel's value, <= 2^-9 (|O_c| + b_c).  Nothing here is fitted to what the kernel returns."""
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
LOG2E = 1.4426950408889634


def _blocks(x, S, Sp):
    """[B, H, S, d] fp32 -> ([B, H, Sp/64, 64, d] zero-padded, the mask of rows < S in that shape)"""
    B, H, _, d = x.shape
    valid = (torch.arange(Sp) < S).view(1, 1, Sp // 64, 64, 1)
    return F.pad(x, (0, 0, 0, Sp - S)).view(B, H, Sp // 64, 64, d), valid


def k_mean(K, S, Sp):
    """fp32, fixed order: the 64 rows of a block in row order, the blocks in block order, one division by S"""
    kb, _ = _blocks(K.float(), S, Sp)
    part = torch.zeros_like(kb[:, :, :, 0])
    for r in range(64):
        part = part + kb[:, :, :, r]
    tot = torch.zeros_like(part[:, :, 0])
    for blk in range(Sp // 64):
        tot = tot + part[:, :, blk]
    return tot / torch.tensor(float(S), dtype=F32)


def _int8_rows(x, S, Sp):
    xb, valid = _blocks(x, S, Sp)
    amax = torch.where(valid, xb.abs(), 0.0).amax((3, 4))
    s = torch.where(amax > 0, amax / 127.0, 1.0)
    q = torch.where(valid, torch.round(xb / s[..., None, None]), 0.0).to(torch.int8)
    return q.view(x.shape[0], x.shape[1], Sp, x.shape[3]), s


def quantize(Q, K, Vt, S, smooth=True):
    """bf16 Q, K [B, H, S, d], Vt [B, H, d, Sp] -> (Qh, Kh int8 [B,H,Sp,d], Vh e4m3 [B,H,d,Sp], sq, sk [B,H,Sp/64], sv [B,H,d]); smooth=False keeps K's mean"""
    Sp = Vt.shape[-1]
    kbar = k_mean(K, S, Sp) if smooth else torch.zeros(K.shape[0], K.shape[1], K.shape[3])
    Qh, sq = _int8_rows(Q.float(), S, Sp)
    Kh, sk = _int8_rows(K.float() - kbar[:, :, None, :], S, Sp)
    valid = torch.arange(Sp) < S
    V = Vt.float()
    amax = torch.where(valid, V.abs(), 0.0).amax(-1)
    sv = torch.where(amax > 0, amax / 448.0, 1.0)
    Vh = torch.where(valid, (V / sv[..., None]).clamp(-448.0, 448.0), 0.0).to(torch.float8_e4m3fn)
    return Qh, Kh, Vh, sq, sk, sv


def dequantize(Qh, Kh, Vh, sq, sk, sv, S):
    """fp64 (q, k, v) [B, H, S, d] from the quantised operands"""
    rows = lambda xh, s: (xh.double() * s.double().repeat_interleave(64, dim=2)[..., None])[:, :, :S]
    return rows(Qh, sq), rows(Kh, sk), (Vh.float().double() * sv.double()[..., None])[..., :S].transpose(2, 3)


def attention(q, k, v, scale):
    """exact fp64 attention, [B, H, S, d] operands of any float dtype -> (O [B, H, S, d], max_k |scale log2e q.k| per row [B, H, S, 1])"""
    s2 = q.double() @ k.double().transpose(2, 3) * (scale * LOG2E)
    return torch.softmax(s2 * (1.0 / LOG2E), -1) @ v.double(), s2.abs().amax(-1, keepdim=True)


def sage(Q, K, Vt, S, scale, smooth=True):
    """the whole algorithm in fp64 after the quantisers, the e4m3 rounding of p 2^8 included -> O [B, H, S, d] fp64"""
    q, k, v = dequantize(*quantize(Q, K, Vt, S, smooth), S)
    s2 = q @ k.transpose(2, 3) * (scale * LOG2E)
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    ph = (p * 256.0).float().to(torch.float8_e4m3fn).float().double()
    return ph @ v / (256.0 * p.sum(-1, keepdim=True))


def bound(O_ref, S2, v, S):
    """the docstring's element-wise bound [B, H, S, d] from the reference O, the rows' score maxima S2 and the dequantised v"""
    u = 2.0 ** -24
    eps_e = u * (5.0 * S2 + 8.0)
    eps_acc = 2.0 * u * (2 * S + 8)
    eps_l = eps_e + u * (2 * S + 8)
    b = v.abs().amax(2, keepdim=True) * (2.0 ** -4 + 2.0 * eps_e + eps_acc + 3.0 * eps_l + S * 2.0 ** -18)
    return b + 2.0 ** -9 * (O_ref.abs() + b)

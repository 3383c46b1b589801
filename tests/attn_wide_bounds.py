"""The one term tests/attn_bounds.py lacks for the wide-head backward (csrc/attention_wide.hip): delta taken from sum_j P_ij dP_ij instead of rowsum(dO o O).

attn_bwd_model is given the fp64 forward O, so its delta is D_i = dO_i . O_i exactly (its own e_delta, u (d + 4) sum|dO O|, models a dot product this route never
forms; it stays, unloosened).  The kernel's delta is  fl( sum_j P32_ij dP32_ij )  with
  P32_ij  = P_ij (1 + eps_ij),  eps_ij <= ln2 ea_ij + 2^-22      the same recomputed exponential as in dS (attn_bounds._arg_err with m = the stored lse2; NOT rounded
                                                                 to bf16: delta is summed from the fp32 values),
  dP32_ij = dP_ij + e_dp_ij,    e_dp_ij <= u (d + 2) sum_c |dO_ic v_jc|          the fp32 MFMA chain,
  the fp32 products and the sum over the Sk keys (a per-lane chain over the tiles, then the two half-waves): u (Sk + 8) sum_j |P_ij dP_ij|  (+ 2u per product).
P comes from the STORED lse2, whose distance from the fp64 lse2 the forward check bounds by t_i = e_lse2_i + u |lse2_i|; the exact sum_j P_ij dP_ij is then
2^(+-t_i) D_i, i.e. off D_i by at most ln2 t_i |D_i| (first order; t ~ 1e-5).  Together
  e_i = ln2 t_i |D_i| + sum_j |P_ij dP_ij| (eps_ij + 2u) + sum_j P_ij e_dp_ij + u (Sk + 8) sum_j |P_ij dP_ij|.
It enters dS_ij = P_ij (dP_ij - delta_i) as P_ij e_i and passes the bf16 rounding of dS (x (1 + 2^-8)), so
  e_dQ_ic += scale (1 + 2^-8) e_i sum_j P_ij |k_jc|,      e_dK_jc += scale (1 + 2^-8) sum_i P_ij e_i |q_ic|.
Variances, with the error of delta_i uniform in +-e_i (the module's convention): it is COMMON to the keys of row i, so dQ_i moves by scale err_i sum_j P_ij k_jc
(var scale^2 e_i^2 / 3 (sum_j P_ij k_jc)^2), and independent across the rows that add up in dK (var scale^2 sum_i (P_ij e_i)^2 / 3 q_ic^2)."""
import math

import torch

from tests import attn_bounds as AB


def add_delta_sum_terms(bw, q, k, v, dO, O, lse2, e_lse2, scale):
    """bw: AB.attn_bwd_model(q, k, v, dO, O, lse2, scale) with O the fp64 forward output; lse2: the kernel's; e_lse2: the forward model's.  Adds the terms above in place."""
    f = lambda x: x.to(AB.F64)
    B, H, Sq, d = q.shape
    Sk = k.shape[2]
    for b in range(B):
        for h in range(H):
            qq, kk, vv, gg = f(q[b, h]), f(k[b, h]), f(v[b, h]), f(dO[b, h])
            L2 = f(lse2[b, h])[:, None]
            s, mag2, _ = AB._scores(qq, kk, None, scale)
            s2 = s * AB.LOG2E
            p = torch.exp2(s2 - L2)
            eps = math.log(2.0) * AB._arg_err(d, mag2, s2, None, L2) + AB.EXP_REL
            pdp = (p * (gg @ vv.t())).abs()
            e_dp = AB.U24 * (d + 2) * (gg.abs() @ vv.abs().t())
            D = (gg * f(O[b, h])).sum(-1, keepdim=True)
            t = f(e_lse2[b, h])[:, None] + AB.U24 * L2.abs()
            e = (math.log(2.0) * t * D.abs() + (pdp * (eps + 2 * AB.U24)).sum(-1, keepdim=True) + (p * e_dp).sum(-1, keepdim=True)
                 + AB.U24 * (Sk + 8) * pdp.sum(-1, keepdim=True))
            pe = p * e
            bw.e_dQ[b, h] += scale * (1 + AB.BF16_REL) * (pe @ kk.abs())
            bw.e_dK[b, h] += scale * (1 + AB.BF16_REL) * (pe.t() @ qq.abs())
            bw.var_dQ[b, h] += scale * scale * (e * (p @ kk)) ** 2 / 3
            bw.var_dK[b, h] += scale * scale * ((pe * pe).t() @ (qq * qq)) / 3
    return bw

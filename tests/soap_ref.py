"""SOAP restated in fp64 (optimizers/soap/__init__.py, 2-D parameters) and a CPU stand-in for the SOAP wrappers of `simpletuner_amd.ops`.

TEST INFRASTRUCTURE ONLY.  `SoapRef` is the yardstick the golden fixture (tests/golden/soap_vectors.pt, the reference's own SOAP executed by
tools/gen_soap_golden.py) and the HIP kernels are held to: every product, the eigendecomposition and the QR in float64.  It follows the class
call by call: the first call only builds GG and Q = flip(eigh(GG)); afterwards exp_avg stays in the original basis, exp_avg_sq lives in the
rotated one, the weight decay comes after the update, GG is updated after the step and, when step % precondition_frequency == 0, the basis
is re-sorted by diag(Q^T GG Q) and re-orthogonalised by one power iteration + QR.  A side longer than max_precond_dim is left as identity
(`[]` in the GG / Q lists).  `store=torch.float32` rounds at the points where the reference materialises a tensor of the parameter dtype (as
tests/muon_ref.py does for bf16): that is how its fp32 runs are restated — every operation exact, then stored as the class stores it.
`install(monkeypatch)` replaces ops.SoapPlan / ops.soap_step / ops.soap_eigh with plain-torch fp32 functions
honouring the same contracts, so St355Soap's host logic and the trainer run with `-m "not gpu"`; the GPU tests are the proof for the kernels.
"""
from __future__ import annotations

import torch

F64 = torch.float64
F32 = torch.float32


def _eigh_desc(a):
    """eigenvectors by descending eigenvalue: flip(eigh(.)) of :385-389"""
    _, q = torch.linalg.eigh(a)
    return torch.flip(q, [1])


def _stable_desc(x):
    return torch.sort(x, descending=True, stable=True).indices


class SoapRef:
    """the reference's per-parameter state and step for ONE 2-D matrix, in `dtype` (float64 unless told otherwise)"""

    def __init__(self, p, lr=3e-3, betas=(0.95, 0.95), shampoo_beta=-1, eps=1e-8, weight_decay=0.01, precondition_frequency=10,
                 max_precond_dim=10000, correct_bias=True, dtype=F64, store=None, **_unused):
        self.dt = dtype
        self.rnd = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
        self.p = p.detach().to(dtype).clone()
        self.lr, self.betas, self.eps, self.wd, self.freq, self.correct_bias = lr, betas, eps, weight_decay, int(precondition_frequency), correct_bias
        self.sb = shampoo_beta if shampoo_beta >= 0 else betas[1]
        self.step = 0
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.GG = [torch.zeros(sh, sh, dtype=dtype) if sh <= max_precond_dim else None for sh in self.p.shape]
        self.Q = None

    # ---- the class's pieces ----
    def project(self, x):
        if self.Q[0] is not None:
            x = self.rnd(self.Q[0].T @ x)
        if self.Q[1] is not None:
            x = self.rnd(x @ self.Q[1])
        return x

    def project_back(self, x):
        if self.Q[0] is not None:
            x = self.rnd(self.Q[0] @ x)
        if self.Q[1] is not None:
            x = self.rnd(x @ self.Q[1].T)
        return x

    def _update_preconditioner(self, g):
        w = 1.0 - self.sb
        if self.GG[0] is not None:
            self.GG[0] = self.rnd(self.GG[0] + w * (self.rnd(g @ g.T) - self.GG[0]))
        if self.GG[1] is not None:
            self.GG[1] = self.rnd(self.GG[1] + w * (self.rnd(g.T @ g) - self.GG[1]))
        if self.Q is None:
            self.Q = [None if a is None else self.rnd(_eigh_desc(a)) for a in self.GG]
        if self.step > 0 and self.step % self.freq == 0:
            for side in (0, 1):
                a, o = self.GG[side], self.Q[side]
                if a is None:
                    continue
                idx = _stable_desc(torch.diag(o.T @ a @ o))
                self.v = self.v.index_select(side, idx)
                self.Q[side] = self.rnd(torch.linalg.qr(self.rnd(a @ o[:, idx])).Q)

    def call(self, grad, grad_scale=1.0):
        g = self.rnd(grad.to(self.dt) * grad_scale)
        if self.Q is None:                               # the first call is skipped (:138-155)
            self._update_preconditioner(g)
            return self.p
        b1, b2 = self.betas
        gp = self.project(g)
        self.step += 1
        self.m = self.rnd(self.rnd(b1 * self.m) + (1.0 - b1) * g)                  # exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
        self.v = self.rnd(self.rnd(b2 * self.v) + (1.0 - b2) * self.rnd(gp * gp))
        denom = self.rnd(self.rnd(self.v.sqrt()) + self.eps)
        mp = self.project(self.m)
        step_size = self.lr
        if self.correct_bias:
            step_size = step_size * ((1.0 - b2 ** self.step) ** 0.5) / (1.0 - b1 ** self.step)
        self.p = self.rnd(self.p - step_size * self.project_back(self.rnd(mp / denom)))
        if self.wd > 0.0:
            self.p = self.rnd(self.p - self.lr * self.wd * self.p)
        self._update_preconditioner(g)
        return self.p

    def load_reference_state(self, sd):
        """one parameter's entry of the reference's state_dict()["state"]"""
        self.step = int(sd["step"])
        self.m, self.v = sd["exp_avg"].to(self.dt).clone(), sd["exp_avg_sq"].to(self.dt).clone()
        self.GG = [a.to(self.dt).clone() if torch.is_tensor(a) else None for a in sd["GG"]]
        self.Q = None if sd["Q"] is None else [a.to(self.dt).clone() if torch.is_tensor(a) else None for a in sd["Q"]]
        self.freq, self.sb = int(sd["precondition_frequency"]), float(sd["shampoo_beta"])


def run_fp64(p0, grads, settings, start_state=None, first_call=0, store=None):
    """the trajectory of a list of matrices under the restatement: grads[k][i] is matrix i's gradient of call k; returns [per call [per matrix p]]"""
    refs = [SoapRef(p, store=store, **settings) for p in p0]
    if start_state is not None:
        for i, rf in enumerate(refs):
            rf.load_reference_state(start_state[i])
    out = []
    for k in range(first_call, len(grads)):
        out.append([rf.call(g).clone() for rf, g in zip(refs, grads[k])])
    return out


# ---- one kernel step from the kernel's own state, in fp64 (tests/test_soap_gpu.py) ----------------------------------------------------------------
def one_step_fp64(p, g, m, v, Q, GG, wide, c):
    """p, g, m, v in the matrix's own orientation, Q, GG r x r; c: the fp32 scalars that cross the ABI (tests/soap_bounds.py:consts).  Returns the fp64
    results and the intermediates the bound needs, all in the r x L orientation"""
    t = (lambda x: x.to(F64)) if wide else (lambda x: x.to(F64).T)
    p, g, m, v, Q, GG = t(p), t(g), t(m), t(v), Q.to(F64), GG.to(F64)
    g1 = g * c["gs"]
    m1 = c["b1"] * m + c["omb1"] * g1
    gp = Q.T @ g1
    v1 = c["b2"] * v + c["omb2"] * gp * gp
    mp = Q.T @ m1
    d = v1.sqrt() + c["eps"]
    w = mp / d
    u = Q @ w
    p1 = p - c["step"] * u
    p2 = p1 - c["lrwd"] * p1 if c["lrwd"] > 0 else p1
    S = g1 @ g1.T
    GG1 = GG + c["w"] * (S - GG) if c["w"] < 0.5 else S - (S - GG) * (1.0 - c["w"])
    return dict(g1=g1, m1=m1, gp=gp, v1=v1, mp=mp, d=d, w=w, u=u, p1=p1, p2=p2, S=S, GG1=GG1, p=p, m=m, v=v, Q=Q, GG=GG)


# ---- CPU stand-in for the st355_soap_* wrappers -------------------------------------------------------------------------------------------------
class SoapPlanCPU:
    def __init__(self, offsets, shapes, device):
        for s in shapes:
            if min(s) > 128:
                raise RuntimeError("soap_plan: short side above 128")
        self.n = len(shapes)
        self.mats = [(int(o), int(s[0]), int(s[1])) for o, s in zip(offsets, shapes)]
        self.short = [min(r, c) for _, r, c in self.mats]
        self.q_offsets, self.r_offsets, qq, rr = [], [], 0, 0
        for r in self.short:
            self.q_offsets.append(qq)
            self.r_offsets.append(rr)
            qq += r * r
            rr += r
        self.qq, self.rr = qq, rr
        self._idx = [torch.arange(r, dtype=torch.int32) for r in self.short]

    def launches(self, first=False, refresh=False):
        ncls = len({(r + 31) // 32 for r in self.short})
        return ncls + 1 + (1 if first else (1 + ncls if refresh else 0))

    def sort_index(self, i):
        return self._idx[i]


def soap_step_cpu(plan, p, g, m, v, gg, q, step_size, beta1, beta2, eps, lr_weight_decay, gg_weight, first, refresh, grad_scale=1.0):
    for i, (off, rows, cols) in enumerate(plan.mats):
        n, r, qo = rows * cols, plan.short[i], plan.q_offsets[i]
        wide = rows < cols
        t = (lambda x: x) if wide else (lambda x: x.T)
        pv, gv, mv, vv = (x[off:off + n].view(rows, cols) for x in (p, g, m, v))
        G, Q = gg[qo:qo + r * r].view(r, r), q[qo:qo + r * r].view(r, r)
        g1 = t(gv) * grad_scale
        if not first:
            mv.copy_(beta1 * mv + (1.0 - beta1) * gv * grad_scale)
            gp = Q.T @ g1
            t(vv).copy_(beta2 * t(vv) + (1.0 - beta2) * gp * gp)
            u = Q @ ((Q.T @ t(mv)) / (t(vv).sqrt() + eps))
            t(pv).sub_(step_size * u)
            if lr_weight_decay > 0:
                pv.sub_(lr_weight_decay * pv)
        G.lerp_(g1 @ g1.T, gg_weight)
        if first:
            Q.copy_(_eigh_desc(G.double()).float())
        elif refresh:
            idx = _stable_desc(torch.diag(Q.T @ G @ Q))
            plan._idx[i] = idx.to(torch.int32)
            t(vv).copy_(t(vv).index_select(0, idx))
            Q.copy_(torch.linalg.qr(G @ Q[:, idx]).Q)


def soap_eigh_cpu(plan, gg, q=None, evals=None):
    q = torch.zeros_like(gg) if q is None else q
    evals = torch.zeros(plan.rr, dtype=F32) if evals is None else evals
    for r, qo, ro in zip(plan.short, plan.q_offsets, plan.r_offsets):
        lam, vec = torch.linalg.eigh(gg[qo:qo + r * r].view(r, r).double())
        q[qo:qo + r * r].view(r, r).copy_(torch.flip(vec, [1]).float())
        evals[ro:ro + r].copy_(torch.flip(lam, [0]).float())
    return q, evals


def install(monkeypatch):
    from simpletuner_amd import ops
    monkeypatch.setattr(ops, "SoapPlan", SoapPlanCPU)
    monkeypatch.setattr(ops, "soap_step", soap_step_cpu)
    monkeypatch.setattr(ops, "soap_eigh", soap_eigh_cpu)

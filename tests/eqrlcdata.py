"""N proofs of ONE equation for the GPU tests of gs_verify_equation_rlc: genuinely different witnesses of the same
public equation (A, B, Gamma, target), and rerandomizations of their proofs (gs_rerandomize_batch: distinct commitments
and proofs of the same statement).  Test plumbing only: group elements, proofs and rerandomizations are made with the
engine's own entry points, which have their own tests against the oracle.

Another witness of the same equation: draw every variable afresh, then solve for x_0 -- the equation
sum_j a_j y_j + sum_i x_i b_i + sum_ij x_i g_ij y_j = s is linear in it (the discrete logarithms are known, as in
stmtutil.StatementInputs)."""
import numpy as np

import forge
from stmtutil import StatementInputs

CONST = ("A", "B", "G", "target")
PROOF = ("xcoms", "ycoms", "pi", "theta")


class Batch:
    """const: dict A[n], B[m], G[m][n], target[1]; proofs: list of dict xcoms, ycoms, pi, theta (uint8 arrays)"""

    def __init__(self, cname, cid, ty, m, n, crs, const, proofs, witnesses):
        self.cname, self.cid, self.ty, self.m, self.n, self.crs = cname, cid, ty, m, n, crs
        self.const, self.proofs, self.witnesses = const, proofs, witnesses
        self.N = len(proofs)


def make_batch(cname, cid, ty, N, m, n, seed=8100, witnesses=3):
    """`witnesses` (at most N) different witnesses proven directly; the other proofs are rerandomizations of those, in
    turn (proof e >= W rerandomizes proof e % W)."""
    import groth_sahai_rs_amd as gs

    eng = gs.Engine(cid, 0)
    try:
        st = StatementInputs(eng, mg=m, ng=n, ms=m, ns=n, seed=seed)
        eng.set_crs(st.crs)
        r = st.r
        xg, yg = ty in (0, 1), ty in (0, 2)
        kx, ky = (2 if xg else 1), (2 if yg else 1)
        a, b, gam = st.scalars(n), st.scalars(m), st.scalars(m * n)
        value = lambda x, y: (sum(a[j] * y[j] for j in range(n)) + sum(x[i] * b[i] for i in range(m)) +
                              sum(x[i] * gam[i * n + j] % r * y[j] for i in range(m) for j in range(n))) % r
        W = max(1, min(witnesses, N))
        xs, ys = [st.scalars(m)], [st.scalars(n)]
        s = value(xs[0], ys[0])
        while len(xs) < W:
            x, y = st.scalars(m), st.scalars(n)
            k0 = (b[0] + sum(gam[j] * y[j] for j in range(n))) % r
            if k0 == 0:
                continue
            x[0] = 0
            x[0] = (s - value(x, y)) * pow(k0, -1, r) % r
            assert value(x, y) == s
            xs.append(x)
            ys.append(y)
        A = st.g(1, a) if xg else st.fr(a)
        B = st.g(2, b) if yg else st.fr(b)
        G = st.fr(gam)
        if ty == 0:
            import torch

            out = torch.empty(eng.GT, dtype=torch.uint8, device="cuda:0")
            eng.gt_pow_batch_dev(1, torch.from_numpy(st.gt.copy()).to("cuda:0"),
                                 torch.from_numpy(st.fr([s]).copy()).to("cuda:0"), out)
            eng.sync()
            target = out.cpu().numpy()
        else:
            target = st.g(1, [s]) if ty == 1 else st.g(2, [s]) if ty == 2 else st.fr([s])
        const = dict(A=forge.u8(A), B=forge.u8(B), G=forge.u8(G), target=forge.u8(target))
        rep = lambda arr, cnt: np.concatenate([forge.u8(arr)] * cnt)
        flat = lambda vals: [v for row in vals for v in row]
        X = st.g(1, flat(xs)) if xg else st.fr(flat(xs))
        Y = st.g(2, flat(ys)) if yg else st.fr(flat(ys))
        out = eng.prove_batch(ty, W, m, n, X, Y, rep(A, W), rep(B, W), rep(G, W), st.fr(st.scalars(W * m * kx)),
                              st.fr(st.scalars(W * n * ky)), st.fr(st.scalars(W * ky * kx)))
        per = dict(xcoms=m * eng.COM1, ycoms=n * eng.COM2, pi=kx * eng.COM2, theta=ky * eng.COM1)
        cut = lambda o, e: {k: forge.u8(o[k]).reshape(-1)[e * per[k]:(e + 1) * per[k]].copy() for k in PROOF}
        proofs = [cut(out, e) for e in range(W)]
        M = N - W
        if M > 0:
            src = [proofs[e % W] for e in range(M)]
            cat = lambda k: np.concatenate([p[k] for p in src])
            o2 = eng.rerandomize_batch(ty, M, m, n, rep(A, M), rep(B, M), rep(G, M), cat("xcoms"), cat("ycoms"), cat("pi"),
                                       cat("theta"), st.fr(st.scalars(M * m * kx)), st.fr(st.scalars(M * n * ky)),
                                       st.fr(st.scalars(M * ky * kx)))
            proofs += [cut(o2, e) for e in range(M)]
        return Batch(cname, cid, ty, m, n, forge.u8(st.crs), const, proofs, W)
    finally:
        eng.close()

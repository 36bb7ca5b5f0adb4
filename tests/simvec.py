"""The simulator's model: what gs_simulate_* must write, from the formulas of include/gs_amd.h ("simulate"), computed with
the test oracles and never with the library under test.

On the hiding CRS of gs_crs_generate_hiding (scalars a1, a2, t1, t2) W1 = u1 + (O, g1) = t1 u0 and W2 = v1 + (O, g2) =
t2 v0.  With Rc[m][kx], Sc[n][ky] the coordinates of the commitments in u / v and Tf[ky][kx] the free proof scalars:

  c_i = sum_a Rc_ia u_a        d_j = sum_b Sc_jb v_b
  QuadEqu  theta = Tf[0][0] u0, pi = pi' v0,
           pi' = t2 sum_i Rc_i b_i + t1 sum_j a_j Sc_j + sum_ij Rc_i Gamma_ij Sc_j - t t1 t2 - Tf[0][0]
  MSMEG1   pi_k = Tf[0][k] v0, theta = (O, V) + (sum_i e_i Rc_i0 - Tf[0][0]) u0 + (sum_i e_i Rc_i1 - Tf[0][1]) u1,
           e_i = t2 b_i + sum_j Gamma_ij Sc_j, V = sum_j Sc_j A_j - t2 T
  MSMEG2   theta_l = Tf[l][0] u0, pi = (O, V) + (sum_j f_j Sc_j0 - Tf[0][0]) v0 + (sum_j f_j Sc_j1 - Tf[1][0]) v1,
           f_j = t1 a_j + sum_i Rc_i Gamma_ij, V = sum_i Rc_i B_i - t1 T

Two arithmetic back ends share the scalar part (coefficients): `simulate` works on gs_oracle's integers (points are
tuples, None the identity; what O.verify and O.prove take), `simulate_bytes` on boundary bytes through the C oracle
(gs_ref_py), for byte comparisons against the GPU.  Scalars are Python integers mod r throughout."""
import os
import sys

import numpy as np

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402

PPE, MSMEG1, MSMEG2, QUAD = 0, 1, 2, 3


def xg(ty):
    return ty in (PPE, MSMEG1)


def yg(ty):
    return ty in (PPE, MSMEG2)


def kxy(ty):
    return (2 if xg(ty) else 1), (2 if yg(ty) else 1)


def coefficients(ty, r, t1, t2, a, b, G, t, Rc, Sc, Tf):
    """The Fr part of the simulator.  a / b / t: the scalar constants and target where the type has them (else unused).
    Returns (th, pi, vs, nt): th[l] / pi[k] = the coordinates of theta_l / pi_k on (u0, u1) / (v0, v1) as lists (one
    entry: a multiple of u0 / v0 alone), vs = the scalars of V's constants (Sc_j or Rc_i; None without V), nt = the
    scalar of the target in V."""
    m, n = len(Rc), len(Sc)
    if ty == QUAD:
        acc = t2 * sum(Rc[i][0] * b[i] for i in range(m)) + t1 * sum(a[j] * Sc[j][0] for j in range(n))
        acc += sum(Rc[i][0] * G[i][j] * Sc[j][0] for i in range(m) for j in range(n))
        acc -= t * t1 * t2 + Tf[0][0]
        return [[Tf[0][0] % r]], [[acc % r]], None, None
    if ty == MSMEG1:
        e = [(t2 * b[i] + sum(G[i][j] * Sc[j][0] for j in range(n))) % r for i in range(m)]
        th = [(sum(e[i] * Rc[i][k] for i in range(m)) - Tf[0][k]) % r for k in range(2)]
        return [th], [[Tf[0][0] % r], [Tf[0][1] % r]], [Sc[j][0] % r for j in range(n)], (-t2) % r
    if ty == MSMEG2:
        f = [(t1 * a[j] + sum(Rc[i][0] * G[i][j] for i in range(m))) % r for j in range(n)]
        pi = [(sum(f[j] * Sc[j][l] for j in range(n)) - Tf[l][0]) % r for l in range(2)]
        return [[Tf[0][0] % r], [Tf[1][0] % r]], [pi], [Rc[i][0] % r for i in range(m)], (-t1) % r
    raise ValueError("GS_PPE is not simulated")


# ---- integers (gs_oracle) -----------------------------------------------------------------------------------------------
def _lincomb(smul, add, zero, basis, ks):
    acc = zero
    for k, el in zip(ks, basis):
        acc = add(acc, smul(el, k))
    return acc


def simulate(equ, crs, t1, t2, Rc, Sc, Tf):
    """(xc, yc, pi, theta) for equ = dict(type, a, b, gamma, target) in gs_oracle's form.  The caller has O.set_curve."""
    ty, r = equ["type"], O.R
    th, pi, vs, nt = coefficients(ty, r, t1, t2, equ["a"], equ["b"], equ["gamma"], equ["target"], Rc, Sc, Tf)
    l1 = lambda ks: _lincomb(O.com1_smul, O.com1_add, O.COM1_ZERO, crs["u"], ks)
    l2 = lambda ks: _lincomb(O.com2_smul, O.com2_add, O.COM2_ZERO, crs["v"], ks)
    xc = [l1(row) for row in Rc]
    yc = [l2(row) for row in Sc]
    theta = [l1(ks) for ks in th]
    pis = [l2(ks) for ks in pi]
    if ty == MSMEG1:
        V = O.g1_mul(nt, equ["target"])
        for s, A in zip(vs, equ["a"]):
            V = O.g1_add(V, O.g1_mul(s, A))
        theta[0] = O.com1_add(theta[0], O.lin1(V))
    if ty == MSMEG2:
        V = O.g2_mul(nt, equ["target"])
        for s, B in zip(vs, equ["b"]):
            V = O.g2_add(V, O.g2_mul(s, B))
        pis[0] = O.com2_add(pis[0], O.lin2(V))
    return xc, yc, pis, theta


def honest_coordinates(ty, r, t1, t2, a, b, G, xs, ys, R, S, T):
    """(Rc, Sc, Tf) at which the simulator reproduces the honest proof of gs_prove_batch(X, Y, R, S, T) under the hiding
    CRS.  xs / ys: the witness as scalars -- xi_i with X_i = xi_i g1 for a group-valued side, x_i itself for a scalar
    one.  a, b: the scalar constants where the type has them (else unused)."""
    m, n = len(R), len(S)
    kx, ky = kxy(ty)
    Rc = [[(R[i][0] + xs[i] * t1) % r, (R[i][1] - xs[i]) % r] if xg(ty) else [(R[i][0] + xs[i] * t1) % r]
          for i in range(m)]
    Sc = [[(S[j][0] + ys[j] * t2) % r, (S[j][1] - ys[j]) % r] if yg(ty) else [(S[j][0] + ys[j] * t2) % r]
          for j in range(n)]
    if ty == MSMEG1:  # the v0-coordinates of the honest pi_k
        Tf = [[(sum(R[i][k] * (t2 * b[i] + sum(G[i][j] * Sc[j][0] for j in range(n))) for i in range(m)) - T[0][k]) % r
               for k in range(2)]]
    else:  # the u0-coordinates of the honest theta_l (MSMEG2, QuadEqu)
        Tf = [[(t1 * sum(S[j][l] * (a[j] + sum(G[i][j] * xs[i] for i in range(m))) for j in range(n)) + T[l][0]) % r]
              for l in range(ky)]
    return Rc, Sc, Tf


def key_identities(crs, t1, t2):
    """The four checks of gs_set_simulation_key, component by component: (u1 + (O, g1)).c == t1 u0.c, then v with t2."""
    w1 = O.com1_add(crs["u"][1], O.lin1(crs["g1"]))
    w2 = O.com2_add(crs["v"][1], O.lin2(crs["g2"]))
    tu, tv = O.com1_smul(crs["u"][0], t1), O.com2_smul(crs["v"][0], t2)
    return [w1[0] == tu[0], w1[1] == tu[1], w2[0] == tv[0], w2[1] == tv[1]]


def make_hiding_crs(p1, p2, a1, a2, t1, t2):
    """gs_crs_generate_hiding in gs_oracle's form: the binding CRS with the generator taken off u[1].1 / v[1].1."""
    crs = O.make_crs(p1, p2, a1, a2, t1, t2)
    crs["u"][1] = (crs["u"][1][0], O.g1_add(crs["u"][1][1], O.g1_neg(p1)))
    crs["v"][1] = (crs["v"][1][0], O.g2_add(crs["v"][1][1], O.g2_neg(p2)))
    return crs


# ---- boundary bytes (C oracle) ---------------------------------------------------------------------------------------------
class Bytes:
    """Sizes and small arithmetic on boundary bytes of one curve + CRS, through gs_ref_py."""

    def __init__(self, cname, crs):
        import gs_ref_py as ref

        self.ref, self.cname, self.c = ref, cname, curve(cname)
        self.FQ, self.FR, self.G1, self.G2, self.GT, self.CRS = ref.sizes(cname)
        crs = np.ascontiguousarray(crs).view(np.uint8).reshape(-1)
        assert crs.size == self.CRS
        self.U = crs[:4 * self.G1]
        self.V = crs[4 * self.G1:4 * self.G1 + 4 * self.G2]
        self.r = self.c.r

    def fr(self, v):
        return np.ascontiguousarray(self.c.fr(v % self.r)).view(np.uint8)

    def fr_mat(self, M):
        return np.concatenate([self.fr(v) for row in M for v in row])

    def fr_ints(self, a):
        a = np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)
        return [self.c.fr_dec(x) for x in a]

    def lincomb(self, group, rows):
        """one Com per row of `rows`: sum_k row[k] basis[k] over the first len(row) elements of u (group 1) or v"""
        sz = 2 * (self.G1 if group == 1 else self.G2)
        basis = (self.U if group == 1 else self.V)[:len(rows[0]) * sz]
        return self.ref.left_mul(self.cname, group, len(rows), len(rows[0]), self.fr_mat(rows), basis)

    def msm(self, group, scalars, pts):
        sz = self.G1 if group == 1 else self.G2
        acc = np.zeros(sz, np.uint8)
        for k, s in enumerate(scalars):
            acc = self.ref.g_add(self.cname, group, acc, self.ref.g_mul(self.cname, group, pts[k * sz:(k + 1) * sz],
                                                                       self.fr(s)))
        return acc


def simulate_bytes(cname, crs, ty, m, n, t1, t2, A, B, G, target, Rc, Sc, Tf):
    """ONE equation in boundary bytes: A, B, G, target as the verifier takes them (uint8), Rc / Sc / Tf lists of ints.
    Returns dict(xcoms, ycoms, pi, theta) of uint8 arrays."""
    bx = Bytes(cname, crs)
    u8 = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    A, B, G, target = map(u8, (A, B, G, target))
    g = bx.fr_ints(G)
    Gm = [g[i * n:(i + 1) * n] for i in range(m)]
    a = None if xg(ty) else bx.fr_ints(A)
    b = None if yg(ty) else bx.fr_ints(B)
    t = bx.fr_ints(target)[0] if ty == QUAD else None
    th, pi, vs, nt = coefficients(ty, bx.r, t1, t2, a, b, Gm, t, Rc, Sc, Tf)
    out = dict(xcoms=bx.lincomb(1, Rc), ycoms=bx.lincomb(2, Sc), theta=bx.lincomb(1, th), pi=bx.lincomb(2, pi))
    if ty == MSMEG1:
        V = bx.msm(1, vs + [nt], np.concatenate([A, target]))
        out["theta"][bx.G1:2 * bx.G1] = bx.ref.g_add(cname, 1, out["theta"][bx.G1:2 * bx.G1], V)
    if ty == MSMEG2:
        V = bx.msm(2, vs + [nt], np.concatenate([B, target]))
        out["pi"][bx.G2:2 * bx.G2] = bx.ref.g_add(cname, 2, out["pi"][bx.G2:2 * bx.G2], V)
    return out

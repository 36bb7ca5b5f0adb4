"""The statement-batched verifier (gs_verify_statements_rlc) restated on the C oracle (oracle/gs_ref.c through gs_ref_py):
the LITERAL value prod_e prod_cells (lhs / rhs)^rho of a statement, from the per-equation cells the oracle's verifier
compares, and the FOLDED multi-pairing of DESIGN.md 6.5, whose pair count does not depend on the number of equations.
Test plumbing only; nothing here calls the library under test.

One statement: E equations of one type over shared commitments xcoms[m], ycoms[n]; the arrays are what
gs_verify_statement takes (A[E][n], B[E][m], G[E][m][n], target[E], pi[E][kx], theta[E][ky]); rho[E][4] with
rho[e][2a+b] the exponent of cell (a, b)."""
import numpy as np

import forge
from forge import ref

PPE, MSMEG1, MSMEG2, QUAD = 0, 1, 2, 3


def shape(ty):
    xg, yg = forge.xg(ty), forge.yg(ty)
    return xg, yg, (2 if xg else 1), (2 if yg else 1)


def pair_count(ty, m, n):
    """Miller pairs of one folded statement: 2n + 2m + 2kx + 2ky with group constants on the Y side (2 pairs against
    W2 instead of the 2m when B is scalar); MSMEG2 adds the two pairs of its G2 targets against W1."""
    xg, yg, kx, ky = shape(ty)
    return 2 * n + (2 * m if yg else 2) + 2 * kx + 2 * ky + (2 if ty == MSMEG2 else 0)


def gt_one(cname):
    return forge.u8(forge.curve(cname).f12(["1"] + ["0"] * 11))


def equations(cname, ty, m, n, E, st, crs):
    """the E equations of a statement as forge dicts (shared commitments)"""
    cx = forge.Ctx(cname, crs)
    xg, yg, kx, ky = shape(ty)
    sx, sy = (cx.G1 if xg else 32), (cx.G2 if yg else 32)
    stz = {PPE: cx.GT, MSMEG1: cx.G1, MSMEG2: cx.G2, QUAD: 32}[ty]
    cut = lambda a, e, sz: forge.u8(a)[e * sz:(e + 1) * sz]
    return [dict(cname=cname, ty=ty, m=m, n=n, crs=cx.crs, A=cut(st["A"], e, n * sx), B=cut(st["B"], e, m * sy),
                 G=cut(st["G"], e, m * n * 32), target=cut(st["target"], e, stz), xcoms=forge.u8(st["xcoms"]),
                 ycoms=forge.u8(st["ycoms"]), pi=cut(st["pi"], e, kx * 2 * cx.G2), theta=cut(st["theta"], e, ky * 2 * cx.G1))
            for e in range(E)]


def literal(cname, ty, m, n, E, st, rho, crs):
    """(W, T, L, verdicts): W = prod_e prod_c (lhs_c / den_c)^rho_e,c with den = rhs without the PPE target,
    T = prod_e t_e^rho_e,3 (PPE, else one), L = prod_e prod_c (lhs_c / rhs_c)^rho_e,c, the oracle's verdict per equation"""
    c = forge.curve(cname)
    one = gt_one(cname)
    W, T, L, oks = one, one, one, []
    for e, eq in enumerate(equations(cname, ty, m, n, E, st, crs)):
        ok, lhs, rhs, rhs_nt = forge.oracle_cells(eq, eq)
        oks.append(ok)
        for k in range(4):
            ex = forge.u8(c.fr(int(rho[e][k])))
            for den, into in ((rhs_nt if ty == PPE else rhs, "W"), (rhs, "L")):
                if (lhs[k] != den[k]).any():
                    q = ref.gt_pow(cname, ref.gt_mul(cname, lhs[k], ref.gt_inv(cname, den[k])), ex)
                    if into == "W":
                        W = ref.gt_mul(cname, W, q)
                    else:
                        L = ref.gt_mul(cname, L, q)
        if ty == PPE:
            T = ref.gt_mul(cname, T, ref.gt_pow(cname, eq["target"], forge.u8(c.fr(int(rho[e][3])))))
    return W, T, L, oks


def folded_pairs(cname, ty, m, n, E, st, rho, crs):
    """[(P, Q)]: the pairs of the folded check, prod e(P, Q) = W of literal()"""
    cx = forge.Ctx(cname, crs)
    r = cx.r
    xg, yg, kx, ky = shape(ty)
    G1, G2 = cx.G1, cx.G2
    rho = [[int(v) for v in row] for row in rho]
    R = lambda e, a, b: rho[e][2 * a + b]
    pt = lambda arr, i, sz: forge.u8(arr)[i * sz:(i + 1) * sz]
    ints = lambda arr: cx.fr_ints(forge.u8(arr))

    def msm(group, terms):
        acc = np.zeros(cx.size(group), np.uint8)  # the identity
        for k, p in terms:
            acc = cx.add(group, acc, cx.mul(group, p, k % r))
        return acc

    W1 = [cx.u[1][:G1], cx.add(1, cx.u[1][G1:], cx.g1)]
    W2 = [cx.v[1][:G2], cx.add(2, cx.v[1][G2:], cx.g2)]
    cc = lambda i, a: pt(st["xcoms"], 2 * i + a, G1)
    dd = lambda j, b: pt(st["ycoms"], 2 * j + b, G2)
    gam = ints(st["G"])
    Gm = lambda e, i, j: gam[(e * m + i) * n + j]
    a_s = None if xg else ints(st["A"])
    b_s = None if yg else ints(st["B"])
    t_s = ints(st["target"]) if ty == QUAD else None
    pairs = []
    # 1. (j, b): the constants' images and the Gamma term, folded into G1
    for j in range(n):
        for b in range(2):
            terms = []
            for e in range(E):
                if xg:
                    terms.append((R(e, 1, b), pt(st["A"], e * n + j, G1)))  # iota1(A) = (O, A)
                else:
                    terms += [(R(e, a, b) * a_s[e * n + j], W1[a]) for a in range(2)]
            for i in range(m):
                for a in range(2):
                    terms.append((sum(R(e, a, b) * Gm(e, i, j) for e in range(E)), cc(i, a)))
            pairs.append((msm(1, terms), dd(j, b)))
    # 2. the commitments against the other side's constants
    if yg:
        for i in range(m):
            for a in range(2):
                pairs.append((cc(i, a), msm(2, [(R(e, a, 1), pt(st["B"], e * m + i, G2)) for e in range(E)])))
    else:
        for b in range(2):
            terms = [(sum(R(e, a, b) * b_s[e * m + i] for e in range(E)), cc(i, a)) for i in range(m) for a in range(2)]
            if ty == MSMEG1:  # 5. G1 targets join the W2 pairs
                terms += [(-R(e, 1, b), pt(st["target"], e, G1)) for e in range(E)]
            if ty == QUAD:    # 5. scalar targets as fixed-base scalars
                terms += [(-sum(R(e, a, b) * t_s[e] for e in range(E)), W1[a]) for a in range(2)]
            pairs.append((msm(1, terms), W2[b]))
    # 3. (k, a): -u_k.a against the folded pi
    for k in range(kx):
        for a in range(2):
            q = msm(2, [(R(e, a, b), pt(st["pi"], 2 * (e * kx + k) + b, G2)) for e in range(E) for b in range(2)])
            pairs.append((cx.neg(1, pt(cx.u[k], a, G1)), q))
    # 4. (l, b): the folded theta, negated, against v_l.b
    for l in range(ky):
        for b in range(2):
            p = msm(1, [(-R(e, a, b), pt(st["theta"], 2 * (e * ky + l) + a, G1)) for e in range(E) for a in range(2)])
            pairs.append((p, pt(cx.v[l], b, G2)))
    # 5. G2 targets against W1
    if ty == MSMEG2:
        for a in range(2):
            pairs.append((cx.neg(1, W1[a]), msm(2, [(R(e, a, 1), pt(st["target"], e, G2)) for e in range(E)])))
    return pairs


def folded_value(cname, pairs):
    return ref.multi_pairing(cname, len(pairs), np.concatenate([p for p, _ in pairs]), np.concatenate([q for _, q in pairs]))

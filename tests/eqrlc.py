"""The batched verifier for N proofs of ONE equation (gs_verify_equation_rlc) restated on the C oracle (oracle/gs_ref.c
through gs_ref_py): the LITERAL value prod_e prod_cells (lhs / rhs')^rho of the batch, from the per-proof cells the
oracle's verifier compares, and the FOLDED multi-pairing of DESIGN.md 6.7, in which only the Gamma term is paired per
proof.  Test plumbing only; nothing here calls the library under test.

One batch: the equation `const` = dict(A[n], B[m], G[m][n], target[1]) in one copy and `proofs`, a list of
dict(xcoms[m], ycoms[n], pi[kx], theta[ky]); rho[N][4] with rho[e][2a+b] the exponent of cell (a, b)."""
import numpy as np

import forge
from forge import ref
from stmtrlc import MSMEG1, MSMEG2, PPE, QUAD, folded_value, gt_one, shape  # noqa: F401

CONST = ("A", "B", "G", "target")
PROOF = ("xcoms", "ycoms", "pi", "theta")


def equation_of(cname, ty, m, n, const, proof, crs):
    """proof e with the shared constants as a forge dict"""
    eq = dict(cname=cname, ty=ty, m=m, n=n, crs=forge.u8(crs))
    eq.update({k: forge.u8(const[k]) for k in CONST})
    eq.update({k: forge.u8(proof[k]) for k in PROOF})
    return eq


def replicated(const, proofs):
    """the eight arrays gs_verify_batch_rlc takes for the same batch: the constants N times"""
    N = len(proofs)
    return [np.concatenate([forge.u8(const[k])] * N) for k in CONST] + \
           [np.concatenate([forge.u8(p[k]) for p in proofs]) for k in PROOF]


def arrays(const, proofs):
    """the eight arrays gs_verify_equation_rlc takes: the constants once"""
    return [forge.u8(const[k]) for k in CONST] + [np.concatenate([forge.u8(p[k]) for p in proofs]) for k in PROOF]


def combine(cname, ty, target, cells, rho):
    """(W, T, verdicts) from the oracle's cells of every proof: W = prod_e prod_c (lhs_c / den_c)^rho_e,c with den = rhs
    without the PPE target, T = t^(sum_e rho_e,3) as the product of the per-proof powers (PPE, else one)"""
    c = forge.curve(cname)
    one = gt_one(cname)
    W, T, oks = one, one, []
    for e, (ok, lhs, rhs, rhs_nt) in enumerate(cells):
        oks.append(ok)
        den = rhs_nt if ty == PPE else rhs
        for k in range(4):
            if (lhs[k] != den[k]).any():
                q = ref.gt_mul(cname, lhs[k], ref.gt_inv(cname, den[k]))
                W = ref.gt_mul(cname, W, ref.gt_pow(cname, q, forge.u8(c.fr(int(rho[e][k])))))
        if ty == PPE:
            T = ref.gt_mul(cname, T, ref.gt_pow(cname, forge.u8(target), forge.u8(c.fr(int(rho[e][3])))))
    return W, T, oks


def literal(cname, ty, m, n, const, proofs, rho, crs):
    cells = []
    for p in proofs:
        eq = equation_of(cname, ty, m, n, const, p, crs)
        cells.append(forge.oracle_cells(eq, eq))
    return combine(cname, ty, const["target"], cells, rho)


def sum_rho(rho):
    """r_ab = sum_e rho_e,ab as exact integers, [r_00, r_01, r_10, r_11]: the contract of the device's 128-bit reduction
    (low and high 32-bit halves summed separately in 64 bits, then put together)"""
    out = []
    for c in range(4):
        lo = hi = 0
        for row in rho:
            v = int(row[c])
            lo += v & 0xFFFFFFFF
            hi += v >> 32
        assert lo < 1 << 64 and hi < 1 << 64  # what the device's counters hold
        out.append(lo + (hi << 32))
    return out


def pair_counts(ty, m, n, fold_pi):
    """(pairs per proof, pairs per batch) of the folded check"""
    xg, yg, kx, ky = shape(ty)
    per_proof = 2 * n + (0 if fold_pi else 2 * kx)
    per_batch = (m if yg else 2) + 2 * ky + (2 * kx if fold_pi else 0) + (1 if ty == MSMEG2 else 0)
    return per_proof, per_batch


def folded_pairs(cname, ty, m, n, const, proofs, rho, crs, fold_pi):
    """([(P, Q)] per proof, [(P, Q)] per batch): prod e(P, Q) over both lists = W of literal().  fold_pi: item 3 of
    DESIGN.md 6.7 folded in G2 across the batch (True) or kept as per-proof pairs e(-U'_e,kb, pi_e,k.b) (False)."""
    cx = forge.Ctx(cname, crs)
    r = cx.r
    xg, yg, kx, ky = shape(ty)
    G1, G2 = cx.G1, cx.G2
    N = len(proofs)
    rho = [[int(v) for v in row] for row in rho]
    R = lambda e, a, b: rho[e][2 * a + b]
    rs = sum_rho(rho)
    RS = lambda a, b: rs[2 * a + b]
    pt = lambda arr, i, sz: forge.u8(arr)[i * sz:(i + 1) * sz]
    ints = lambda arr: cx.fr_ints(forge.u8(arr))

    def msm(group, terms):
        acc = np.zeros(cx.size(group), np.uint8)  # the identity
        for k, p in terms:
            acc = cx.add(group, acc, cx.mul(group, p, k % r))
        return acc

    W1 = [cx.u[1][:G1], cx.add(1, cx.u[1][G1:], cx.g1)]
    W2 = [cx.v[1][:G2], cx.add(2, cx.v[1][G2:], cx.g2)]
    gam = ints(const["G"])
    a_s = None if xg else ints(const["A"])
    b_s = None if yg else ints(const["B"])
    t_s = ints(const["target"])[0] if ty == QUAD else None
    # C'_e,ib and Th'_e,lb
    Cp = [[[msm(1, [(R(e, a, b), pt(p["xcoms"], 2 * i + a, G1)) for a in range(2)]) for b in range(2)] for i in range(m)]
          for e, p in enumerate(proofs)]
    Thp = [[[msm(1, [(R(e, a, b), pt(p["theta"], 2 * l + a, G1)) for a in range(2)]) for b in range(2)] for l in range(ky)]
           for e, p in enumerate(proofs)]
    per_proof, per_batch = [], []
    # 1. per proof: e(P'_e,jb, d_e,j.b)
    for e, p in enumerate(proofs):
        for j in range(n):
            for b in range(2):
                if xg:
                    terms = [(R(e, 1, b), pt(const["A"], j, G1))]
                else:
                    terms = [(a_s[j] * R(e, a, b), W1[a]) for a in range(2)]
                terms += [(gam[i * n + j], Cp[e][i][b]) for i in range(m)]
                per_proof.append((msm(1, terms), pt(p["ycoms"], 2 * j + b, G2)))
        if not fold_pi:  # 3, alternative: e(-U'_e,kb, pi_e,k.b)
            for k in range(kx):
                for b in range(2):
                    U = msm(1, [(-R(e, a, b), pt(cx.u[k], a, G1)) for a in range(2)])
                    per_proof.append((U, pt(p["pi"], 2 * k + b, G2)))
    # 2. per batch, against the other side's constants
    Csum = [[msm(1, [(1, Cp[e][i][b]) for e in range(N)]) for b in range(2)] for i in range(m)]
    if yg:
        for i in range(m):
            per_batch.append((Csum[i][1], pt(const["B"], i, G2)))
    else:
        for b in range(2):
            terms = [(b_s[i], Csum[i][b]) for i in range(m)]
            if ty == MSMEG1:
                terms.append((-RS(1, b), forge.u8(const["target"])))
            if ty == QUAD:
                terms += [(-RS(a, b) * t_s, W1[a]) for a in range(2)]
            per_batch.append((msm(1, terms), W2[b]))
    # 3. per batch: e(-u_k.a, sum_e sum_b rho_e,ab pi_e,k.b)
    if fold_pi:
        for k in range(kx):
            for a in range(2):
                q = msm(2, [(R(e, a, b), pt(p["pi"], 2 * k + b, G2)) for e, p in enumerate(proofs) for b in range(2)])
                per_batch.append((cx.neg(1, pt(cx.u[k], a, G1)), q))
    # 4. per batch: e(-sum_e Th'_e,lb, v_l.b)
    for l in range(ky):
        for b in range(2):
            per_batch.append((msm(1, [(-1, Thp[e][l][b]) for e in range(N)]), pt(cx.v[l], b, G2)))
    # 5. MSMEG2: e(-(r_01 W1.0 + r_11 W1.1), t)
    if ty == MSMEG2:
        per_batch.append((msm(1, [(-RS(a, 1), W1[a]) for a in range(2)]), forge.u8(const["target"])))
    return per_proof, per_batch

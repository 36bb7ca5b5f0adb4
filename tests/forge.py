"""Well-formed forged proofs: variants of one Groth-Sahai equation whose every group element is a point of the
prime-order subgroup (or the identity) and whose every scalar is canonical, so that a verifier cannot reject them for
what they ARE, only for what the equation says about them.  (A flipped bit in a coordinate gives a point off the curve;
any verifier that reads the element rejects it, whether or not it checks the equation.)

Everything here is computed with the test oracles (oracle/gs_ref.c through gs_ref_py, oracle/gs_oracle.py for the
on-curve test), never with the library under test.  Arrays are uint8 in the boundary layout of include/gs_amd.h.

An equation is a dict: cname, ty, m, n, A, B, G, target, xcoms, ycoms, pi, theta, crs, and for the variants that need
a new honest proof also the witness X, Y.  A variant is a dict with the eight verifier inputs, `name`, `kind`, and
  accepted : True for the kinds that are valid proofs by construction (the verdict of every other variant is whatever
             the oracle says: a forged slot the equation does not look at -- a zero row of Gamma with a zero B -- is
             accepted by the reference too);
  cell     : for the single-cell kinds, the one cell (a, b) of the ComT comparison that disagrees.

The single-cell kinds need a CRS in the hiding form of include/gs_amd.h whose trapdoors are known (crs_pair):
  u = [(p1, a1 p1), (t1 p1, t1 a1 p1 - p1)],  v = [(p2, a2 p2), (t2 p2, t2 a2 p2 - p2)].
Adding s Q to pi[0].b and s' Q to pi[1].b (Q in G2) multiplies the right-hand side of cell (0,b) by
e(p1,Q)^(s + s' t1) and that of cell (1,b) by e(p1,Q)^(a1 (s + s' t1) - s').  s = -s' t1 leaves a mismatch in cell (1,b)
alone; s' = a1 w, s = w (1 - a1 t1) leaves e(p1,Q)^w in cell (0,b) alone.  Mirrored on theta with P in G1, a2, t2:
theta[0].a += s P, theta[1].a += s' P changes cell (a,0) by s + s' t2 and cell (a,1) by a2 (s + s' t2) - s'.
Which cells each type can isolate:
  PPE     (kx = ky = 2): all four, each through pi and through theta;
  MSMEG1  (kx = 2, ky = 1): all four through pi (b = 0, 1; row 0 or 1);
  MSMEG2  (kx = 1, ky = 2): all four through theta;
  QuadEqu (kx = ky = 1): none.  With one pi and one theta the four slots give changes
          (c00, c01, c10, c11) = (s0 + r0, s1 + a2 r0, a1 s0 + r1, a1 s1 + a2 r1), which always satisfy
          c11 = a1 c01 + a2 c10 - a1 a2 c00; a vector with exactly one non-zero entry does not (a1, a2 != 0).
On the BINDING form (u1 = t1 u0) the choice s = -s' t1 cancels in both cells: an accepted variant."""
import os
import sys

import numpy as np

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402
import gs_ref_py as ref  # noqa: E402

PPE, MSMEG1, MSMEG2, QUAD = 0, 1, 2, 3
INPUTS = ("A", "B", "G", "target", "xcoms", "ycoms", "pi", "theta")
SLOT_ARRAYS = (("xcoms", 1), ("ycoms", 2), ("pi", 2), ("theta", 1))
# every kind the builder knows; test_forge_cpu.py fails if one of them is produced nowhere
KINDS = ("plus_gen", "neg", "identity", "swap_halves", "swap_pi", "swap_theta", "A_plus", "B_plus", "gamma_plus",
         "gamma_zero", "target", "other_proof", "other_all", "accepted_fresh", "accepted_rerand", "accepted_bindcancel",
         "cell")


def xg(ty):
    return ty in (PPE, MSMEG1)


def yg(ty):
    return ty in (PPE, MSMEG2)


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


class Ctx:
    """Sizes, generators and small arithmetic of one curve + CRS (all through the C oracle)."""

    def __init__(self, cname, crs):
        self.cname, self.c = cname, curve(cname)
        self.FQ, self.FR, self.G1, self.G2, self.GT, self.CRS = ref.sizes(cname)
        self.crs = u8(crs)
        assert self.crs.size == self.CRS
        o = 4 * self.G1
        self.u = [self.crs[k * 2 * self.G1:(k + 1) * 2 * self.G1] for k in range(2)]
        self.v = [self.crs[o + k * 2 * self.G2:o + (k + 1) * 2 * self.G2] for k in range(2)]
        o += 4 * self.G2
        self.g1, self.g2, self.gt = self.crs[o:o + self.G1], self.crs[o + self.G1:o + self.G1 + self.G2], \
            self.crs[o + self.G1 + self.G2:]
        self.r = self.c.r

    def size(self, group):
        return self.G1 if group == 1 else self.G2

    def gen(self, group):
        return self.g1 if group == 1 else self.g2

    def fr(self, v):
        return u8(self.c.fr(v % self.r))

    def fr_mat(self, M):
        return np.concatenate([self.fr(v) for row in M for v in row]) if M and M[0] else np.zeros(0, np.uint8)

    def fr_ints(self, a):
        a = u8(a).view(np.uint64).reshape(-1, 4)
        return [self.c.fr_dec(x) for x in a]

    def add(self, group, p, q):
        return ref.g_add(self.cname, group, p, q)

    def mul(self, group, p, k):
        return ref.g_mul(self.cname, group, p, self.fr(k))

    def neg(self, group, p):
        return self.mul(group, p, self.r - 1)

    def slots_add(self, group, a, b):
        """element-wise sum of two arrays of points"""
        sz = self.size(group)
        return np.concatenate([self.add(group, a[i:i + sz], b[i:i + sz]) for i in range(0, a.size, sz)])


def crs_pair(cname, p1, p2, a1, a2, t1, t2):
    """(binding, hiding) CRS bytes over the generators p1, p2 with the trapdoors a1, a2, t1, t2 (C oracle arithmetic).
    The hiding form is the binding form with p1 (p2) subtracted from u[1].1 (v[1].1)."""
    c = curve(cname)
    fr = lambda v: u8(c.fr(v % c.r))
    m1 = lambda p, k: ref.g_mul(cname, 1, p, fr(k))
    m2 = lambda p, k: ref.g_mul(cname, 2, p, fr(k))
    p1, p2 = u8(p1), u8(p2)
    q1, q2 = m1(p1, a1), m2(p2, a2)
    u1, u2 = m1(p1, t1), m2(p2, t2)
    v1, v2 = m1(q1, t1), m2(q2, t2)
    gt = ref.multi_pairing(cname, 1, p1, p2)
    binding = np.concatenate([p1, q1, u1, v1, p2, q2, u2, v2, p1, p2, gt])
    h1 = ref.g_add(cname, 1, v1, m1(p1, c.r - 1))
    h2 = ref.g_add(cname, 2, v2, m2(p2, c.r - 1))
    hiding = np.concatenate([p1, q1, u1, h1, p2, q2, u2, h2, p1, p2, gt])
    return binding, hiding


def prove(eq, R, S, T):
    """Honest commitments and proof of eq's statement for its witness, by the C oracle (R, S, T: lists of ints)."""
    cx = Ctx(eq["cname"], eq["crs"])
    return ref.commit_and_prove(eq["cname"], eq["ty"], eq["m"], eq["n"], eq["X"], eq["Y"], eq["A"], eq["B"], eq["G"],
                                cx.fr_mat(R), cx.fr_mat(S), cx.fr_mat(T), cx.crs)


def rand_mats(eq, rng):
    ty, m, n = eq["ty"], eq["m"], eq["n"]
    kx, ky = (2 if xg(ty) else 1), (2 if yg(ty) else 1)
    r = curve(eq["cname"]).r
    mat = lambda a, b: [[rng.randrange(1, r) for _ in range(b)] for _ in range(a)]
    return mat(m, kx), mat(n, ky), mat(ky, kx)


def _matmul(a, b, r):
    return [[sum(a[i][k] * b[k][j] for k in range(len(b))) % r for j in range(len(b[0]))] for i in range(len(a))]


def _tr(a):
    return [list(x) for x in zip(*a)]


def rerandomize(eq, R1, S1, T1):
    """The formulas of gs_rerandomize_batch (include/gs_amd.h; restated in tests/test_rerand_algebra.py) with the C oracle:
         c' = c + R' U      d' = d + S' V
         pi' = pi + R'^T iota2(B) + (R'^T Gamma) d + (R'^T Gamma S' - T'^T) V
         theta' = theta + S'^T iota1(A) + (S'^T Gamma^T) c + T' U"""
    cx = Ctx(eq["cname"], eq["crs"])
    cn, ty, m, n, r = eq["cname"], eq["ty"], eq["m"], eq["n"], cx.r
    kx, ky = (2 if xg(ty) else 1), (2 if yg(ty) else 1)
    U = np.concatenate(cx.u[:kx])
    V = np.concatenate(cx.v[:ky])
    z1, z2 = np.zeros(cx.G1, np.uint8), np.zeros(cx.G2, np.uint8)
    if xg(ty):
        map_a = np.concatenate([np.concatenate([z1, eq["A"][j * cx.G1:(j + 1) * cx.G1]]) for j in range(n)])
    else:
        w = np.concatenate([cx.u[1][:cx.G1], cx.add(1, cx.u[1][cx.G1:], cx.g1)])
        map_a = np.concatenate([np.concatenate([ref.g_mul(cn, 1, w[:cx.G1], eq["A"][j * 32:(j + 1) * 32]),
                                                ref.g_mul(cn, 1, w[cx.G1:], eq["A"][j * 32:(j + 1) * 32])])
                                for j in range(n)])
    if yg(ty):
        map_b = np.concatenate([np.concatenate([z2, eq["B"][i * cx.G2:(i + 1) * cx.G2]]) for i in range(m)])
    else:
        w = np.concatenate([cx.v[1][:cx.G2], cx.add(2, cx.v[1][cx.G2:], cx.g2)])
        map_b = np.concatenate([np.concatenate([ref.g_mul(cn, 2, w[:cx.G2], eq["B"][i * 32:(i + 1) * 32]),
                                                ref.g_mul(cn, 2, w[cx.G2:], eq["B"][i * 32:(i + 1) * 32])])
                                for i in range(m)])
    g = cx.fr_ints(eq["G"])
    G = [g[i * n:(i + 1) * n] for i in range(m)]
    R1t, S1t = _tr(R1), _tr(S1)
    lm = lambda group, lhs, col: ref.left_mul(cn, group, len(lhs), len(lhs[0]), cx.fr_mat(lhs), col)
    xc2 = cx.slots_add(1, eq["xcoms"], lm(1, R1, U))
    yc2 = cx.slots_add(2, eq["ycoms"], lm(2, S1, V))
    psi = _matmul(R1t, G, r)
    omega = [[(a - b) % r for a, b in zip(ra, rb)] for ra, rb in zip(_matmul(psi, S1, r), _tr(T1))]
    pi2 = cx.slots_add(2, cx.slots_add(2, cx.slots_add(2, eq["pi"], lm(2, R1t, map_b)), lm(2, psi, eq["ycoms"])),
                       lm(2, omega, V))
    phi = _matmul(S1t, _tr(G), r)
    th2 = cx.slots_add(1, cx.slots_add(1, cx.slots_add(1, eq["theta"], lm(1, S1t, map_a)), lm(1, phi, eq["xcoms"])),
                       lm(1, T1, U))
    return dict(xcoms=xc2, ycoms=yc2, pi=pi2, theta=th2)


def other_of(eq, rng):
    """Commitments and honest proof of a DIFFERENT equation of the same shape: the same constants and Gamma with the
    first x variable moved by the generator (by one for scalars), hence another target; new randomness."""
    cx = Ctx(eq["cname"], eq["crs"])
    e2 = dict(eq)
    X = u8(eq["X"])
    if xg(eq["ty"]):
        X[:cx.G1] = cx.add(1, X[:cx.G1], cx.g1)
    else:
        X[:32] = cx.fr(cx.fr_ints(X[:32])[0] + 1)
    e2["X"] = X
    return prove(e2, *rand_mats(eq, rng))


def _variant(eq, name, kind, accepted=False, cell=None, **changed):
    v = {k: eq[k] for k in INPUTS}
    v.update({k: u8(a) for k, a in changed.items()})
    v.update(name=name, kind=kind, accepted=accepted, cell=cell)
    return v


def same_bytes(a, b):
    return all(a[k].size == b[k].size and (a[k] == b[k]).all() for k in INPUTS)


def build(eq, rng, other=None, trap=None, hiding=False):
    """All variants of `eq`.  other: commitments and proof (xcoms, ycoms, pi, theta) of a different honest equation of the
    same shape.  trap = (a1, a2, t1, t2) of eq's CRS, hiding = its form: enables the single-cell kinds (hiding) or the
    cancelling accepted kind (binding).  A kind that would leave a slot unchanged is not generated for that slot."""
    cx = Ctx(eq["cname"], eq["crs"])
    ty, m, n, r = eq["ty"], eq["m"], eq["n"], cx.r
    kx, ky = (2 if xg(ty) else 1), (2 if yg(ty) else 1)
    eq = dict(eq)
    for k in INPUTS:
        eq[k] = u8(eq[k])
    out = []

    def put(arr, off, val):
        a = arr.copy()
        a[off:off + val.size] = val
        return a

    # ---- every G1/G2 slot of the commitments and the proof
    for key, group in SLOT_ARRAYS:
        sz, arr = cx.size(group), eq[key]
        for s in range(arr.size // sz):
            p = arr[s * sz:(s + 1) * sz]
            nm = "%s[%d].%d" % (key, s // 2, s % 2)
            out.append(_variant(eq, nm + " += gen", "plus_gen", **{key: put(arr, s * sz, cx.add(group, p, cx.gen(group)))}))
            if p.any():
                out.append(_variant(eq, nm + " negated", "neg", **{key: put(arr, s * sz, cx.neg(group, p))}))
                out.append(_variant(eq, nm + " = identity", "identity", **{key: put(arr, s * sz, np.zeros(sz, np.uint8))}))
        for k in range(arr.size // (2 * sz)):
            a, b = arr[2 * k * sz:(2 * k + 1) * sz], arr[(2 * k + 1) * sz:(2 * k + 2) * sz]
            if (a != b).any():
                out.append(_variant(eq, "%s[%d] halves swapped" % (key, k), "swap_halves",
                                    **{key: put(arr, 2 * k * sz, np.concatenate([b, a]))}))
    for key, kind, k, group in (("pi", "swap_pi", kx, 2), ("theta", "swap_theta", ky, 1)):
        sz = 2 * cx.size(group)
        if k == 2 and (eq[key][:sz] != eq[key][sz:]).any():
            out.append(_variant(eq, key + "[0] <-> " + key + "[1]", kind,
                                **{key: np.concatenate([eq[key][sz:], eq[key][:sz]])}))
    # ---- the statement: constants, Gamma, target
    one = lambda a, i: put(a, i * 32, cx.fr(cx.fr_ints(a[i * 32:(i + 1) * 32])[0] + 1))
    for key, kind, cnt, isg, group in (("A", "A_plus", n, xg(ty), 1), ("B", "B_plus", m, yg(ty), 2)):
        for i in range(cnt):
            if isg:
                sz = cx.size(group)
                new = put(eq[key], i * sz, cx.add(group, eq[key][i * sz:(i + 1) * sz], cx.gen(group)))
            else:
                new = one(eq[key], i)
            out.append(_variant(eq, "%s[%d] += %s" % (key, i, "gen" if isg else "1"), kind, **{key: new}))
    gam = cx.fr_ints(eq["G"])
    for i in range(m * n):
        out.append(_variant(eq, "Gamma[%d][%d] += 1" % (i // n, i % n), "gamma_plus", G=one(eq["G"], i)))
    nz = [i for i in range(m * n) if gam[i] != 0]
    if nz:
        i = nz[len(nz) // 2]
        out.append(_variant(eq, "Gamma[%d][%d] = 0" % (i // n, i % n), "gamma_zero", G=put(eq["G"], i * 32, cx.fr(0))))
    if ty == PPE:
        tgt, what = ref.gt_mul(cx.cname, eq["target"], cx.gt), "*= gt"
    elif ty == MSMEG1:
        tgt, what = cx.add(1, eq["target"], cx.g1), "+= g1"
    elif ty == MSMEG2:
        tgt, what = cx.add(2, eq["target"], cx.g2), "+= g2"
    else:
        tgt, what = one(eq["target"], 0), "+= 1"
    out.append(_variant(eq, "target " + what, "target", target=tgt))
    # ---- somebody else's honest proof
    if other is not None:
        out.append(_variant(eq, "pi, theta of another equation", "other_proof", pi=other["pi"], theta=other["theta"]))
        out.append(_variant(eq, "commitments and proof of another equation", "other_all",
                            **{k: other[k] for k in ("xcoms", "ycoms", "pi", "theta")}))
    # ---- valid proofs that differ from the prover's output
    if "X" in eq:
        out.append(_variant(eq, "accepted: fresh randomness", "accepted_fresh", accepted=True, **prove(eq, *rand_mats(eq, rng))))
    out.append(_variant(eq, "accepted: rerandomized", "accepted_rerand", accepted=True,
                        **rerandomize(eq, *rand_mats(eq, rng))))
    # ---- trapdoor kinds
    if trap is not None:
        a1, a2, t1, t2 = trap
        sides = []
        if kx == 2:
            sides.append(("pi", 2, a1, t1))
        if ky == 2:
            sides.append(("theta", 1, a2, t2))
        for key, group, a, t in sides:
            sz, Q = cx.size(group), cx.gen(group)

            def shifted(comp, s, s1):
                arr = eq[key]
                for k, sc in ((0, s), (1, s1)):
                    off = (2 * k + comp) * sz
                    arr = put(arr, off, cx.add(group, arr[off:off + sz], cx.mul(group, Q, sc)))
                return arr

            for comp in (0, 1):
                w = rng.randrange(1, r)
                if not hiding:
                    out.append(_variant(eq, "accepted: %s[.].%d += (-w t, w) gen on the binding key" % (key, comp),
                                        "accepted_bindcancel", accepted=True, **{key: shifted(comp, -w * t % r, w)}))
                    continue
                # (row, col) of the cell: pi shifts column `comp`, rows (0 | 1); theta shifts row `comp`, columns (0 | 1)
                cell = lambda other_idx: (other_idx, comp) if key == "pi" else (comp, other_idx)
                out.append(_variant(eq, "cell %s only: %s[.].%d += (-w t, w) gen" % (cell(1), key, comp), "cell",
                                    cell=cell(1), **{key: shifted(comp, -w * t % r, w)}))
                out.append(_variant(eq, "cell %s only: %s[.].%d += (w (1 - a t), a w) gen" % (cell(0), key, comp), "cell",
                                    cell=cell(0), **{key: shifted(comp, w * (1 - a * t) % r, a * w % r)}))
    return out


def on_curve(cname, ty, v):
    """Every G1/G2 element of a variant passes the big-integer oracle's on-curve test; every scalar is canonical."""
    c = curve(cname)
    O.set_curve(O.BLS12_381 if cname == "bls12_381" else O.BN254)
    G1, G2 = 16 * c.nq, 32 * c.nq

    def pts(a, group):
        sz = G1 if group == 1 else G2
        a = a.view(np.uint64)
        for i in range(0, a.size, sz // 8):
            p = a[i:i + sz // 8]
            if group == 1:
                if not O.g1_on_curve(O.dec_g1(c.g1_dec(p))):
                    return False
            elif not O.g2_on_curve(O.dec_g2(c.g2_dec(p))):
                return False
        return True

    def frs(a):
        a = a.view(np.uint64).reshape(-1, 4)
        return all(sum(int(x) << (64 * i) for i, x in enumerate(row)) < c.r for row in a)

    ok = pts(v["xcoms"], 1) and pts(v["theta"], 1) and pts(v["ycoms"], 2) and pts(v["pi"], 2) and frs(v["G"])
    ok = ok and (pts(v["A"], 1) if xg(ty) else frs(v["A"])) and (pts(v["B"], 2) if yg(ty) else frs(v["B"]))
    if ty == MSMEG1:
        ok = ok and pts(v["target"], 1)
    elif ty == MSMEG2:
        ok = ok and pts(v["target"], 2)
    elif ty == QUAD:
        ok = ok and frs(v["target"])
    return ok


def oracle_verdict(eq, v):
    return ref.verify(eq["cname"], eq["ty"], eq["m"], eq["n"], v["A"], v["B"], v["G"], v["target"], v["xcoms"],
                      v["ycoms"], v["pi"], v["theta"], u8(eq["crs"]))


def oracle_cells(eq, v):
    """(verdict, lhs, rhs, rhs without the target's lin_t): 4 GT each, cells (0,0) (0,1) (1,0) (1,1)"""
    return ref.verify_cells(eq["cname"], eq["ty"], eq["m"], eq["n"], v["A"], v["B"], v["G"], v["target"], v["xcoms"],
                            v["ycoms"], v["pi"], v["theta"], u8(eq["crs"]))


# ---- golden statements in boundary layout -------------------------------------------------------------------------
def golden_crs(c):
    g = c.golden["crs"]
    return u8(np.concatenate([c.com1(g["u"][0]), c.com1(g["u"][1]), c.com2(g["v"][0]), c.com2(g["v"][1]), c.g1(g["g1"]),
                              c.g2(g["g2"]), c.f12(g["gt"])]))


def golden_eq(cname, case, crs=None, rng=None):
    """The statement and witness of a golden case with the oracle's honest proof: the stored one (crs None: the golden
    CRS and the case's own R, S, T) or a new one under `crs` with randomness from rng."""
    c = curve(cname)
    ty, m, n = case["type"], case["m"], case["n"]
    ex = c.g1 if xg(ty) else c.fr_hex
    ey = c.g2 if yg(ty) else c.fr_hex
    cat = lambda f, vals: u8(np.concatenate([f(v) for v in vals]))
    eq = dict(cname=cname, ty=ty, m=m, n=n, X=cat(ex, case["xvars"]), Y=cat(ey, case["yvars"]), A=cat(ex, case["a"]),
              B=cat(ey, case["b"]), G=u8(c.fr_mat(case["gamma"])),
              target=u8({0: c.f12, 1: c.g1, 2: c.g2, 3: c.fr_hex}[ty](case["target"])),
              crs=golden_crs(c) if crs is None else u8(crs))
    if crs is None:
        ints = lambda M: [[int(s, 16) for s in row] for row in M]
        eq.update(prove(eq, ints(case["R"]), ints(case["S"]), ints(case["T"])))
    else:
        eq.update(prove(eq, *rand_mats(eq, rng)))
    return eq


def bigint_verdict(cname, ty, m, n, v, crs):
    """The verdict of the big-integer oracle (gs_oracle.verify) on a variant; ~5 s for a 2x1 equation."""
    c = curve(cname)
    O.set_curve(O.BLS12_381 if cname == "bls12_381" else O.BN254)
    w = lambda a: u8(a).view(np.uint64)
    g1s = lambda a: [O.dec_g1(c.g1_dec(p)) for p in w(a).reshape(-1, 2 * c.nq)]
    g2s = lambda a: [O.dec_g2(c.g2_dec(p)) for p in w(a).reshape(-1, 4 * c.nq)]
    frs = lambda a: [c.fr_dec(x) for x in w(a).reshape(-1, 4)]
    pairs = lambda pts: [(pts[i], pts[i + 1]) for i in range(0, len(pts), 2)]
    G1, G2 = 16 * c.nq, 32 * c.nq
    crs = u8(crs)
    o = 4 * G1 + 4 * G2
    key = {"u": pairs(g1s(crs[:4 * G1])), "v": pairs(g2s(crs[4 * G1:o])), "g1": g1s(crs[o:o + G1])[0],
           "g2": g2s(crs[o + G1:o + G1 + G2])[0], "gt": O.dec_f12(c.f12_dec(w(crs[o + G1 + G2:])))}
    gam = frs(v["G"])
    tgt = {PPE: lambda a: O.dec_f12(c.f12_dec(w(a))), MSMEG1: lambda a: g1s(a)[0], MSMEG2: lambda a: g2s(a)[0],
           QUAD: lambda a: frs(a)[0]}[ty](v["target"])
    equ = {"type": ty, "a": g1s(v["A"]) if xg(ty) else frs(v["A"]), "b": g2s(v["B"]) if yg(ty) else frs(v["B"]),
           "gamma": [gam[i * n:(i + 1) * n] for i in range(m)], "target": tgt}
    return int(bool(O.verify(equ, pairs(g1s(v["xcoms"])), pairs(g2s(v["ycoms"])), pairs(g2s(v["pi"])),
                             pairs(g1s(v["theta"])), key)))

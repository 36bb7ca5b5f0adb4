"""The named scalars of tests/scalarvec.py on the device: every kernel that turns an Fr scalar into digits -- k_smul_batch
(Barrett division / lattice rounding + signed windows, and recode_w4 with endo = 0), the one-term lanes of run_side behind
gs_mat_left_mul, k_fix on the 16-bit window tables, k_extract with an adversarial launch-wide key (shared_digits),
k_gt_pow's bit loop, and the Straus lanes of prove / verify -- bit-exact against the C restatement of the reference
(oracle/gs_ref.c) and, on a sample of every test, the big-integer oracle (oracle/gs_oracle.py).

The points are known multiples of the generator, so an expectation is the reference's [s] generator for a scalar s the
test composes with integers (as tests/test_extract_algebra.py composes commitments); where the reference has the
operation itself (left_mul, gt_pow, commit_and_prove, verify) that is compared too."""
import fnmatch
import os
import random
import sys

import numpy as np
import pytest

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu

CURVES = [(0, "bls12_381"), (1, "bn254")]
CG = [(cid, cname, g) for cid, cname in CURVES for g in (1, 2)]


class Ctx:
    """One engine per curve, the table, and the reference's multiples of the generators (computed once, shared)."""

    def __init__(self, cid, cname):
        import groth_sahai_rs_amd as gs
        import scalarvec as S
        import wirevec as V

        self.cid, self.cname, self.c = cid, cname, curve(cname)
        self.oc = V.setc(cname)
        self.r = self.oc.r
        self.eng = gs.Engine(cid, 0)
        self.gen = {1: np.asarray(V.point_limbs(cname, self.oc.g1, 1)).view(np.uint8),
                    2: np.asarray(V.point_limbs(cname, self.oc.g2, 2)).view(np.uint8)}
        self.cases = S.table(cname)
        self.ks = [case.k for case in self.cases]
        self.named = S.by_name(cname)
        self._pt = {}

    def frs(self, vals):
        """Montgomery scalars, one row of 32 bytes each"""
        if len(vals) == 0:
            return np.zeros((0, 32), dtype=np.uint8)
        return np.concatenate([self.c.fr(v % self.r) for v in vals]).view(np.uint8).reshape(len(vals), 32)

    def mul(self, group, k):
        """[k] generator on the C restatement of the reference"""
        import gs_ref_py as ref

        key = (group, k % self.r)
        if key not in self._pt:
            self._pt[key] = ref.g_mul(self.cname, group, self.gen[group], self.c.fr(key[1]))
        return self._pt[key]

    def muls(self, group, ks):
        return np.stack([self.mul(group, k) for k in ks])

    def oracle_mul(self, group, k):
        """[k] generator on the big-integer oracle"""
        import gs_oracle as O
        import wirevec as V

        V.setc(self.cname)
        pt = O.ec_mul(V.fld(group), k % self.r, self.oc.g1 if group == 1 else self.oc.g2)
        return np.asarray(V.point_limbs(self.cname, pt, group)).view(np.uint8).reshape(-1)

    def check_oracle(self, group, ks):
        """the two references agree on these multiples"""
        for k in ks:
            assert (self.mul(group, k) == self.oracle_mul(group, k)).all(), hex(k)

    def name(self, k):
        import scalarvec as S

        return S.name_of(self.cname, k % self.r)


_CTX = {}


def ctx(cid, cname):
    if cid not in _CTX:
        _CTX[cid] = Ctx(cid, cname)
    K = _CTX[cid]
    for key, val in (("endo", 1), ("var_tm", 0), ("var_w", 0), ("var_mo", 0), ("var_tab", 0)):
        K.eng.set_option(key, val)
    return K


class profiled:
    """kernel names that ran inside the block"""

    def __init__(self, eng):
        self.eng, self.names = eng, []

    def __enter__(self):
        self.eng.prof_enable(True)
        self.eng.prof_reset()
        return self

    def __exit__(self, *exc):
        self.eng.sync()
        self.names = [p[0] for p in self.eng.prof_get()]
        self.eng.prof_enable(False)
        return False

    def ran(self, pattern):
        return any(fnmatch.fnmatchcase(nm, pattern) for nm in self.names)


def same(got, want, labels):
    got = np.asarray(got).reshape(len(labels), -1)
    want = np.asarray(want).reshape(len(labels), -1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [labels[i] for i in bad[:8]]


# ---- 1. g_mul_batch (k_smul_batch) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("endo", [1, 0])
@pytest.mark.parametrize("cid,cname,group", CG)
def test_g_mul_batch_table(cid, cname, group, endo):
    """The whole table in one call on one broadcast point; slices of 1, 63, 64 and 65 lanes; then per-lane points
    (multiples of the generator, every third lane the identity) with the table in order and reversed, so that a wave
    mixes digit shapes.  endo = 1: the GLV / GLS decompositions; endo = 0: recode_w4 on the whole scalar."""
    K = ctx(cid, cname)
    eng, ks, n, r = K.eng, K.ks, len(K.ks), K.r
    names = [case.name for case in K.cases]
    want = K.muls(group, ks)
    if endo:
        K.check_oracle(group, ks[::24])
    eng.set_option("endo", endo)
    with profiled(eng) as prof:
        got = eng.g_mul_batch(group, K.gen[group], K.frs(ks), broadcast=True)
    assert prof.ran("k_smul_batch%s.g%d" % ("" if endo else ".plain", group)), prof.names
    same(got, want, names)
    for cnt in (1, 63, 64, 65):
        for start in (0, (n - cnt) // 2, n - cnt):
            got = eng.g_mul_batch(group, K.gen[group], K.frs(ks[start:start + cnt]), broadcast=True)
            same(got, want[start:start + cnt], names[start:start + cnt])
    ms = [0 if i % 3 == 2 else 2 + i % 7 for i in range(n)]
    pts = K.muls(group, ms)
    for order, tag in ((ks, "in order"), (ks[::-1], "reversed")):
        got = eng.g_mul_batch(group, pts, K.frs(order))
        want2 = K.muls(group, [k * m % r for k, m in zip(order, ms)])
        same(got, want2, ["%s, lane %d (%s) x %d" % (tag, i, K.name(k), m) for i, (k, m) in enumerate(zip(order, ms))])
        assert not got[2].any() and got[0].any() == (order[0] != 0)


# ---- 2. mat_left_mul (run_side) -----------------------------------------------------------------------------------------
# columns as (c.0, c.1) multiples of the generator: a repeated commitment, its negative, the identity, half identities
COLS = [(2, 3), (2, 3), (-2, -3), (0, 0), (5, 7), (1, 0), (11, 13), (0, 1), (-5, -7), (17, 19), (23, 29)]
EDGE = ["r-1", "one", "nibbles_8", "nibbles_7", "(r+1)/2", "quints_10000"]


@pytest.mark.parametrize("k", [1, 2, 5, 8, 11])
@pytest.mark.parametrize("cid,cname,group", CG)
def test_mat_left_mul_table(cid, cname, group, k):
    """Rows of k consecutive table scalars, shifted cyclically: every scalar visits every term position.  Behind them
    the rows (s, r - s) on (P, P) and (s, s) on (P, -P), which must give the identity.  gs_mat_left_mul plans one term
    per lane (k_var.lm); here it runs as planned and with endo = 0 (k_var.plain.lm).  Under a forced var_tm / var_w /
    var_mo it takes the Straus lanes: tests/test_gpu_straus_edges.py."""
    import gs_ref_py as ref

    K = ctx(cid, cname)
    eng, ks, n, r = K.eng, K.ks, len(K.ks), K.r
    rows = [[ks[(i + j) % n] for j in range(k)] for i in range(n)]
    labels = ["row %d (%s ...)" % (i, K.name(ks[i])) for i in range(n)]
    zero_rows = []
    for nm in EDGE:
        s = K.named[nm]
        if k >= 2:
            zero_rows.append(len(rows))
            rows.append([s, r - s] + [0] * (k - 2))
            labels.append("(s, r - s) on (P, P), s = " + nm)
        if k >= 3:
            zero_rows.append(len(rows))
            rows.append([s, 0, s] + [0] * (k - 3))
            labels.append("(s, s) on (P, -P), s = " + nm)
    col = np.concatenate([np.concatenate([K.mul(group, a), K.mul(group, b)]) for a, b in COLS[:k]])
    lhs = K.frs([v for row in rows for v in row])
    want = np.stack([np.concatenate([K.mul(group, sum(v * ab[comp] for v, ab in zip(row, COLS)) % r) for comp in (0, 1)])
                     for row in rows])
    for endo, kern in ((1, "k_var.lm"), (0, "k_var.plain.lm")):
        eng.set_option("endo", endo)
        with profiled(eng) as prof:
            got = eng.mat_left_mul(group, len(rows), k, lhs, col)
        assert prof.ran(kern), (kern, prof.names)
        same(got, want, labels)
        assert not got[zero_rows].any()
    # the reference's own left_mul on a sample of the rows (every 40th and the identity rows)
    sample = list(range(0, n, 40)) + zero_rows
    out = ref.left_mul(cname, group, len(sample), k, lhs.reshape(len(rows), -1)[sample], col)
    same(out, want[sample], [labels[i] for i in sample])


# ---- 3. commit (k_fix on the 16-bit window tables) ---------------------------------------------------------------------
class Keyed:
    """A binding CRS whose trapdoors the test knows, installed on the curve's engine."""

    def __init__(self, K, a1, a2, t1, t2):
        self.K, self.a, self.t = K, {1: a1 % K.r, 2: a2 % K.r}, {1: t1 % K.r, 2: t2 % K.r}
        self.crs = K.eng.crs_generate(K.gen[1], K.gen[2], K.frs([a1, a2, t1, t2]))
        # the CRS is what the reference's multiples say: (p, a p, t p, t a p) per group, then the generators
        g1, g2 = K.eng.G1, K.eng.G2
        for group, off, sz in ((1, 0, g1), (2, 4 * g1, g2)):
            a, t = self.a[group], self.t[group]
            for i, s in enumerate((1, a, t, t * a)):
                assert (self.crs[off + i * sz:off + (i + 1) * sz] == K.mul(group, s)).all(), (group, i)
        K.eng.set_crs(self.crs)


_KEYED = {}


def commit_crs(K):
    """the CRS of the commit tests (one table build per curve); re-installed when an extract test replaced it"""
    if K.cid not in _KEYED:
        rnd = random.Random(8300 + K.cid)
        _KEYED[K.cid] = Keyed(K, *(rnd.randrange(2, K.r) for _ in range(4)))
    else:
        K.eng.set_crs(_KEYED[K.cid].crs)
    return _KEYED[K.cid]


COLLIDE = [(0, 1), (3, 0xFF00), (7, 0xFFFF), (8, 0x00FF), (15, 0x0100)]  # (window, digit) of the colliding entry


@pytest.mark.parametrize("kind", ["g1", "g2", "fr_b1", "fr_b2"])
@pytest.mark.parametrize("cid,cname", CURVES)
def test_commit_window_classes(cid, cname, kind):
    """Randomness from the 16-bit window classes (one window alone at d = 1, 0x00FF, 0x0100, 0xFF00, 0xFFFF; every low /
    every high byte zero), and collision lanes: the sum of one fixed-base term equals the other term's single table
    entry d 2^(16 w) * base, or its negative (r' = +-t d 2^(16 w) against a scalar whose only window w is d, both term
    orders), and a committed X that equals what the chain holds when X is added, or its negative."""
    import scalarvec as S

    K = ctx(cid, cname)
    Q = commit_crs(K)
    eng, r = K.eng, K.r
    group = 1 if kind in ("g1", "fr_b1") else 2
    a, t = Q.a[group], Q.t[group]
    tinv = pow(t, -1, r)
    W = S.scalars(cname, "window16")
    lanes, labels = [], []  # (x, r0, r1) for points (X = x * generator), (x, r0) for scalars
    if kind in ("g1", "g2"):
        for i, w0 in enumerate(W):
            lanes.append((K.ks[(5 * i + 1) % len(K.ks)], w0, W[(7 * i + 3) % len(W)]))
            labels.append("r0 = %s, r1 = %s" % (K.name(w0), K.name(lanes[-1][2])))
        for w, d in COLLIDE:
            e = d << (16 * w)
            for sg in (1, -1):
                lanes += [(3, sg * t * e, e), (3, e, sg * tinv * e),  # term sums that meet: r0 p = +-e (t p)
                          (sg * t * a * e, 0, e), (sg * a * e, e, 0),  # X = +-(what the chain holds when X is added)
                          (sg * a * (e + t * e), e, e)]
                labels += ["%s window %d digit %#x sign %+d" % (nm, w, d, sg)
                           for nm in ("r0 meets r1's entry", "r1 meets r0's entry", "X meets r1's entry",
                                      "X meets r0's entry", "X meets the sum")]
        xs = [v[0] for v in lanes]
        vars_ = K.muls(group, xs)
        rand = K.frs([v for lane in lanes for v in lane[1:]])
        rho = [(r0 + t * r1) % r for _, r0, r1 in lanes]
        want = [(rh, (x + a * rh) % r) for (x, _, _), rh in zip(lanes, rho)]
    else:
        for i, w0 in enumerate(W):
            lanes.append((w0, W[(7 * i + 3) % len(W)]))
            labels.append("x = %s, r = %s" % (K.name(w0), K.name(lanes[-1][1])))
        for w, d in COLLIDE:
            e = d << (16 * w)
            for sg in (1, -1):
                lanes += [(e, sg * t * e), (sg * tinv * e, e), (e, sg * e), (sg * e, e)]
                labels += ["%s window %d digit %#x sign %+d" % (nm, w, d, sg)
                           for nm in ("r p meets x's entry", "x (t p) meets r's entry", "x = +-r (a)", "x = +-r (b)")]
        vars_ = K.frs([v[0] for v in lanes])
        rand = K.frs([v[1] for v in lanes])
        # c = x (u1 + (O, p)) + r u0 = ((x t + r) p, (x t a + x + r a) p)
        want = [((x * t + r0) % r, (x * t * a + x + r0 * a) % r) for x, r0 in lanes]
    with profiled(eng) as prof:
        got = eng.commit(kind, vars_, rand)
    assert prof.ran("k_fix*"), prof.names
    wantb = np.stack([np.concatenate([K.mul(group, s0), K.mul(group, s1)]) for s0, s1 in want])
    same(got, wantb, labels)
    K.check_oracle(group, [s for pair in want[len(W)::5] + want[:len(W):16] for s in pair])
    # the collision lanes are what they claim: whole commitments or components at the identity
    ident = [i for i, (s0, s1) in enumerate(want) if s0 == 0 or s1 == 0]
    assert len(ident) >= len(COLLIDE) and all(i >= len(W) for i in ident)


# ---- 4. extract with an adversarial key (shared_digits, jac_smul_shared) ----------------------------------------------
def extract_keys(K):
    """(label, a1, a2): at most six keys per curve, the first four the named classes"""
    import scalarvec as S

    nm = K.named
    m = S.model(K.cname)
    if K.cname == "bls12_381":
        return [("r-1", K.r - 1, K.r - 1),
                ("multiple of lambda / one non-zero base-|x| digit", nm["g1_multiple_#0"], nm["g2_only_d2=8888888888888888"]),
                ("a Barrett correction in every division", nm["g1_corr1_#0"], nm["g2_multiple_x^3_#0"]),
                ("all nibbles 0x8", nm["nibbles_8"], nm["nibbles_8"]),
                ("largest sub-scalars", nm["g1_qmax_smax"], nm["g2_all_digits_%x" % (m.xabs - 1)]),
                ("plain carry chain", nm["plain_carry_chain_below_top"], nm["plain_top_nibble_neg8_chain"])]
    last = lambda g: max((k for k in K.ks), key=lambda k: (sum(m.decompose(g, k).signs), k))  # most negated streams
    return [("r-1", K.r - 1, K.r - 1),
            ("last rounding step of c0", nm["bn_g1_c0_step_last"], nm["bn_g2_c0_step_last"]),
            ("most negated streams", last(1), last(2)),
            ("all nibbles 0x8", nm["nibbles_8"], nm["nibbles_8"]),
            ("longest sub-scalars", nm["bn_g1_longest_stream0_#0"], nm["bn_g2_longest_stream0_#0"]),
            ("plain carry chain", nm["plain_carry_chain_below_top"], nm["plain_top_nibble_neg8_chain"])]


@pytest.mark.parametrize("key", range(6))
@pytest.mark.parametrize("cid,cname", CURVES)
def test_extract_with_adversarial_key(cid, cname, key):
    """out = c.1 - a c.0 for 65 commitments (a full wave and one lane; identity components among them) under a key `a`
    from the table, endo = 1 (the key's GLV / GLS streams) and endo = 0 (its recode_w4 digits).  None of these keys is
    one that gs_crs_generate or gs_set_extraction_key may refuse: a refusal raises here with its status code."""
    import gs_oracle as O
    import gs_ref_py as ref
    import wirevec as V
    from test_gpu_extract import neg_point

    K = ctx(cid, cname)
    eng, r, ks = K.eng, K.r, K.ks
    label, a1, a2 = extract_keys(K)[key]
    rnd = random.Random(8400 + cid)
    Q = Keyed(K, a1, a2, rnd.randrange(2, r), rnd.randrange(2, r))
    eng.set_extraction_key(K.frs([a1, a2]))
    n = 65
    for group in (1, 2):
        a = Q.a[group]
        us = [0 if i % 11 == 5 else ks[(13 * i + 7 * key) % len(ks)] for i in range(n)]
        vs = [0 if i % 13 == 6 else ks[(17 * i + 3) % len(ks)] for i in range(n)]
        us[-1], vs[-1] = 1, a  # c.1 = a c.0: the identity out
        c0, c1 = K.muls(group, us), K.muls(group, vs)
        coms = np.concatenate([c0, c1], axis=1)
        want = np.stack([ref.g_add(cname, group, c1[i], neg_point(K.c, ref.g_mul(cname, group, c0[i], K.c.fr(a)), group))
                         for i in range(n)])
        assert not want[-1].any()
        V.setc(cname)
        F, g = V.fld(group), (K.oc.g1 if group == 1 else K.oc.g2)
        for i in (0, 5, 6, 33, 64):  # the big-integer oracle on a few lanes, the identity lanes among them
            pt = O.ec_add(F, O.ec_mul(F, vs[i], g), O.ec_neg(F, O.ec_mul(F, a, O.ec_mul(F, us[i], g))))
            assert (want[i] == np.asarray(V.point_limbs(cname, pt, group)).view(np.uint8)).all(), (label, group, i)
        for endo in (1, 0):
            eng.set_option("endo", endo)
            with profiled(eng) as prof:
                got = eng.extract(group, coms)
            assert prof.ran("k_extract.g%d%s" % (group, "" if endo else ".plain")), prof.names
            same(got, want, ["%s: key %s, group %d, endo %d, lane %d" % (cname, label, group, endo, i) for i in range(n)])
    eng.set_extraction_key(None)


# ---- 5. gt_pow_batch_dev (k_gt_pow) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_gt_pow_exponent_runs(cid, cname):
    """base^k for the exponent-run class (1 0^n 1 repeated, n = 0 .. 4: every length the lazy squaring chain of the bit
    loop can reach; a lone top bit; a lone bottom bit) and the universal class, on a golden pairing value."""
    import torch as T

    import gs_oracle as O
    import gs_ref_py as ref
    import scalarvec as S
    import wirevec as V

    K = ctx(cid, cname)
    eng, c = K.eng, K.c
    ks = S.scalars(cname, "exponent") + [k for k in S.scalars(cname, "universal") if k not in S.scalars(cname, "exponent")]
    gold = c.golden["pairing"][0]["out"]
    base = np.ascontiguousarray(c.f12(gold)).view(np.uint8)
    out = T.empty(len(ks) * eng.GT, dtype=T.uint8, device="cuda:0")
    with profiled(eng) as prof:
        eng.gt_pow_batch_dev(len(ks), T.from_numpy(base.copy()).to("cuda:0"),
                             T.from_numpy(K.frs(ks).reshape(-1).copy()).to("cuda:0"), out)
    assert prof.ran("k_gt_pow"), prof.names
    got = out.cpu().numpy().reshape(len(ks), eng.GT)
    want = np.stack([ref.gt_pow(cname, base, K.frs([k])) for k in ks])
    same(got, want, [K.name(k) for k in ks])
    V.setc(cname)
    f = O.f12_unflat([int(s, 16) for s in gold])
    for i in list(range(7)) + [7 + ks[7:].index(K.r - 1)]:  # the exponent class and r - 1 on the big-integer oracle
        assert (want[i] == np.asarray(V.gt_limbs(cname, O.f12_pow(f, ks[i]))).view(np.uint8)).all(), K.name(ks[i])


# ---- 6. prove and verify ------------------------------------------------------------------------------------------------
SHAPES = {
    "planned": {},
    "straus4w5x2": dict(var_tm=4, var_w=5, var_mo=2),
    "straus4": dict(var_tm=4, var_w=4, var_mo=1),
    "lanes": dict(var_tm=1),
    "plain": dict(endo=0),
}
SHAPE_KERNEL = {"straus4w5x2": "k_var_multi4w5x2.g?", "straus4": "k_var_multi4.g?", "lanes": "k_var.g?",
                "plain": "k_var.plain.g?"}
_PROVE_ENG = {}
PROVE_CASES = [(ty, "planned") for ty in (0, 1, 2, 3)] + [(0, s) for s in SHAPES if s != "planned"]


def table_workload(K, eng, ty, N, m, n):
    """A batch of true statements whose Gamma, R, S and T cycle through the table (the start moves with the type: the
    four types together cover it); variables and constants are seeded random multiples of the generators."""
    import torch as T

    from groth_sahai_rs_amd.workload import Workload

    wl = Workload(eng, ty=ty, N=N, m=m, n=n, seed=8500 + K.cid, corrupt_every=0)
    sh, r, ks = wl.sh, K.r, K.ks
    kx, ky = sh["kx"], sh["ky"]
    rnd = random.Random(8600 + 10 * K.cid + ty)
    draw = lambda cnt: [rnd.randrange(r) for _ in range(cnt)]
    pos = [192 * ty]

    def cycle(cnt):
        out = [ks[(pos[0] + i) % len(ks)] for i in range(cnt)]
        pos[0] += cnt
        return out

    xs, ys, as_, bs = draw(N * m), draw(N * n), draw(N * n), draw(N * m)
    gam = cycle(N * m * n)
    tg = []
    for e in range(N):
        s = sum(as_[e * n + j] * ys[e * n + j] for j in range(n)) + sum(xs[e * m + i] * bs[e * m + i] for i in range(m))
        s += sum(xs[e * m + i] * gam[(e * m + i) * n + j] * ys[e * n + j] for i in range(m) for j in range(n))
        tg.append(s % r)
    dev = wl.X.device
    fr_t = lambda vals: T.from_numpy(K.frs(vals).reshape(-1).copy()).to(dev)
    gens = {1: T.from_numpy(wl.g1_gen.copy()).to(dev), 2: T.from_numpy(wl.g2_gen.copy()).to(dev)}

    def elems(vals, group, isg):
        k = fr_t(vals)
        if not isg:
            return k
        out = T.empty(len(vals) * (eng.G1 if group == 1 else eng.G2), dtype=T.uint8, device=dev)
        eng.g_mul_batch_dev(group, len(vals), gens[group], True, k, out)
        return out

    wl.X, wl.A = elems(xs, 1, sh["xg"]), elems(as_, 1, sh["xg"])
    wl.Y, wl.B = elems(ys, 2, sh["yg"]), elems(bs, 2, sh["yg"])
    wl.Gamma = fr_t(gam)
    if ty == 0:
        wl.target = T.empty(N * eng.GT, dtype=T.uint8, device=dev)
        eng.gt_pow_batch_dev(N, T.from_numpy(wl.gt_gen.copy()).to(dev), fr_t(tg), wl.target)
    elif ty == 3:
        wl.target = fr_t(tg)
    else:
        wl.target = elems(tg, ty, True)
    wl.R, wl.S, wl.T = fr_t(cycle(N * m * kx)), fr_t(cycle(N * n * ky)), fr_t(cycle(N * ky * kx))
    eng.sync()
    return wl


@pytest.mark.parametrize("ty,shape", PROVE_CASES)
@pytest.mark.parametrize("cid,cname", CURVES)
def test_prove_and_verify_table_scalars(cid, cname, ty, shape):
    """2 x 2 equations of every type, N = 16, Gamma / R / S / T from the table: commitments, pi and theta of every
    equation against the reference's commit_and_prove, its verdict on them true, the engine's verdicts true -- planned,
    and (PPE) with the Straus lanes forced to 4-term groups at both window widths, to one term per lane and to the
    plain path; then the same proofs verified on shared per-base tables (var_tab = 1), which must accept."""
    import groth_sahai_rs_amd as gs
    import gs_ref_py as ref
    from gpubatch import oracle_check

    K = ctx(cid, cname)
    if cid not in _PROVE_ENG:
        _PROVE_ENG[cid] = gs.Engine(cid, 0)  # its own engine: the workload's CRS stays installed between the cases
    eng = _PROVE_ENG[cid]
    try:
        for key, val in SHAPES[shape].items():
            eng.set_option(key, val)
        N, m, n = 16, 2, 2
        wl = table_workload(K, eng, ty, N, m, n)
        with profiled(eng) as prof:
            wl.prove()
            wl.verify()
        if shape in SHAPE_KERNEL:
            assert prof.ran(SHAPE_KERNEL[shape]), (shape, prof.names)
        oracle_check(ref, cname, eng, wl, range(N))
        assert wl.ok.cpu().numpy().all()
        eng.set_option("var_tab", 1)
        wl.ok.zero_()
        with profiled(eng) as prof:
            wl.verify()
        # (endo = 0 keeps one plain lane per term: the shared tables are an endomorphism shape)
        assert prof.ran("k_var.plain.vg1" if shape == "plain" else "k_var_tab8.vg1"), prof.names
        assert wl.ok.cpu().numpy().all()
    finally:
        for key, val in (("endo", 1), ("var_tm", 0), ("var_w", 0), ("var_mo", 0), ("var_tab", 0)):
            eng.set_option(key, val)

"""gs_set_extraction_key / gs_extract_g1 / gs_extract_g2 on the GPU (include/gs_amd.h): whoever drew a1, a2 opens any
commitment, out = c.1 - a c.0.  Every test draws its own a1, a2, t1, t2 and builds the CRS with gs_crs_generate, so it
knows the key.  The big-integer oracle's plain point arithmetic is the reference for arbitrary Com pairs (the formula
is a map on all of Com); honest commitments must give back exactly what was committed (tests/test_extract_algebra.py
pins that on the oracle).  Counts 1, 64, 65, 130: one lane, a full wave, a partial second wave, several blocks."""
import os
import random
import sys

import numpy as np
import pytest

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu

CURVES = [(0, "bls12_381"), (1, "bn254")]
COUNTS = [1, 64, 65, 130]


class Keyed:
    """One engine per curve with a binding CRS whose key the test knows."""

    def __init__(self, cid, cname):
        import groth_sahai_rs_amd as gs
        import wirevec as V

        self.cid, self.cname, self.c = cid, cname, curve(cname)
        oc = V.setc(cname)
        self.r = oc.r
        rnd = random.Random(7100 + cid)
        self.a1, self.a2, self.t1, self.t2 = (rnd.randrange(2, oc.r) for _ in range(4))
        self.p1 = V.point_limbs(cname, oc.g1, 1)
        self.p2 = V.point_limbs(cname, oc.g2, 2)
        self.eng = gs.Engine(cid, 0)
        sc = self.frs([self.a1, self.a2, self.t1, self.t2])
        self.crs = self.eng.crs_generate(self.p1, self.p2, sc)
        self.crs_hiding = self.eng.crs_generate(self.p1, self.p2, sc, hiding=True)
        self.key = self.frs([self.a1, self.a2])
        self.eng.set_crs(self.crs)
        self.eng.set_extraction_key(self.key)

    def frs(self, vals):
        """Montgomery limbs of canonical scalars"""
        if len(vals) == 0:
            return np.zeros(0, dtype=np.uint64)
        return np.concatenate([self.c.fr(v % self.r) for v in vals])

    def a(self, group):
        return self.a1 if group == 1 else self.a2

    def t(self, group):
        return self.t1 if group == 1 else self.t2

    def gen(self, group):
        return self.p1 if group == 1 else self.p2

    def mul_gen(self, group, ks):
        """[k] generator for every k, on the engine"""
        return self.eng.g_mul_batch(group, self.gen(group), self.frs(ks), broadcast=True)


_K = {}


def keyed(cid, cname):
    if cid not in _K:
        _K[cid] = Keyed(cid, cname)
    K = _K[cid]
    K.eng.set_option("endo", 1)
    return K


def with_endo(K, endo, fn):
    K.eng.set_option("endo", endo)
    try:
        return fn()
    finally:
        K.eng.set_option("endo", 1)


def neg_point(c, pt, group):
    """-P on boundary limbs (y -> p - y; the identity stays all zero)"""
    a = np.asarray(pt).view(np.uint64).reshape(-1, c.nq).copy()
    if not a.any():
        return a.reshape(-1).view(np.uint8)
    h = a.shape[0] // 2
    for i in range(h, 2 * h):
        a[i] = c.fq((-c.fq_dec(a[i])) % c.p)
    return a.reshape(-1).view(np.uint8)


# ---- 1. round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("endo", [1, 0])
@pytest.mark.parametrize("count", COUNTS)
def test_round_trip(cid, cname, endo, count):
    K = keyed(cid, cname)
    eng = K.eng
    rnd = random.Random(100 * count + 10 * cid + endo)
    fr = lambda n: [rnd.randrange(K.r) for _ in range(n)]
    xs, ys = fr(count), fr(count)
    X, Y = K.mul_gen(1, xs), K.mul_gen(2, ys)  # also g_mul_batch(gen, x, broadcast=True), the image of a scalar x

    def run():
        c1 = eng.commit("g1", X, K.frs(fr(2 * count)))
        c2 = eng.commit("g2", Y, K.frs(fr(2 * count)))
        assert (eng.extract(1, c1) == X).all() and (eng.extract(2, c2) == Y).all()
        s1 = eng.commit("fr_b1", K.frs(xs), K.frs(fr(count)))
        s2 = eng.commit("fr_b2", K.frs(ys), K.frs(fr(count)))
        assert (eng.extract(1, s1) == X).all() and (eng.extract(2, s2) == Y).all()

    with_endo(K, endo, run)


# ---- 2. arbitrary Com pairs against the oracle ------------------------------------------------------------------------
_POOL = {}


def pool(K, group):
    """130 pairs of unrelated subgroup points (two arithmetic progressions with random starts and steps) and the
    oracle's c1 - a c0 for each, computed once per (curve, group)."""
    import gs_oracle as O
    import wirevec as V

    key = (K.cid, group)
    if key not in _POOL:
        oc = V.setc(K.cname)
        F = V.fld(group)
        g = oc.g1 if group == 1 else oc.g2
        rnd = random.Random(4300 + 10 * K.cid + group)
        s0, d0, s1, d1 = (O.ec_mul(F, rnd.randrange(2, oc.r), g) for _ in range(4))
        coms, want = [], []
        c0, c1 = s0, s1
        for _ in range(max(COUNTS)):
            coms.append(np.concatenate([V.point_limbs(K.cname, c0, group), V.point_limbs(K.cname, c1, group)]))
            w = O.ec_add(F, c1, O.ec_neg(F, O.ec_mul(F, K.a(group), c0)))
            want.append(V.point_limbs(K.cname, w, group))
            c0, c1 = O.ec_add(F, c0, d0), O.ec_add(F, c1, d1)
        _POOL[key] = (np.stack(coms).view(np.uint8), np.stack(want).view(np.uint8))
    return _POOL[key]


@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("count", COUNTS)
def test_arbitrary_pairs_match_the_oracle(cid, cname, group, count):
    K = keyed(cid, cname)
    coms, want = pool(K, group)
    got1 = K.eng.extract(group, coms[:count])
    got0 = with_endo(K, 0, lambda: K.eng.extract(group, coms[:count]))
    bad = np.nonzero((got1 != want[:count]).any(axis=1))[0]
    assert bad.size == 0, ("endo=1", bad[:8])
    bad = np.nonzero((got0 != want[:count]).any(axis=1))[0]
    assert bad.size == 0, ("endo=0", bad[:8])
    assert (got0 == got1).all()  # identical bytes on subgroup inputs


# ---- 3. edge lanes inside a wave of ordinary lanes --------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("endo", [1, 0])
def test_edge_lanes(cid, cname, group, endo):
    K = keyed(cid, cname)
    eng, r, a, t = K.eng, K.r, K.a(group), K.t(group)
    n = 64
    rnd = random.Random(900 + 10 * cid + group)
    xs = [rnd.randrange(1, r) for _ in range(n)]
    rr = [[rnd.randrange(1, r), rnd.randrange(1, r)] for _ in range(n)]
    rho = lambda i: (rr[i][0] + rr[i][1] * t) % r
    ZERO_RAND, X_INF, DOUBLING, C1_INF, BOTH_INF = 5, 17, 30, 44, 63
    rr[ZERO_RAND] = [0, 0]  # c = (O, X)
    xs[X_INF] = 0  # X = O: the result is the identity
    xs[DOUBLING] = (-2 * a * rho(DOUBLING)) % r  # c.1 = -a c.0: the subtraction is a doubling
    xs[C1_INF] = (-a * rho(C1_INF)) % r  # c.1 = O, c.0 != O
    xs[BOTH_INF], rr[BOTH_INF] = 0, [0, 0]
    X = K.mul_gen(group, xs)
    pt = X.shape[1]

    def run():
        c = eng.commit("g1" if group == 1 else "g2", X, K.frs([v for row in rr for v in row]))
        c0, c1 = c[:, :pt], c[:, pt:]
        # the lanes really are the edge cases they are meant to be
        assert not c0[ZERO_RAND].any() and c1[ZERO_RAND].any()
        assert not c0[BOTH_INF].any() and not c1[BOTH_INF].any()
        assert c0[C1_INF].any() and not c1[C1_INF].any()
        ac0 = eng.g_mul_batch(group, c0[DOUBLING].copy(), K.frs([a]))[0]
        assert (neg_point(K.c, ac0, group) == c1[DOUBLING]).all() and c1[DOUBLING].any()
        got = eng.extract(group, c)
        bad = np.nonzero((got != X).any(axis=1))[0]
        assert bad.size == 0, bad
        assert not got[X_INF].any() and not got[BOTH_INF].any()  # the identity is all-zero bytes
        assert got[DOUBLING].any() and got[C1_INF].any()

    with_endo(K, endo, run)


# ---- 4. endo = 0 on curve points outside the subgroup -----------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", [(0, "bls12_381", 1), (0, "bls12_381", 2), (1, "bn254", 2)])
def test_plain_path_outside_the_subgroup(cid, cname, group):
    import gs_oracle as O
    import wirevec as V

    K = keyed(cid, cname)
    tq = V.cofactor_points(cname, group)
    assert tq, "no cofactor points"
    oc = V.setc(cname)
    F = V.fld(group)
    g = oc.g1 if group == 1 else oc.g2
    rnd = random.Random(5500 + 10 * cid + group)
    S = [O.ec_mul(F, rnd.randrange(2, oc.r), g) for _ in range(2)]
    pairs = []
    for q, T in sorted(tq.items()):
        mixed = O.ec_add(F, S[0], T)  # of order q r
        assert O.ec_mul(F, oc.r, mixed) is not None
        pairs += [(T, S[1]), (mixed, O.ec_add(F, S[1], T)), (S[0], T), (mixed, None), (T, T)]
    pairs.append((S[0], S[1]))
    lim = lambda p: V.point_limbs(cname, p, group)
    coms = np.stack([np.concatenate([lim(c0), lim(c1)]) for c0, c1 in pairs]).view(np.uint8)
    want = np.stack([lim(O.ec_add(F, c1, O.ec_neg(F, O.ec_mul(F, K.a(group), c0)))) for c0, c1 in pairs]).view(np.uint8)
    got = with_endo(K, 0, lambda: K.eng.extract(group, coms))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad


# ---- 5. key handling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_key_handling(cid, cname):
    import groth_sahai_rs_amd as gs

    K = keyed(cid, cname)
    coms, want = pool(K, 1)
    coms, want = coms[:3], want[:3]
    e = gs.Engine(cid, 0)
    try:
        def refused(fn, code=3):
            with pytest.raises(gs.GsError) as ei:
                fn()
            assert ei.value.code == code, str(ei.value)
            return str(ei.value)

        refused(lambda: e.set_extraction_key(K.key), code=4)  # no CRS yet
        e.set_crs(K.crs)
        refused(lambda: e.extract(1, coms))  # no key yet
        assert "u[0]" in refused(lambda: e.set_extraction_key(K.frs([K.a1 + 1, K.a2])))  # wrong a1
        refused(lambda: e.extract(1, coms))  # a refused key installs nothing
        assert "v[0]" in refused(lambda: e.set_extraction_key(K.frs([K.a1, K.a2 + 1])))  # wrong a2
        e.set_extraction_key(K.key)
        assert (e.extract(1, coms) == want).all()
        # count = 0 is a no-op
        assert e.extract(1, np.zeros(0, dtype=np.uint8)).shape == (0, e.G1)
        assert e.extract(2, np.zeros(0, dtype=np.uint8)).shape == (0, e.G2)
        # a refused key also removes the one that was installed
        refused(lambda: e.set_extraction_key(K.frs([K.a1, K.a2 + 1])))
        refused(lambda: e.extract(1, coms))
        e.set_extraction_key(K.key)
        e.set_crs(K.crs)  # gs_set_crs clears the key
        refused(lambda: e.extract(1, coms))
        e.set_extraction_key(K.key)
        assert (e.extract(1, coms) == want).all()
        e.set_extraction_key(None)  # NULL clears the key
        refused(lambda: e.extract(2, np.zeros(e.COM2, dtype=np.uint8)))
        # the right key on the hiding CRS: u[1].1 = t a p - p binds nothing
        e.set_crs(K.crs_hiding)
        assert "u[1]" in refused(lambda: e.set_extraction_key(K.key))
        refused(lambda: e.extract(1, coms))
    finally:
        e.close()


# ---- 6. prove -> rerandomize -> extract -------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty,m,n", [(0, 4, 4), (3, 2, 3)])
def test_extract_after_rerandomization(cid, cname, ty, m, n):
    import torch

    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.workload import Workload

    K = keyed(cid, cname)
    N = 65
    e = gs.Engine(cid, 0)
    try:
        wl = Workload(e, ty=ty, N=N, m=m, n=n, seed=616 + ty, corrupt_every=0)
        # the same generators under a CRS whose key the test knows (targets do not depend on a, t)
        crs = e.crs_generate(wl.g1_gen, wl.g2_gen, K.frs([K.a1, K.a2, K.t1, K.t2]))
        e.set_crs(crs)
        wl.crs = crs
        e.set_extraction_key(K.key)
        wl.prove()
        rnd = random.Random(77 + ty)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
        fresh = lambda t: dev(K.frs([rnd.randrange(K.r) for _ in range(t.numel() // 32)]))
        out = [torch.empty_like(t) for t in (wl.xcoms, wl.ycoms, wl.pi, wl.theta)]
        e.rerandomize_batch_dev(ty, N, m, n, wl.A, wl.B, wl.Gamma, wl.xcoms, wl.ycoms, wl.pi, wl.theta, fresh(wl.R),
                                fresh(wl.S), fresh(wl.T), *out)
        assert not (out[0] == wl.xcoms).all()
        ok = torch.empty(N, dtype=torch.uint8, device="cuda:0")
        e.verify_batch_dev(ty, N, m, n, wl.A, wl.B, wl.Gamma, wl.target, *out, ok)
        gx = torch.empty(N * m * e.G1, dtype=torch.uint8, device="cuda:0")
        gy = torch.empty(N * n * e.G2, dtype=torch.uint8, device="cuda:0")
        e.extract_dev(1, out[0], gx)
        e.extract_dev(2, out[1], gy)
        e.sync()
        assert ok.cpu().numpy().all()
        if ty == 0:
            wx, wy = wl.X, wl.Y
        else:  # scalar witnesses come back as their images
            wx, wy = torch.empty_like(gx), torch.empty_like(gy)
            e.g_mul_batch_dev(1, N * m, dev(wl.g1_gen), True, wl.X, wx)
            e.g_mul_batch_dev(2, N * n, dev(wl.g2_gen), True, wl.Y, wy)
            e.sync()
        assert (gx == wx).all() and (gy == wy).all()
        if ty == 0:
            # the extracted witness satisfies the equation: prod e(A_j, Y_j) e(X_i, B_i) e(X_i, gamma_ij Y_j) = target
            X3, Y3 = gx.view(N, m, 1, e.G1), gy.view(N, 1, n, e.G2)
            Yt = Y3.expand(N, m, n, e.G2).contiguous()
            GY = torch.empty_like(Yt)
            e.g_mul_batch_dev(2, N * m * n, Yt, False, wl.Gamma, GY)
            P = torch.cat([wl.A.view(N, n, e.G1), gx.view(N, m, e.G1), X3.expand(N, m, n, e.G1).reshape(N, m * n, e.G1)],
                          dim=1).contiguous()
            Q = torch.cat([gy.view(N, n, e.G2), wl.B.view(N, m, e.G2), GY.view(N, m * n, e.G2)], dim=1).contiguous()
            gt = torch.empty(N * e.GT, dtype=torch.uint8, device="cuda:0")
            e.multi_pairing_batch_dev(N, n + m + m * n, P, Q, gt)
            e.sync()
            assert (gt == wl.target).all()
    finally:
        e.close()


# ---- 7. host and _dev forms, profile names ----------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_host_and_dev_forms_agree_and_are_profiled(cid, cname):
    import torch

    K = keyed(cid, cname)
    eng = K.eng
    eng.prof_enable(True)
    try:
        for group in (1, 2):
            coms, want = pool(K, group)
            coms, want = coms[:65], want[:65]
            for endo, name in ((1, "k_extract.g%d" % group), (0, "k_extract.g%d.plain" % group)):
                def run():
                    eng.prof_reset()
                    d = torch.from_numpy(coms.reshape(-1).copy()).to("cuda:0")
                    o = torch.empty(want.size, dtype=torch.uint8, device="cuda:0")
                    eng.extract_dev(group, d, o)
                    eng.sync()
                    names = {nm: n for nm, _, n in eng.prof_get()}
                    assert names.get(name) == 1, (name, names)
                    host = eng.extract(group, coms)
                    assert (o.cpu().numpy().reshape(host.shape) == host).all() and (host == want).all()
                    # an output that overlaps the input is refused, not computed
                    import groth_sahai_rs_amd as gs

                    with pytest.raises(gs.GsError) as ei:
                        eng.extract_dev(group, d, d[:want.size])
                    assert ei.value.code == 3

                with_endo(K, endo, run)
    finally:
        eng.prof_enable(False)


# ---- 8. the mirror layer ----------------------------------------------------------------------------------------------
class _Rng:
    def __init__(self, c, seed):
        self.c, self.rnd = c, random.Random(seed)

    def fr(self):
        return self.c.fr(self.rnd.randrange(self.c.r))


@pytest.mark.parametrize("cid,cname", CURVES)
def test_mirror_generate_with_key_and_extract(cid, cname):
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd import mirror as M

    K = keyed(cid, cname)
    plain = M.generate_crs(K.p1, K.p2, _Rng(K.c, 5), cid)
    crs, key = M.generate_crs_with_key(K.p1, K.p2, _Rng(K.c, 5), cid)
    try:
        for a, b in zip(plain.u + plain.v + [plain.g1_gen, plain.g2_gen, plain.gt_gen],
                        crs.u + crs.v + [crs.g1_gen, crs.g2_gen, crs.gt_gen]):
            assert (a == b).all()  # the same draws: the same CRS
        rng = _Rng(K.c, 6)
        xs = [3, 0, 12345]
        X = [x.view(np.uint64).copy() for x in K.mul_gen(1, xs)]
        Y = [y.view(np.uint64).copy() for y in K.mul_gen(2, xs)]
        for got, want in ((M.extract(M.batch_commit_G1(X, crs, rng), crs, key), X),
                          (M.extract(M.batch_commit_G2(Y, crs, rng), crs, key), Y),
                          (M.extract(M.batch_commit_scalar_to_B1([K.c.fr(x) for x in xs], crs, rng), crs, key), X),
                          (M.extract(M.batch_commit_scalar_to_B2([K.c.fr(x) for x in xs], crs, rng), crs, key), Y)):
            assert len(got) == len(want) and all((g == w).all() for g, w in zip(got, want))
        assert M.extract(M.Commit1([], []), crs, key) == []
        hid, hkey = M.generate_crs_with_key(K.p1, K.p2, _Rng(K.c, 5), cid, hiding=True)
        try:
            with pytest.raises(gs.GsError) as ei:
                M.extract(M.batch_commit_G1(X, hid, rng), hid, hkey)
            assert ei.value.code == 3
        finally:
            hid.engine.close()
    finally:
        plain.engine.close()
        crs.engine.close()

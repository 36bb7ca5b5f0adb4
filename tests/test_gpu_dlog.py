"""gs_dlog_prepare / gs_dlog_g1 / gs_dlog_g2 / gs_extract_scalar_b1 / _b2 on the GPU (include/gs_amd.h): bounded discrete
logarithms by baby-step giant-step.  Every test knows every x by construction: the points are x * generator from
Engine.g_mul_batch(..., broadcast=True), which the existing suite holds to the oracle, and a handful per test come
from the big-integer oracle's ec_mul directly.  With a table of B = 2^log2_table baby steps the stride of the walk is
S = 2 B and its centres are B + t S."""
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


class Keyed:
    """One engine per curve with a binding CRS whose key the test knows (as tests/test_gpu_extract.py builds its own)."""

    def __init__(self, cid, cname):
        import groth_sahai_rs_amd as gs
        import wirevec as V

        self.cid, self.cname, self.c = cid, cname, curve(cname)
        self.oc = V.setc(cname)
        self.r = self.oc.r
        rnd = random.Random(8200 + cid)
        self.a1, self.a2, self.t1, self.t2 = (rnd.randrange(2, self.r) for _ in range(4))
        self.p1 = V.point_limbs(cname, self.oc.g1, 1)
        self.p2 = V.point_limbs(cname, self.oc.g2, 2)
        self.eng = gs.Engine(cid, 0)
        self.crs = self.eng.crs_generate(self.p1, self.p2, self.frs([self.a1, self.a2, self.t1, self.t2]))
        self.key = self.frs([self.a1, self.a2])
        self.eng.set_crs(self.crs)
        self.eng.set_extraction_key(self.key)

    def frs(self, vals):
        """Montgomery limbs of canonical scalars"""
        if len(vals) == 0:
            return np.zeros(0, dtype=np.uint64)
        return np.concatenate([self.c.fr(v % self.r) for v in vals])

    def fr_bytes(self, vals):
        return self.frs(vals).view(np.uint8).reshape(len(vals), 32)

    def gen(self, group):
        return self.p1 if group == 1 else self.p2

    def mul_gen(self, group, ks):
        """[k] generator for every k, on the engine"""
        return self.eng.g_mul_batch(group, self.gen(group), self.frs(ks), broadcast=True)

    def oracle_mul(self, group, k):
        """[k] generator on the big-integer oracle, as boundary bytes"""
        import gs_oracle as O
        import wirevec as V

        V.setc(self.cname)
        pt = O.ec_mul(V.fld(group), k % self.r, self.oc.g1 if group == 1 else self.oc.g2)
        return np.asarray(V.point_limbs(self.cname, pt, group)).view(np.uint8).reshape(-1)

    def points(self, group, xs, oracle=3):
        """x * generator for every x; the first `oracle` of them from the oracle instead of the engine"""
        pts = self.mul_gen(group, xs).copy()
        for i in range(min(oracle, len(xs))):
            o = self.oracle_mul(group, xs[i])
            assert (pts[i] == o).all()
            pts[i] = o
        return pts


_K = {}


def keyed(cid, cname):
    if cid not in _K:
        _K[cid] = Keyed(cid, cname)
    K = _K[cid]
    for k in ("dlog_steps", "dlog_fp_bits"):
        K.eng.set_option(k, 0)
    K.eng.set_option("endo", 1)
    return K


def check(K, xs, bits, out, found):
    """found is exactly the in-range mask, out the committed bytes where found and zero elsewhere"""
    inr = [0 <= x % K.r < (1 << bits) for x in xs]
    assert found.tolist() == [1 if v else 0 for v in inr], (found.tolist(), inr)
    want = K.fr_bytes([x if v else 0 for x, v in zip(xs, inr)])
    assert (out == want).all()


# ---- 1. exhaustive small range ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_exhaustive_small_range(cid, cname, group):
    """log2_table = 3, bits = 9: every x in [0, 512) -- every offset inside a stride, every centre, block boundaries,
    waves whose lanes finish at different steps -- in one launch, in many launches, and with 3-bit fingerprints."""
    K = keyed(cid, cname)
    eng = K.eng
    xs = list(range(512))
    pts = K.points(group, xs)
    eng.dlog_prepare(group, K.gen(group), 3)
    runs = []
    try:
        for opt, val in ((None, 0), ("dlog_steps", 4), ("dlog_fp_bits", 3)):
            if opt:
                eng.set_option(opt, val)
            out, found = eng.dlog(group, pts, 9)
            if opt:
                eng.set_option(opt, 0)
            check(K, xs, 9, out, found)
            runs.append(out.tobytes() + found.tobytes())
    finally:
        eng.set_option("dlog_steps", 0)
        eng.set_option("dlog_fp_bits", 0)
    assert runs[0] == runs[1] == runs[2]


# ---- 2. not in range ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_not_in_range(cid, cname, group):
    K = keyed(cid, cname)
    eng = K.eng
    bits, S, r = 9, 16, K.r
    rnd = random.Random(310 + 10 * cid + group)
    big = rnd.getrandbits(250) % r
    assert big >= (1 << bits)
    outside = [1 << bits, (1 << bits) + 1, (1 << bits) + S - 1, r - 1, r - 2, r - (1 << bits), big]
    xs = outside + [0] + [rnd.randrange(1 << bits) for _ in range(64 - len(outside) - 1)]  # 0: the identity
    order = list(range(64))
    rnd.shuffle(order)
    xs = [xs[i] for i in order]
    pts = K.points(group, xs)
    assert not pts[xs.index(0)].any()
    eng.dlog_prepare(group, K.gen(group), 3)
    for fp in (0, 3):
        eng.set_option("dlog_fp_bits", fp)
        try:
            out, found = eng.dlog(group, pts, bits)
        finally:
            eng.set_option("dlog_fp_bits", 0)
        check(K, xs, bits, out, found)
        # -1 and -2 have the x coordinate of the table entries 1 and 2: only the confirmation refuses them
        for v in (r - 1, r - 2):
            i = xs.index(v)
            assert found[i] == 0 and not out[i].any()


# ---- 3. range shorter than a stride ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_range_shorter_than_a_stride(cid, cname, group):
    K = keyed(cid, cname)
    xs = list(range(32))
    pts = K.points(group, xs)
    K.eng.dlog_prepare(group, K.gen(group), 4)
    out, found = K.eng.dlog(group, pts, 3)
    check(K, xs, 3, out, found)
    assert found.tolist() == [1] * 8 + [0] * 24


# ---- 4. counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_counts(cid, cname, group, count):
    K = keyed(cid, cname)
    rnd = random.Random(400 + count)
    xs = [rnd.randrange(1 << 12) for _ in range(count)]
    if count > 2:
        xs[1], xs[-1] = 0, (1 << 12) - 1
    pts = K.points(group, xs, oracle=1)
    K.eng.dlog_prepare(group, K.gen(group), 4)
    out, found = K.eng.dlog(group, pts, 12)
    assert found.tolist() == [1] * count
    check(K, xs, 12, out, found)


# ---- 5. the base is used -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_the_base_is_used(cid, cname, group):
    K = keyed(cid, cname)
    eng = K.eng
    ys = list(range(40))
    on = K.points(group, [5 * y for y in ys])
    off = K.points(group, [5 * y + 1 for y in ys])
    base5 = K.mul_gen(group, [5])[0]
    eng.dlog_prepare(group, base5, 3)
    out, found = eng.dlog(group, on, 8)
    check(K, ys, 8, out, found)
    assert found.all()
    out, found = eng.dlog(group, off, 8)
    assert not found.any() and not out.any()
    eng.dlog_prepare(group, K.gen(group), 3)  # replaces the table
    out, found = eng.dlog(group, on, 8)
    check(K, [5 * y for y in ys], 8, out, found)
    assert found.all()


# ---- 6. a realistic walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", [(0, "bls12_381", 1), (0, "bls12_381", 2), (1, "bn254", 1)])
def test_realistic_walk(cid, cname, group):
    """bits = 32 over a 2^16 table: 2^15 giant steps for the lanes that find nothing"""
    K = keyed(cid, cname)
    rnd = random.Random(600 + 10 * cid + group)
    xs = [0, 1, 1 << 31, (1 << 32) - 1, 1 << 32] + [rnd.randrange(1 << 32) for _ in range(60)]
    pts = K.points(group, xs, oracle=5)
    K.eng.dlog_prepare(group, K.gen(group), 16)
    out, found = K.eng.dlog(group, pts, 32)
    check(K, xs, 32, out, found)
    assert found.tolist() == [1, 1, 1, 1, 0] + [1] * 60


# ---- 7. cofactor / mixed-order inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", [(0, "bls12_381", 1), (0, "bls12_381", 2), (1, "bn254", 2)])
def test_points_outside_the_subgroup(cid, cname, group):
    import gs_oracle as O
    import wirevec as V

    K = keyed(cid, cname)
    tq = V.cofactor_points(cname, group)
    assert tq
    V.setc(cname)
    F = V.fld(group)
    g = K.oc.g1 if group == 1 else K.oc.g2
    rnd = random.Random(700 + group)
    pts, xs = [], []
    for q, t in sorted(tq.items()):
        pts.append(t)  # order q alone
        for x in (0, 1, 8, 24, rnd.randrange(512)):  # x G + T_q: in range but for the cofactor component
            pts.append(O.ec_add(F, O.ec_mul(F, x, g), t) if x else t)
    honest = [rnd.randrange(512) for _ in range(3)]
    arr = np.stack([np.asarray(V.point_limbs(cname, p, group)).view(np.uint8).reshape(-1) for p in pts] +
                   [K.oracle_mul(group, x) for x in honest])
    K.eng.dlog_prepare(group, K.gen(group), 3)
    for fp in (0, 3):
        K.eng.set_option("dlog_fp_bits", fp)
        try:
            out, found = K.eng.dlog(group, arr, 9)
        finally:
            K.eng.set_option("dlog_fp_bits", 0)
        assert found.tolist() == [0] * len(pts) + [1] * 3
        assert not out[:len(pts)].any() and (out[len(pts):] == K.fr_bytes(honest)).all()


# ---- 8. extract_scalar --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
@pytest.mark.parametrize("endo", [1, 0])
def test_extract_scalar(cid, cname, group, endo):
    K = keyed(cid, cname)
    eng = K.eng
    rnd = random.Random(800 + 10 * cid + group)
    xs = [0, 1, (1 << 16) - 1] + [rnd.randrange(1 << 16) for _ in range(62)] + [rnd.getrandbits(200) | (1 << 199)]
    kind = "fr_b1" if group == 1 else "fr_b2"
    eng.dlog_prepare(group, K.gen(group), 8)
    eng.set_option("endo", endo)
    try:
        coms = eng.commit(kind, K.frs(xs), K.frs([rnd.randrange(K.r) for _ in xs]))
        out, found = eng.extract_scalar(group, coms, 16)
        out2, found2 = eng.dlog(group, eng.extract(group, coms), 16)
    finally:
        eng.set_option("endo", 1)
    assert found.tolist() == [1] * 65 + [0]
    check(K, xs, 16, out, found)  # exactly the committed Fr bytes
    assert (out == out2).all() and (found == found2).all()


# ---- 9. forms, names, refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_host_and_dev_forms_profile_names(cid, cname, group):
    import torch

    import groth_sahai_rs_amd as gs

    K = keyed(cid, cname)
    eng = K.eng
    rnd = random.Random(900 + group)
    xs = [rnd.randrange(600) for _ in range(65)]
    pts = K.points(group, xs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    eng.prof_enable(True)
    try:
        eng.prof_reset()
        eng.dlog_prepare(group, K.gen(group), 3)
        names = {nm: n for nm, _, n in eng.prof_get()}
        assert names.get("k_dlog_table.g%d" % group) == 1, names
        eng.set_option("dlog_steps", 4)  # 2^9 / 16 = 32 centres: 8 launches
        eng.prof_reset()
        d, o, f = dev(pts), torch.empty(65 * 32, dtype=torch.uint8, device="cuda:0"), torch.empty(65, dtype=torch.uint8,
                                                                                                 device="cuda:0")
        eng.dlog_dev(group, d, 9, o, f)
        eng.sync()
        names = {nm: n for nm, _, n in eng.prof_get()}
        assert names.get("k_dlog.g%d" % group) == 8, names
        eng.set_option("dlog_steps", 0)
        eng.prof_reset()
        out, found = eng.dlog(group, pts, 9)
        names = {nm: n for nm, _, n in eng.prof_get()}
        assert names.get("k_dlog.g%d" % group) == 1, names
    finally:
        eng.set_option("dlog_steps", 0)
        eng.prof_enable(False)
    check(K, xs, 9, out, found)
    assert (o.cpu().numpy().reshape(65, 32) == out).all() and (f.cpu().numpy() == found).all()
    # the extraction forms
    kind = "fr_b1" if group == 1 else "fr_b2"
    coms = eng.commit(kind, K.frs(xs), K.frs([rnd.randrange(K.r) for _ in xs]))
    eout, efound = eng.extract_scalar(group, coms, 9)
    dc = dev(coms)
    eng.extract_scalar_dev(group, dc, 9, o, f)
    eng.sync()
    assert (o.cpu().numpy().reshape(65, 32) == eout).all() and (f.cpu().numpy() == efound).all()
    check(K, xs, 9, eout, efound)
    # overlapping outputs are refused, not computed
    for args in ((d, 9, d[:65 * 32], f), (d, 9, o, d[32:32 + 65]), (d, 9, o, o[64:64 + 65])):
        with pytest.raises(gs.GsError) as ei:
            eng.dlog_dev(group, *args)
        assert ei.value.code == 3
    with pytest.raises(gs.GsError) as ei:
        eng.extract_scalar_dev(group, dc, 9, dc[:65 * 32], f)
    assert ei.value.code == 3
    # count = 0
    out0, found0 = eng.dlog(group, np.zeros(0, dtype=np.uint8), 9)
    assert out0.shape == (0, 32) and found0.shape == (0,)
    out0, found0 = eng.extract_scalar(group, np.zeros(0, dtype=np.uint8), 9)
    assert out0.shape == (0, 32) and found0.shape == (0,)


@pytest.mark.parametrize("cid,cname,group", CG)
def test_refusals(cid, cname, group):
    import groth_sahai_rs_amd as gs

    K = keyed(cid, cname)
    pts = K.mul_gen(group, [5, 6])

    def refused(fn, needle=None):
        with pytest.raises(gs.GsError) as ei:
            fn()
        assert ei.value.code == 3, str(ei.value)
        if needle:
            assert needle in str(ei.value), str(ei.value)

    e = gs.Engine(cid, 0)
    try:
        refused(lambda: e.dlog(group, pts, 8), "gs_dlog_prepare")  # no table
        refused(lambda: e.dlog_prepare(group, np.zeros_like(K.gen(group)), 3), "identity")
        refused(lambda: e.dlog_prepare(group, K.gen(group), 1))
        refused(lambda: e.dlog_prepare(group, K.gen(group), 29))
        refused(lambda: e.dlog(group, pts, 8))  # the refused prepares left no table
        e.dlog_prepare(group, K.gen(group), 3)
        refused(lambda: e.dlog(group, pts, 0))
        refused(lambda: e.dlog(group, pts, 49))
        refused(lambda: e.dlog(group, pts, 3 + 26), "log2_table >= 4")
        out, found = e.dlog(group, pts, 8)
        assert found.tolist() == [1, 1]
        # extraction needs the key
        e.set_crs(K.crs)
        coms = K.eng.commit("fr_b1" if group == 1 else "fr_b2", K.frs([5]), K.frs([9]))
        refused(lambda: e.extract_scalar(group, coms, 8), "gs_set_extraction_key")
        e.set_extraction_key(K.key)
        out, found = e.extract_scalar(group, coms, 8)
        assert found.tolist() == [1] and (out == K.fr_bytes([5])).all()
        e.set_crs(K.crs)  # forgets the key, keeps the table (public data)
        refused(lambda: e.extract_scalar(group, coms, 8), "gs_set_extraction_key")
        out, found = e.dlog(group, pts, 8)
        assert found.tolist() == [1, 1] and (out == K.fr_bytes([5, 6])).all()
    finally:
        e.close()


# ---- 10. the mirror layer -----------------------------------------------------------------------------------------------
class _Rng:
    def __init__(self, c, seed):
        self.c, self.rnd = c, random.Random(seed)

    def fr(self):
        return self.c.fr(self.rnd.randrange(self.c.r))


@pytest.mark.parametrize("cid,cname", CURVES)
def test_mirror_extract_scalars(cid, cname):
    from groth_sahai_rs_amd import mirror as M

    K = keyed(cid, cname)
    crs, key = M.generate_crs_with_key(K.p1, K.p2, _Rng(K.c, 5), cid)
    try:
        rng = _Rng(K.c, 6)
        xs = [3, 0, 12345, (1 << 16) - 1, 1 << 16]
        sc = [K.c.fr(x) for x in xs]
        for commit in (M.batch_commit_scalar_to_B1(sc, crs, rng), M.batch_commit_scalar_to_B2(sc, crs, rng)):
            got = M.extract_scalars(commit, crs, key, 16)
            assert len(got) == 5 and got[4] is None
            assert all((g == w).all() for g, w in zip(got[:4], sc[:4]))
            got = M.extract_scalars(commit, crs, key, 17, log2_table=5)  # another table: prepared again
            assert all((g == w).all() for g, w in zip(got, sc))
        assert M.extract_scalars(M.Commit1([], []), crs, key, 16) == []
    finally:
        crs.engine.close()

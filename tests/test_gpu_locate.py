"""gs_verify_batch_rlc_locate[_dev] against the oracle.

The expectation is never a constant of this file: for every entry the pair (W_e, T_e) is computed from the oracle's cells
exactly as test_gpu_soundness.oracle_rlc's `entry` does (W_e = prod_c Q[e][c]^rho[e][c], T_e = target_e^rho[e][3] for PPE,
one otherwise), the tree of products is formed with ref.gt_mul, and tests/locatevec.py descends it.  ok, info[0] and
info[1] must equal the model's, bit for bit and count for count; acc must equal gs_verify_batch_rlc_dev's, byte for byte;
the host and the device entry must agree.  rho comes from a seeded generator (a test of arithmetic; the CSPRNG contract
of the header is about production) without edge rows, so that no two faults cancel by accident: for such rho ok is also
required to equal the oracle's exact verdicts, once W_e != T_e is confirmed for every rejected entry.

Cancellation, case (c): a z | 1/z pair in two neighbouring LEAF groups (entries 7 and 8, K = 8) with a third fault at
entry 100 is reported by the model -- and by the device -- as entry 100 alone: node (2, 0) holds entries 0 .. 63, both
halves of the pair, and passes.  The pair is reached only when the split goes up to a failing node: entries 63 and 64
(case c2) lie under two different children of the root, and all three faults are reported."""
import numpy as np
import pytest

import forge
import locatevec
from gpubatch import pool
from gsutil import curve
from test_gpu_soundness import Batch, dev, drawn_equation, engine, full_batch, gt_one, interleave, valid_batch

pytestmark = pytest.mark.gpu

CURVES = [("bls12_381", 0), ("bn254", 1)]
TYPES = [0, 1, 2, 3]


def plain_rho(N, seed):
    return np.random.default_rng(seed).integers(1, 1 << 64, size=(N, 4), dtype=np.uint64, endpoint=False)


_PAIRS = {}


def oracle_pairs(b, rho):
    """[(W_e, T_e)] for every entry of the batch, as oracle_rlc's inner `entry`"""
    import gs_ref_py as ref

    key = (id(b), rho.tobytes())
    if key not in _PAIRS:
        cn, c = b.cname, curve(b.cname)
        one = gt_one(cn)

        def entry(e):
            _, lhs, rhs, rhs_nt = b.cells[e]
            den = rhs_nt if b.ty == 0 else rhs
            w = one
            for k in range(4):
                if (lhs[k] != den[k]).any():
                    q = ref.gt_mul(cn, lhs[k], ref.gt_inv(cn, den[k]))
                    w = ref.gt_mul(cn, w, ref.gt_pow(cn, q, forge.u8(c.fr(int(rho[e][k])))))
            t = ref.gt_pow(cn, b.entries[e]["target"], forge.u8(c.fr(int(rho[e][3])))) if b.ty == 0 else one
            return w, t

        _PAIRS[key] = (b, list(pool().map(entry, range(b.N))))  # (b is held: its id is the key)
    return _PAIRS[key][1]


def model(b, rho, K, lo=0, hi=None):
    """(ok, n_bad, n_checks) of the descent over the oracle's pairs of entries [lo, hi)"""
    import gs_ref_py as ref

    pairs = oracle_pairs(b, rho)[lo:hi]
    passes = locatevec.from_pairs(pairs, K, lambda x, y: ref.gt_mul(b.cname, x, y), lambda x, y: (x == y).all())
    ok, n_bad, n_checks = locatevec.descend(passes, len(pairs), K)
    return np.array(ok, dtype=np.uint8), n_bad, n_checks


def run(eng, b, rho, lo=0, hi=None):
    """host entry, device entry (they must agree) and acc against gs_verify_batch_rlc_dev -> (ok, info)"""
    import torch

    hi = b.N if hi is None else hi
    N, r = hi - lo, np.ascontiguousarray(rho[lo:hi])
    args = b.args(lo, hi)
    ok, info, acc = eng.verify_batch_rlc_locate(b.ty, N, b.m, b.n, *args, r)
    t = [dev(a) for a in args]
    drho = dev(r.view(np.int64).reshape(-1))
    dacc = torch.zeros(2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    dok = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
    dinfo = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
    eng.verify_batch_rlc_locate_dev(b.ty, N, b.m, b.n, *t, drho, dacc, dok, dinfo)
    eng.sync()
    where = (b.cname, b.ty, lo, hi)
    assert (dok.cpu().numpy() == ok).all(), (where, "host and _dev ok differ")
    assert (dinfo.cpu().numpy().view(np.uint32) == info).all(), (where, "host and _dev info differ")
    assert (dacc.cpu().numpy() == acc).all(), (where, "host and _dev acc differ")
    racc = torch.zeros(2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    eng.verify_batch_rlc_dev(b.ty, N, b.m, b.n, *t, drho, racc)
    eng.sync()
    assert (racc.cpu().numpy() == acc).all(), (where, "acc differs from gs_verify_batch_rlc_dev's")
    return ok, [int(info[0]), int(info[1])]


def check(eng, b, rho, K, lo=0, hi=None, exact=False):
    """the device against the model; exact: also against the oracle's per-entry verdicts"""
    ok, info = run(eng, b, rho, lo, hi)
    want_ok, n_bad, n_checks = model(b, rho, K, lo, hi)
    where = (b.cname, b.ty, K, lo, hi)
    print("locate", where, "info", info, "model", [n_bad, n_checks])
    assert (ok == want_ok).all(), (where, np.nonzero(ok != want_ok)[0][:8], b.names(np.nonzero(ok != want_ok)[0][:8]))
    assert info == [n_bad, n_checks], (where, info, [n_bad, n_checks])
    assert info[0] == int((ok == 0).sum())
    if exact:
        pairs = oracle_pairs(b, rho)[lo:hi]
        want = b.want[lo:hi]
        assert all((w != t).any() for (w, t), v in zip(pairs, want) if v == 0), (where, "a rejected entry with W == T")
        assert (ok == want).all(), (where, np.nonzero(ok != want)[0][:8])
    return ok, info


def profiled(eng, fn):
    eng.prof_enable(True)
    eng.prof_reset()
    out = fn()
    names = [p[0] for p in eng.prof_get()]
    eng.prof_enable(False)
    return out, names


# ---- 1: every type, both curves, planned options ----------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_locate_follows_the_oracle(cname, cid, ty):
    b = full_batch(cname, cid, ty, 4, 4, True)
    assert (b.want == 0).any() and (b.want == 1).any()
    eng = engine(cid, b.crs)
    try:
        (ok, info), names = profiled(eng, lambda: check(eng, b, plain_rho(b.N, 1100 + ty), 8, exact=True))
        assert info[0] == int((b.want == 0).sum()) and info[1] > 1
        assert "k_rlc_leaf" in names and "k_rlc_tree" in names, names
        assert any(nm.startswith("k_rlc_locate") for nm in names), names
    finally:
        eng.close()


# ---- 2: forced arity and kernel form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coop", [0, 2])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("ty", [0, 3])
def test_locate_forced_arity_and_form(ty, K, coop):
    cname, cid = CURVES[0]
    b = full_batch(cname, cid, ty, 4, 4, True)
    eng = engine(cid, b.crs, {"locate_k": K, "coop_fe": coop})
    try:
        _, names = profiled(eng, lambda: check(eng, b, plain_rho(b.N, 1200 + ty), K, exact=True))
        loc = sorted({nm for nm in names if nm.startswith("k_rlc_locate")})
        assert loc == (["k_rlc_locate.coop"] if coop == 2 else ["k_rlc_locate"]), names
    finally:
        eng.close()


@pytest.mark.parametrize("ty", [0, 3])
def test_locate_without_endomorphisms(ty):
    cname, cid = CURVES[0]
    b = full_batch(cname, cid, ty, 4, 4, True)
    eng = engine(cid, b.crs, {"endo": 0})
    try:
        _, names = profiled(eng, lambda: check(eng, b, plain_rho(b.N, 1250 + ty), 8, exact=True))
        assert not [nm for nm in names if nm.startswith("k_var_multi")], names
        assert any(nm.startswith("k_var.plain") for nm in names), names
    finally:
        eng.close()


def test_locate_k_is_validated():
    import groth_sahai_rs_amd as gs

    eng = gs.Engine(0, 0)
    try:
        for v in (0, 2, 4, 8):
            eng.set_option("locate_k", v)
        for v in (-1, 1, 3, 16):
            with pytest.raises(gs.GsError) as ei:
                eng.set_option("locate_k", v)
            assert ei.value.code == 3
    finally:
        eng.close()


# ---- 3: a valid batch costs one node check ------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,cid,ty", [("bls12_381", 0, 0), ("bls12_381", 0, 1), ("bls12_381", 0, 2), ("bls12_381", 0, 3),
                                          ("bn254", 1, 0)])
def test_locate_valid_batch(cname, cid, ty):
    v = valid_batch(cname, cid, ty)
    assert v.want.all()
    eng = engine(cid, v.crs)
    try:
        ok, info = check(eng, v, plain_rho(v.N, 1300 + ty), 8, exact=True)
        assert ok.all() and info == [0, 1]
    finally:
        eng.close()


# ---- 4: lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 2])
def test_locate_lengths(K):
    """a single leaf (accepted, rejected), a full node, a node plus one, two full levels (K = 8), two full levels plus one"""
    cname, cid = CURVES[0]
    b = full_batch(cname, cid, 0, 4, 4, True)
    rho = plain_rho(b.N, 1400)
    rej = int(np.nonzero(b.want == 0)[0][0])
    assert b.want[0] == 1
    eng = engine(cid, b.crs, {"locate_k": 0 if K == 8 else K})
    try:
        ok, info = check(eng, b, rho, K, 0, 1, exact=True)
        assert list(ok) == [1] and info == [0, 1]
        ok, info = check(eng, b, rho, K, rej, rej + 1, exact=True)
        assert list(ok) == [0] and info == [1, 1]
        for n in (2, 8, 9, 64, 65):
            for lo in (0, 1):
                check(eng, b, rho, K, lo, lo + n, exact=True)
    finally:
        eng.close()


# ---- 5: everything is bad ---------------------------------------------------------------------------------------------------
def test_locate_all_bad():
    cname, cid = CURVES[0]
    eq, vs = drawn_equation(cname, cid, 0, 4, 4, True)
    rejected = [v for v in vs if not v["accepted"]]
    ents = [rejected[i % len(rejected)] for i in range(65)]
    b = Batch(eq, ents)
    assert not b.want.any()
    for K in (8, 2):
        eng = engine(cid, b.crs, {"locate_k": 0 if K == 8 else K})
        try:
            ok, info = check(eng, b, plain_rho(b.N, 1500), K, exact=True)
            assert not ok.any()
            assert info == [65, sum(locatevec.level_sizes(65, K))]  # every node of the tree is checked once
        finally:
            eng.close()


# ---- 6: cancellation ----------------------------------------------------------------------------------------------------------
def cancelling_batch(cname, cid, pair, extra=None):
    """valid PPE batch with targets * z and / z at `pair`, and (extra) a rejected variant of the same equation at entry 100"""
    import gs_ref_py as ref

    v = valid_batch(cname, cid, 0)
    cx = forge.Ctx(cname, v.crs)
    z = ref.gt_pow(cname, cx.gt, cx.fr(0xABCDEF0123456789ABCDEF))
    e1, e2 = pair
    ents = list(v.entries)
    ents[e1] = dict(ents[e1], name="target * z", target=ref.gt_mul(cname, ents[e1]["target"], z))
    ents[e2] = dict(ents[e2], name="target / z", target=ref.gt_mul(cname, ents[e2]["target"], ref.gt_inv(cname, z)))
    if extra is not None:
        _, vs = drawn_equation(cname, cid, 0, 4, 4, False)
        ents[extra] = [x for x in vs if not x["accepted"]][0]
    b = Batch(v.eq, ents)
    bad = sorted([e1, e2] + ([extra] if extra is not None else []))
    assert list(np.nonzero(b.want == 0)[0]) == bad  # each of them fails on its own, by the oracle
    return b


@pytest.mark.parametrize("case,pair,extra,equal,reported", [
    ("a", (8, 9), None, True, []),
    ("b", (8, 9), 100, True, [100]),
    ("c", (7, 8), 100, True, [100]),        # node (2, 0) = entries 0 .. 63 holds both halves and passes (module docstring)
    ("c2", (63, 64), 100, True, [63, 64, 100]),
    ("d", (8, 9), 100, False, [8, 9, 100]),
])
def test_locate_cancelling_pairs(case, pair, extra, equal, reported):
    cname, cid = CURVES[0]
    b = cancelling_batch(cname, cid, pair, extra)
    assert b.N > 100
    rho = plain_rho(b.N, 1600)
    rho[pair[0]][3] = rho[pair[1]][3] = (1 << 63) + 12345
    if not equal:
        rho[pair[1]][3] += 1
    eng = engine(cid, b.crs)
    try:
        ok, info = check(eng, b, rho, 8, exact=not equal)
        assert list(np.nonzero(ok == 0)[0]) == reported, case
        if case == "a":
            assert info == [0, 1]
    finally:
        eng.close()


# ---- 7: other shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(3, 1), (8, 3)])
def test_locate_other_shapes(m, n):
    cname, cid = CURVES[0]
    b = full_batch(cname, cid, 0, m, n, True)
    eng = engine(cid, b.crs)
    try:
        check(eng, b, plain_rho(b.N, 1700 + m), 8, exact=True)
    finally:
        eng.close()


# ---- 8: argument errors -----------------------------------------------------------------------------------------------------------
def test_locate_argument_errors():
    import groth_sahai_rs_amd as gs

    cname, cid = CURVES[0]
    b = full_batch(cname, cid, 0, 4, 4, True)
    eng = engine(cid, b.crs)
    try:
        rho = plain_rho(b.N, 1800)
        rho[b.N // 2][2] = 0
        with pytest.raises(gs.GsError) as ei:
            eng.verify_batch_rlc_locate(b.ty, b.N, b.m, b.n, *b.args(), rho)
        assert ei.value.code == 3
        empty = [np.zeros(0, dtype=np.uint8)] * 8
        with pytest.raises(gs.GsError) as ei:
            eng.verify_batch_rlc_locate(b.ty, 0, b.m, b.n, *empty, np.zeros(0, dtype=np.uint64))
        assert ei.value.code == 3
        # an output over an input, and two outputs over each other (the C ABI itself: the binding allocates its outputs)
        import ctypes

        from groth_sahai_rs_amd.capi import _p

        rho = plain_rho(b.N, 1801).reshape(-1)
        args = [forge.u8(a) for a in b.args()]
        ok, info, acc = np.zeros(b.N, dtype=np.uint8), np.zeros(2, dtype=np.uint32), np.zeros(2 * eng.GT, dtype=np.uint8)
        call = lambda acc_, ok_, info_: eng.lib.gs_verify_batch_rlc_locate(
            eng.ctx, b.ty, ctypes.c_size_t(b.N), b.m, b.n, *[_p(a) for a in args], _p(rho), _p(acc_), _p(ok_), _p(info_))
        assert call(args[3][:2 * eng.GT], ok, info) == 3   # acc inside target
        assert call(acc, args[7][:b.N], info) == 3          # ok inside theta
        assert call(acc, acc[8:8 + b.N], info) == 3         # ok inside acc
        assert call(acc, ok, info) == 0 and info[0] == int((b.want == 0).sum())
    finally:
        eng.close()


# ---- 9: the mirror ------------------------------------------------------------------------------------------------------------------
class Rng:
    def __init__(self, seed):
        self.r = np.random.default_rng(seed)

    def fr(self):
        v = self.r.integers(0, 1 << 62, size=4, dtype=np.uint64)
        v[3] &= np.uint64((1 << 60) - 1)
        return v


def test_mirror_verify_batch_locate():
    from groth_sahai_rs_amd import mirror

    cname, cid = CURVES[0]
    eq, vs = drawn_equation(cname, cid, 0, 4, 4, True)
    forged = [v for v in vs if not v["accepted"]]
    ents = [eq, eq, forged[0], eq, eq, eq, forged[-1], eq]
    want = [bool(forge.oracle_verdict(eq, v)) for v in ents]
    assert want == [True, True, False, True, True, True, False, True]
    m, n = eq["m"], eq["n"]
    c = curve(cname)
    words = lambda a, cnt: [x.copy() for x in forge.u8(a).reshape(cnt, -1).view(np.uint64)]
    raw, o, pieces = forge.u8(eq["crs"]), 0, []
    G1, G2, GT = 2 * c.nq * 8, 4 * c.nq * 8, 12 * c.nq * 8
    for sz in (2 * G1, 2 * G1, 2 * G2, 2 * G2, G1, G2, GT):
        pieces.append(raw[o:o + sz].view(np.uint64).copy())
        o += sz
    assert o == raw.size
    crs = mirror.CRS(pieces[:2], pieces[2:4], pieces[4], pieces[5], pieces[6])
    equs, proofs = [], []
    for v in ents:
        g = words(v["G"], m * n)
        equs.append(mirror.PPE(words(v["A"], n), words(v["B"], m), [[g[i * n + j] for j in range(n)] for i in range(m)],
                               forge.u8(v["target"]).view(np.uint64).copy()))
        proofs.append(mirror.CProof(mirror.Commit1(words(v["xcoms"], m), None), mirror.Commit2(words(v["ycoms"], n), None),
                                    [mirror.EquProof(words(v["pi"], 2), words(v["theta"], 2), 0, None)]))
    assert [e.verify(p, crs) for e, p in zip(equs, proofs)] == want  # the exact verifier, entry by entry
    assert mirror.verify_batch_locate(equs, proofs, crs, Rng(5)) == want
    with pytest.raises(AssertionError):  # lengths from the wire are checked before the C ABI
        proofs[3].equ_proofs[0].pi = proofs[3].equ_proofs[0].pi[:-1]
        mirror.verify_batch_locate(equs, proofs, crs, Rng(6))

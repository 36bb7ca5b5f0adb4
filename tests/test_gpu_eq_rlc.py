"""gs_verify_equation_rlc[_dev]: N proofs of ONE equation (constants in one copy), one combined pairing check with the
random linear combination taken across the proofs, against the C oracle (tests/eqrlc.py: the per-proof
cells of ref_verify_cells) and against gs_verify_batch_rlc on the same proofs with the constants replicated.

Convention checked (include/gs_amd.h): FE(acc[0]) = W = prod_e prod_c (lhs_c / rhs'_c)^rho_e,c (rhs' = the right-hand
side without the PPE target), acc[1] = T = t^(sum_e rho_e,3) (PPE; one otherwise), ok_all = (W == T).  acc[1] is
compared byte for byte; acc[0] is an un-exponentiated Miller value and is compared through gs_gt_finalize.
rho is FIXED and seeded here (a test of arithmetic; the CSPRNG contract of the header is about production).
No tolerance anywhere: verdicts are bits.  Every test sends at most 150 equations through the oracle.
Not tested: the refusal inside a mixed call.  The library refuses the entry while a gs_*_mixed call records its launches,
but nothing a caller can do through the C ABI runs another entry in that window, so no test can reach the check."""
import ctypes

import numpy as np
import pytest

import eqrlc
import forge
from eqrlcdata import make_batch
from forge import ref
from gpubatch import pool

pytestmark = pytest.mark.gpu

CURVES = [("bls12_381", 0), ("bn254", 1)]
TYPES = [0, 1, 2, 3]
EDGE_RHO = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
MIXED_ROW = [(1 << 64) - 1, 1, 1 << 32, (1 << 63) + 5]
# (N, m, n, types): N = 9 is one more than a run of the sum (K = 8); N = 65 is a second wave of proof lanes and three
# levels of the sum; N = 513 four levels (no oracle at that size: test_five_hundred_and_thirteen_proofs)
SHAPES = [(1, 1, 1, TYPES), (2, 2, 3, TYPES), (9, 3, 1, TYPES), (65, 1, 1, [0, 3])]

_DATA, _CELLS = {}, {}


def data(cname, cid, ty, N, m, n):
    key = (cname, ty, N, m, n)
    if key not in _DATA:
        _DATA[key] = make_batch(cname, cid, ty, N, m, n)
    return _DATA[key]


def oracle(d, rho, proofs=None):
    """(W, T, verdicts) of the batch; the cells of a proof are computed once per distinct input (they do not depend on
    rho), on the oracle's thread pool"""
    proofs = d.proofs if proofs is None else proofs
    eqs = [eqrlc.equation_of(d.cname, d.ty, d.m, d.n, d.const, p, d.crs) for p in proofs]
    keys = [(d.cname, d.ty) + tuple(eq[k].tobytes() for k in forge.INPUTS) for eq in eqs]
    new = {k: eq for k, eq in zip(keys, eqs) if k not in _CELLS}
    for k, cells in zip(new, pool().map(lambda eq: forge.oracle_cells(eq, eq), new.values())):
        _CELLS[k] = cells
    return eqrlc.combine(d.cname, d.ty, d.const["target"], [_CELLS[k] for k in keys], rho)


def seeded_rho(N, seed):
    """Fixed exponents [N][4]: random rows, the mixed row first, a row of edge values last, all-ones-64 second (the sums
    pass 2^64 as soon as N >= 3)"""
    rho = np.random.default_rng(seed).integers(1, 1 << 64, size=(N, 4), dtype=np.uint64, endpoint=False)
    rho[0] = np.array(MIXED_ROW, dtype=np.uint64)
    if N > 1:
        rho[N - 1] = np.array([EDGE_RHO[(seed + k) % len(EDGE_RHO)] for k in (0, 3, 4, 5)], dtype=np.uint64)
    if N > 2:
        rho[1] = (1 << 64) - 1
    return rho


def engine(cid, crs, opts=None):
    import groth_sahai_rs_amd as gs

    eng = gs.Engine(cid, 0)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    eng.set_crs(crs)
    return eng


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def run_dev(eng, d, arrays, rho, N):
    import torch

    acc = torch.zeros(2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    t = [dev(a) for a in arrays]
    eng.verify_equation_rlc_dev(d.ty, N, d.m, d.n, *t, dev(rho.view(np.int64).reshape(-1)), acc)
    eng.sync()
    return acc.cpu().numpy()


def check(eng, d, rho, what, proofs=None, want_ok=None, against_oracle=True):
    """One call through the host and the device entry against the oracle and against gs_verify_batch_rlc on the
    replicated constants.  -> (ok_all, acc)"""
    proofs = d.proofs if proofs is None else proofs
    N, GT = len(proofs), eng.GT
    arrays = eqrlc.arrays(d.const, proofs)
    ok, acc = eng.verify_equation_rlc(d.ty, N, d.m, d.n, *arrays, rho)
    acc = np.asarray(acc)
    where = (what, d.cname, d.ty, N, d.m, d.n)
    ok1, acc1 = eng.verify_batch_rlc(d.ty, N, d.m, d.n, *eqrlc.replicated(d.const, proofs), rho)
    acc1 = np.asarray(acc1)
    assert (acc[GT:] == acc1[GT:]).all(), (where, "acc[1] != gs_verify_batch_rlc's")
    assert ok == ok1, (where, "verdict != gs_verify_batch_rlc's", ok, ok1)
    if against_oracle:
        W, T, oks = oracle(d, rho, proofs)
        assert (acc[GT:] == T).all(), (where, "acc[1] != t^(sum rho[3])")
        assert eng.gt_finalize(np.concatenate([acc[:GT], W])) == 1, (where, "FE(acc[0]) != W")
        gt = forge.Ctx(d.cname, d.crs).gt  # (the comparison does tell W from W * gt)
        assert eng.gt_finalize(np.concatenate([acc[:GT], ref.gt_mul(d.cname, W, gt)])) == 0, where
        assert ok == int((W == T).all()), (where, "verdict", ok)
    if want_ok is not None:
        assert ok == want_ok, (where, ok)
    dacc = run_dev(eng, d, arrays, rho, N)
    assert (dacc == acc).all(), (where, "host and _dev results differ")
    return ok, acc


# ---- a. valid batches: both forms of the pi term, and the forced kernel shapes ---------------------------------------------
CASES_A = [(cname, cid, ty, N, m, n) for cname, cid in CURVES for N, m, n, tys in SHAPES for ty in tys]


@pytest.mark.parametrize("cname,cid,ty,N,m,n", CASES_A)
def test_valid_batches(cname, cid, ty, N, m, n):
    d = data(cname, cid, ty, N, m, n)
    assert d.witnesses == min(N, 3)
    rho = seeded_rho(N, 40 + ty)
    accs = {}
    for pi_form in (0, 1):
        eng = engine(cid, d.crs, {"eq_pi": pi_form})
        try:
            ok, acc = check(eng, d, rho, "valid, eq_pi %d" % pi_form, want_ok=1)
            accs[pi_form] = acc
            eng.prof_enable(True)
            eng.prof_reset()
            run_dev(eng, d, eqrlc.arrays(d.const, d.proofs), rho, N)
            names = [p[0] for p in eng.prof_get()]
            eng.prof_enable(False)
            assert "k_miller.eqrlc" in names and "k_miller.eqrlc.batch" in names and "k_prep_verify_eq_rlc" in names, names
            assert "k_batch_sum.eqs1" in names and ("k_batch_sum.eqs2" in names) == (pi_form == 1), names
            assert ("k_eq_rlc_tpow" in names) == (ty == 0) and "k_rlc_tpow" not in names, names
        finally:
            eng.close()
    assert (accs[0][accs[0].size // 2:] == accs[1][accs[1].size // 2:]).all()
    if (N, m, n) not in ((2, 2, 3), (9, 3, 1)):
        return
    # the planned form, and the forced shapes of the lanes underneath: the same target side, the same verdict
    for opts in ({}, {"endo": 0}, {"line_tables": 0}, {"miller_ch": 2, "eq_pi": 1}, {"var_tm": 2, "eq_pi": 1}):
        eng = engine(cid, d.crs, opts)
        try:
            check(eng, d, rho, "valid, %r" % (opts,), want_ok=1, against_oracle=False)
            W, T, _ = oracle(d, rho)
            ok, acc = eng.verify_equation_rlc(ty, N, m, n, *eqrlc.arrays(d.const, d.proofs), rho)
            assert eng.gt_finalize(np.concatenate([np.asarray(acc)[:eng.GT], W])) == 1, opts
            if "var_tm" in opts:  # the forced lane shape is the one that ran: pass 2 in 4-term Straus lanes
                eng.prof_enable(True)
                eng.prof_reset()
                run_dev(eng, d, eqrlc.arrays(d.const, d.proofs), rho, N)
                names = [p[0] for p in eng.prof_get()]
                eng.prof_enable(False)
                assert any(nm.startswith("k_var_multi4") and nm.endswith(".q2") for nm in names), names
                assert not any(nm.startswith("k_var_multi8") for nm in names), names
        finally:
            eng.close()


# ---- b. one well-formed forged proof at the first, a middle and the last position ------------------------------------------
def forged(d, e):
    """the proofs of d with proof e forged: the generator added to theta[0].0 (a point of the subgroup)"""
    cx = forge.Ctx(d.cname, d.crs)
    proofs = [dict(p) for p in d.proofs]
    th = forge.u8(proofs[e]["theta"])
    th[:cx.G1] = cx.add(1, th[:cx.G1], cx.g1)
    proofs[e]["theta"] = th
    return proofs


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_one_forged_proof_in_nine(cname, cid, ty):
    d = data(cname, cid, ty, 9, 3, 1)
    rho = seeded_rho(9, 60 + ty)
    for pi_form in (0, 1):
        eng = engine(cid, d.crs, {"eq_pi": pi_form})
        try:
            for e in (0, 4, 8):
                check(eng, d, rho, "proof %d forged" % e, proofs=forged(d, e), want_ok=0)
            # another kind of forgery: the pi of proof 4 is proof 5's
            proofs = [dict(p) for p in d.proofs]
            proofs[4]["pi"] = d.proofs[5]["pi"]
            check(eng, d, rho, "pi of proof 5 in proof 4", proofs=proofs, want_ok=0)
        finally:
            eng.close()


# ---- c. the edges of the sum across the batch ---------------------------------------------------------------------------------
def negated(d, p):
    cx = forge.Ctx(d.cname, d.crs)
    out = {}
    for k, group in (("xcoms", 1), ("ycoms", 2), ("pi", 2), ("theta", 1)):
        sz = cx.size(group)
        a = forge.u8(p[k])
        out[k] = np.concatenate([cx.neg(group, a[i:i + sz]) for i in range(0, a.size, sz)])
    return out


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_sum_edges(cname, cid, ty):
    """Equal inputs (every addition of the sum is a doubling), opposite inputs (every sum is the identity and its pair
    contributes one), identity commitments, identity theta: each against the oracle's value, both forms of the pi term."""
    d = data(cname, cid, ty, 2, 2, 3)
    p0, p1 = d.proofs
    same = np.array([MIXED_ROW, MIXED_ROW], dtype=np.uint64)
    rho3 = np.array([MIXED_ROW, MIXED_ROW, [5, 6, 7, 8]], dtype=np.uint64)
    zero = lambda a: np.zeros_like(forge.u8(a))
    sets = [("two identical proofs, identical rho rows", [p0, p0], same),
            ("a proof and its negation, identical rho rows", [p0, negated(d, p0)], same),
            ("a proof, its negation and a third", [p0, negated(d, p0), p1], rho3),
            ("all commitments the identity", [dict(p0, xcoms=zero(p0["xcoms"]), ycoms=zero(p0["ycoms"])),
                                              dict(p1, xcoms=zero(p1["xcoms"]), ycoms=zero(p1["ycoms"]))], seeded_rho(2, 3)),
            ("identity theta", [dict(p0, theta=zero(p0["theta"])), dict(p1, theta=zero(p1["theta"]))], seeded_rho(2, 4)),
            ("identity pi in one proof", [dict(p0, pi=zero(p0["pi"])), p1], seeded_rho(2, 5))]
    for pi_form in (0, 1):
        eng = engine(cid, d.crs, {"eq_pi": pi_form})
        try:
            for name, proofs, rho in sets:
                ok, _ = check(eng, d, rho, name, proofs=proofs)
                if name.startswith("two identical"):
                    assert ok == 1
        finally:
            eng.close()


# ---- d. four levels of the sum: no oracle at this size ------------------------------------------------------------------------
@pytest.mark.parametrize("ty", [0, 3])
@pytest.mark.parametrize("cname,cid", CURVES)
def test_five_hundred_and_thirteen_proofs(cname, cid, ty):
    d = data(cname, cid, ty, 513, 1, 1)
    rho = seeded_rho(513, 90 + ty)
    for pi_form in (0, 1):
        eng = engine(cid, d.crs, {"eq_pi": pi_form})
        try:
            ok, acc = check(eng, d, rho, "513 valid", want_ok=1, against_oracle=False)
            assert eng.gt_finalize(acc) == 1
            ok, acc = check(eng, d, rho, "513, proof 512 forged", proofs=forged(d, 512), want_ok=0, against_oracle=False)
            assert eng.gt_finalize(acc) == 0
        finally:
            eng.close()


# ---- e. the pairing work ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", [0, 3])
@pytest.mark.parametrize("cname,cid", CURVES)
def test_pairing_work(cname, cid, ty):
    """k_miller.eqrlc runs exactly 2 n N pairs with the pi term folded; the batch-level pairs are the same number at
    N = 9 (the first nine proofs) and at N = 65"""
    d = data(cname, cid, ty, 65, 1, 1)
    work = {}
    for N in (9, 65):
        eng = engine(cid, d.crs, {"eq_pi": 1})
        try:
            eng.prof_enable(True)
            eng.prof_reset()
            run_dev(eng, d, eqrlc.arrays(d.const, d.proofs[:N]), seeded_rho(N, 5), N)
            prof = eng.prof_get_work()
            eng.prof_enable(False)
        finally:
            eng.close()
        assert sorted(nm for nm in prof if nm.startswith("k_miller")) == ["k_miller.eqrlc", "k_miller.eqrlc.batch"], sorted(prof)
        assert prof["k_miller.eqrlc"][1] == 2 * d.n * N, (N, prof["k_miller.eqrlc"])
        work[N] = prof["k_miller.eqrlc.batch"]
    assert work[9] == work[65], work
    assert work[9][1] <= eqrlc.pair_counts(ty, 1, 1, True)[1]  # (a table-read CRS pair counts below one stepped pair)


# ---- f. composition: two calls, one verdict ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_split_batches_compose(cname, cid, ty):
    d = data(cname, cid, ty, 9, 3, 1)
    rho = seeded_rho(9, 70 + ty)
    eng = engine(cid, d.crs)
    try:
        for proofs, want in ((d.proofs, 1), (forged(d, 6), 0)):
            pairs = []
            for lo, hi in ((0, 4), (4, 9)):
                _, acc = eng.verify_equation_rlc(ty, hi - lo, 3, 1, *eqrlc.arrays(d.const, proofs[lo:hi]), rho[lo:hi])
                pairs.append(np.asarray(acc))
            assert eng.gt_finalize(np.concatenate(pairs)) == want
            ok, whole = eng.verify_equation_rlc(ty, 9, 3, 1, *eqrlc.arrays(d.const, proofs), rho)
            assert ok == want
            # the target sides multiply to the whole batch's
            both = ref.gt_mul(d.cname, pairs[0][eng.GT:], pairs[1][eng.GT:])
            assert (both == np.asarray(whole)[eng.GT:]).all()
    finally:
        eng.close()


# ---- g. status codes ------------------------------------------------------------------------------------------------------------------
def test_status_codes():
    import groth_sahai_rs_amd as gs

    d = data("bls12_381", 0, 0, 2, 2, 3)
    eng = engine(0, d.crs)
    try:
        arrays = eqrlc.arrays(d.const, d.proofs)
        rho = seeded_rho(2, 1)
        zero = rho.copy()
        zero[1][2] = 0
        with pytest.raises(gs.GsError) as ei:
            eng.verify_equation_rlc(0, 2, 2, 3, *arrays, zero)
        assert ei.value.code == 3 and "rho" in str(ei.value)
        # short arrays -- and constants replicated as gs_verify_batch_rlc takes them -- are refused by the binding
        # (GS_ERR_SHAPE) before a pointer crosses the C ABI
        for i in range(8):
            short = list(arrays)
            short[i] = arrays[i][:-1]
            with pytest.raises(gs.GsError) as ei:
                eng.verify_equation_rlc(0, 2, 2, 3, *short, rho)
            assert ei.value.code == 1, i
        with pytest.raises(gs.GsError) as ei:
            eng.verify_equation_rlc(0, 2, 2, 3, *eqrlc.replicated(d.const, d.proofs), rho)
        assert ei.value.code == 1
        with pytest.raises(gs.GsError) as ei:
            eng.verify_equation_rlc(0, 2, 2, 3, *arrays, rho.reshape(-1)[:7])
        assert ei.value.code == 1
        buf = np.ones(1 << 16, dtype=np.uint8)
        p = ctypes.c_void_p(buf.ctypes.data)
        z = lambda v: ctypes.c_size_t(v)
        host, devf = eng.lib.gs_verify_equation_rlc, eng.lib.gs_verify_equation_rlc_dev
        # N = 0
        assert host(eng.ctx, 0, z(0), 1, 1, *[p] * 11) == 3
        assert devf(eng.ctx, 0, z(0), 1, 1, *[p] * 10) == 3
        # bad shape (GS_ERR_SHAPE), bad type (GS_ERR_ARG, as check_shape answers every entry)
        assert devf(eng.ctx, 0, z(1), 0, 1, *[p] * 10) == 1
        assert devf(eng.ctx, 0, z(1), 1, 5000, *[p] * 10) == 1
        assert devf(eng.ctx, 7, z(1), 1, 1, *[p] * 10) == 3
        # null pointers: every array of the _dev form, every input of the host form (acc and ok_all may be NULL there)
        for i in range(10):
            args = [p] * 10
            args[i] = None
            assert devf(eng.ctx, 0, z(1), 1, 1, *args) == 3, i
        for i in range(9):
            args = [p] * 11
            args[i] = None
            assert host(eng.ctx, 0, z(1), 1, 1, *args) == 3, i
        ok, _ = eng.verify_equation_rlc(0, 2, 2, 3, *arrays, rho)  # the context still works
        assert ok == 1
        with pytest.raises(gs.GsError):
            eng.set_option("eq_pi", 2)
    finally:
        eng.close()
    # no CRS
    bare = gs.Engine(0, 0)
    try:
        assert bare.lib.gs_verify_equation_rlc_dev(bare.ctx, 0, ctypes.c_size_t(1), 1, 1, *[p] * 10) == 4  # GS_ERR_NOCRS
        assert bare.lib.gs_verify_equation_rlc(bare.ctx, 0, ctypes.c_size_t(1), 1, 1, *[p] * 11) == 4
    finally:
        bare.close()

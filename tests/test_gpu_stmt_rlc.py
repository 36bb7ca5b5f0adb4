"""gs_verify_statements_rlc[_dev]: S statements of E equations over shared commitments, one combined pairing check per
statement, against the C oracle (tests/stmtrlc.py: the per-equation cells of ref_verify_cells on the shared commitments,
as oracle_rlc in test_gpu_soundness.py).

Convention checked (include/gs_amd.h): FE(acc[s][0]) = W_s = prod_e prod_c (lhs_c / rhs'_c)^rho_e,c (rhs' = the right-hand
side without the PPE target), acc[s][1] = T_s = prod_e t_e^rho_e,3 (PPE; one otherwise), ok[s] = (W_s == T_s).  acc[s][1]
is compared byte for byte; acc[s][0] is an un-exponentiated Miller value and is compared through gs_gt_finalize.
rho is FIXED and seeded here (a test of arithmetic; the CSPRNG contract of the header is about production).
No tolerance anywhere: verdicts are bits.  Every test sends at most 150 equations through the oracle."""
import ctypes

import numpy as np
import pytest

import forge
import stmtrlc
from forge import ref
from gpubatch import pool

pytestmark = pytest.mark.gpu

CURVES = [("bls12_381", 0), ("bn254", 1)]
TYPES = [0, 1, 2, 3]
EDGE_RHO = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
MIXED_ROW = [(1 << 64) - 1, 1, 1 << 32, (1 << 63) + 5]
KEYS = ("A", "B", "G", "target", "xcoms", "ycoms", "pi", "theta")
# (S, E, m, n, types): E = 9 is one more term than a Straus lane shares; E = 65 gives the theta / pi sums 130 terms (more
# than 16 partials: the slot fold runs); S = 65 is a second wave of statement lanes; S = 22 a second wave of 3-lane groups
# (coop_fe forced).  The two longest shapes run PPE and QuadEqu only (the 150-equation cap on the oracle).
SHAPES = [(1, 1, 1, 1, TYPES), (3, 2, 2, 3, TYPES), (3, 9, 3, 1, TYPES), (1, 65, 1, 1, [0, 3]), (65, 2, 1, 1, [0, 3]),
          (22, 1, 1, 1, TYPES)]


# ---- statements, proofs and the oracle's values: built once per (curve, type, shape), never changed --------------------
class Data:
    """S proven statements of one type and shape under one CRS: per-statement dicts of the eight verifier inputs."""

    def __init__(self, cname, cid, ty, S, E, m, n, crs, stmts):
        self.cname, self.cid, self.ty, self.S, self.E, self.m, self.n, self.crs, self.stmts = cname, cid, ty, S, E, m, n, crs, stmts
        self.cells = {}

    def arrays(self, stmts=None):
        stmts = self.stmts if stmts is None else stmts
        return [np.concatenate([forge.u8(s[k]) for s in stmts]) for k in KEYS]

    def oracle(self, rho, stmts=None):
        """[(W_s, T_s, verdicts of the equations)]"""
        stmts = self.stmts if stmts is None else stmts
        # the cells of every equation not seen yet, on the oracle's thread pool (the C oracle runs outside the GIL)
        new = {}
        for st in stmts:
            for eq in stmtrlc.equations(self.cname, self.ty, self.m, self.n, self.E, st, self.crs):
                key = tuple(eq[k].tobytes() for k in forge.INPUTS)
                if key not in self.cells:
                    new[key] = eq
        for key, cells in zip(new, pool().map(lambda eq: forge.oracle_cells(eq, eq), new.values())):
            self.cells[key] = cells
        return [literal_cached(self, s, rho[i]) for i, s in enumerate(stmts)]


def literal_cached(d, st, rho):
    """stmtrlc.literal with the cells of an equation computed once per distinct input"""
    c = forge.curve(d.cname)
    one = stmtrlc.gt_one(d.cname)
    W, T, oks = one, one, []
    for e, eq in enumerate(stmtrlc.equations(d.cname, d.ty, d.m, d.n, d.E, st, d.crs)):
        key = tuple(eq[k].tobytes() for k in forge.INPUTS)
        if key not in d.cells:
            d.cells[key] = forge.oracle_cells(eq, eq)
        ok, lhs, rhs, rhs_nt = d.cells[key]
        oks.append(ok)
        den = rhs_nt if d.ty == 0 else rhs
        for k in range(4):
            if (lhs[k] != den[k]).any():
                q = ref.gt_mul(d.cname, lhs[k], ref.gt_inv(d.cname, den[k]))
                W = ref.gt_mul(d.cname, W, ref.gt_pow(d.cname, q, forge.u8(c.fr(int(rho[e][k])))))
        if d.ty == 0:
            T = ref.gt_mul(d.cname, T, ref.gt_pow(d.cname, eq["target"], forge.u8(c.fr(int(rho[e][3])))))
    return W, T, oks


_DATA = {}


def data(cname, cid, ty, S, E, m, n):
    key = (cname, ty, S, E, m, n)
    if key not in _DATA:
        import groth_sahai_rs_amd as gs
        from stmtutil import StatementInputs

        eng = gs.Engine(cid, 0)
        try:
            st = StatementInputs(eng, mg=m, ng=n, ms=m, ns=n, seed=7100)
            stmts = []
            for s in range(S):
                if s:  # other variables, other commitments: a wrong per-statement stride must not go unnoticed
                    st.dlog = {k: st.scalars(len(v)) for k, v in st.dlog.items()}
                    st.vars = dict(xg=st.g(1, st.dlog["xg"]), yg=st.g(2, st.dlog["yg"]), xs=st.fr(st.dlog["xs"]),
                                   ys=st.fr(st.dlog["ys"]))
                    st.rand = dict(xg=st.fr(st.scalars(2 * m)), yg=st.fr(st.scalars(2 * n)), xs=st.fr(st.scalars(m)),
                                   ys=st.fr(st.scalars(n)))
                p = st.part(ty, E)
                assert (p["m"], p["n"]) == (m, n)
                out = eng.prove_statement(ty, E, m, n, p["X"], p["Y"], p["A"], p["B"], p["Gamma"], p["R"], p["S"], p["T"])
                stmts.append(dict(A=forge.u8(p["A"]), B=forge.u8(p["B"]), G=forge.u8(p["Gamma"]), target=forge.u8(p["target"]),
                                  xcoms=forge.u8(out["xcoms"]), ycoms=forge.u8(out["ycoms"]), pi=forge.u8(out["pi"]),
                                  theta=forge.u8(out["theta"])))
            _DATA[key] = Data(cname, cid, ty, S, E, m, n, forge.u8(st.crs), stmts)
        finally:
            eng.close()
    return _DATA[key]


def seeded_rho(S, E, seed):
    """Fixed exponents [S][E][4]: random rows (all four cells different), with rows of edge values and the mixed row on
    the first and the last equation of the statements"""
    rho = np.random.default_rng(seed).integers(1, 1 << 64, size=(S, E, 4), dtype=np.uint64, endpoint=False)
    for s in range(S):
        rho[s][0] = EDGE_RHO[s % len(EDGE_RHO)] if s % 2 else np.array(MIXED_ROW, dtype=np.uint64)
        if E > 1:
            rho[s][E - 1] = np.array(MIXED_ROW, dtype=np.uint64) if s % 2 else EDGE_RHO[(s + 3) % len(EDGE_RHO)]
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


def run_dev(eng, d, arrays, rho, S=None):
    import torch

    S = d.S if S is None else S
    acc = torch.zeros(S * 2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    ok = torch.full((S,), 7, dtype=torch.uint8, device="cuda:0")
    t = [dev(a) for a in arrays]
    eng.verify_statements_rlc_dev(d.ty, S, d.E, d.m, d.n, *t, dev(rho.view(np.int64).reshape(-1)), acc, ok)
    eng.sync()
    return ok.cpu().numpy(), acc.cpu().numpy().reshape(S, 2, eng.GT)


def check(eng, d, rho, what, stmts=None, want_ok=None, exact=True):
    """One call through the host and the device entry against the oracle.  -> (ok, acc)"""
    stmts = d.stmts if stmts is None else stmts
    S, GT = len(stmts), eng.GT
    arrays = d.arrays(stmts)
    want = d.oracle(rho, stmts)
    ok, acc = eng.verify_statements_rlc(d.ty, S, d.E, d.m, d.n, *arrays, rho)
    gt = forge.Ctx(d.cname, d.crs).gt
    for s, (W, T, oks) in enumerate(want):
        where = (what, d.cname, d.ty, "statement", s)
        assert (acc[s][1] == T).all(), (where, "acc[1] != prod target^rho[3]")
        assert eng.gt_finalize(np.concatenate([acc[s][0], W])) == 1, (where, "FE(acc[0]) != W")
        if s in (0, S // 2, S - 1):  # (the comparison does tell W from W * gt)
            assert eng.gt_finalize(np.concatenate([acc[s][0], ref.gt_mul(d.cname, W, gt)])) == 0, where
        assert int(ok[s]) == int((W == T).all()), (where, "verdict", ok)
    if want_ok is not None:
        assert [int(v) for v in ok] == list(want_ok), (what, d.cname, d.ty, ok)
    dok, dacc = run_dev(eng, d, arrays, rho, S)
    assert (dok == ok).all() and (dacc == acc).all(), (what, "host and _dev results differ")
    if exact:  # agreement with the exact verifier: the statement holds iff every equation does
        for s, st in enumerate(stmts):
            each = eng.verify_statement(d.ty, d.E, d.m, d.n, *[st[k] for k in KEYS])
            assert [int(v) for v in each] == want[s][2], (what, s, "gs_verify_statement against the oracle")
            assert int(ok[s]) == int(each.all()), (what, s, ok, each)
    return ok, acc


# ---- a. parity on true statements (and e. agreement with the existing verifiers) -----------------------------------------
CASES_A = [(cname, cid, ty, S, E, m, n) for cname, cid in CURVES for S, E, m, n, tys in SHAPES for ty in tys]


@pytest.mark.parametrize("cname,cid,ty,S,E,m,n", CASES_A)
def test_true_statements(cname, cid, ty, S, E, m, n):
    d = data(cname, cid, ty, S, E, m, n)
    rho = seeded_rho(S, E, 40 + ty)
    # which final kernel runs: 3-lane groups forced at S = 22 (a second wave of groups), one lane per statement forced at
    # S = 65 (a second wave of statement lanes: the planner itself takes the groups until S fills the chip), planned else
    opts = {"coop_fe": 2} if S == 22 else {"coop_fe": 0} if S == 65 else {}
    eng = engine(cid, d.crs, opts)
    try:
        ok, acc = check(eng, d, rho, "true statements", want_ok=[1] * S)
        eng.prof_enable(True)  # which kernels one call runs
        eng.prof_reset()
        run_dev(eng, d, d.arrays(), rho)
        names = [p[0] for p in eng.prof_get()]
        eng.prof_enable(False)
        if S == 22:
            assert "k_stmt_final.coop" in names and "k_stmt_final" not in names, names
        if S == 65:
            assert "k_stmt_final" in names and "k_stmt_final.coop" not in names, names
        if E == 65:
            assert any(nm.startswith("k_slot_fold") for nm in names), names
        if E == 1:  # the same equation and rho through gs_verify_batch_rlc: the same target-side accumulator
            for s, st in enumerate(d.stmts):
                ok1, acc1 = eng.verify_batch_rlc(ty, 1, m, n, *[st[k] for k in KEYS], rho[s])
                assert ok1 == 1 and (np.asarray(acc1)[eng.GT:] == acc[s][1]).all(), s
    finally:
        eng.close()
    plain = engine(cid, d.crs, dict(opts, endo=0))  # without endomorphisms: the same verdicts and target products
    try:
        ok0, acc0 = plain.verify_statements_rlc(ty, S, E, m, n, *d.arrays(), rho)
        assert (ok0 == ok).all() and (acc0[:, 1] == acc[:, 1]).all()
    finally:
        plain.close()


# ---- b. / c. forgeries in ONE statement of three, rho edges on the first and last equation -------------------------------
def forged_sets(d):
    """[(name, statements, the statements the oracle must reject or None)]: one change at a time in statement 1 at
    equation 0, 2 or 4, and one in the commitments of statement 2"""
    cx = forge.Ctx(d.cname, d.crs)
    ty, E, m, n = d.ty, d.E, d.m, d.n
    xg, yg, kx, ky = stmtrlc.shape(ty)
    G1, G2 = cx.G1, cx.G2
    out = []

    def with_stmt(i, **changed):
        st = [dict(s) for s in d.stmts]
        st[i].update({k: forge.u8(v) for k, v in changed.items()})
        return st

    def put(arr, off, val):
        a = forge.u8(arr)
        a[off:off + val.size] = val
        return a

    base = d.stmts[1]
    for e in (0, 2, 4):
        # the target of the unsatisfied twin: the discrete logarithm of the target moved by 1 + e
        if ty == 0:
            t = base["target"][e * cx.GT:(e + 1) * cx.GT]
            tw = put(base["target"], e * cx.GT, ref.gt_mul(d.cname, t, ref.gt_pow(d.cname, cx.gt, cx.fr(1 + e))))
        elif ty == 3:
            tw = put(base["target"], e * 32, cx.fr(cx.fr_ints(base["target"][e * 32:(e + 1) * 32])[0] + 1 + e))
        else:
            g, sz = (1, G1) if ty == 1 else (2, G2)
            t = base["target"][e * sz:(e + 1) * sz]
            tw = put(base["target"], e * sz, cx.add(g, t, cx.mul(g, cx.gen(g), 1 + e)))
        out.append(("target of equation %d: the unsatisfied twin's" % e, with_stmt(1, target=tw), [1]))
        # pi swapped with the next equation's
        f, sz = (e + 1) % E, kx * 2 * G2
        pi = forge.u8(base["pi"])
        pi[e * sz:(e + 1) * sz], pi[f * sz:(f + 1) * sz] = base["pi"][f * sz:(f + 1) * sz], base["pi"][e * sz:(e + 1) * sz]
        out.append(("pi of equations %d and %d swapped" % (e, f), with_stmt(1, pi=pi), [1]))
        # the generator added to theta[e][0].0: cells (0, .) only
        off = e * ky * 2 * G1
        th = put(base["theta"], off, cx.add(1, base["theta"][off:off + G1], cx.g1))
        out.append(("theta[%d][0].0 += gen" % e, with_stmt(1, theta=th), [1]))
    xc = put(d.stmts[2]["xcoms"], G1, cx.add(1, d.stmts[2]["xcoms"][G1:2 * G1], cx.g1))
    out.append(("statement 2: xcoms[0].1 += gen", with_stmt(2, xcoms=xc), [2]))
    return out


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_forgeries_in_one_statement(cname, cid, ty):
    """S = 3, E = 5, 2 x 2: only the forged statement is rejected, the accumulators follow the oracle (the forged
    statement's W is not one: the edge rows of rho on its first and last equation enter the compared value)."""
    d = data(cname, cid, ty, 3, 5, 2, 2)
    rho = seeded_rho(3, 5, 60 + ty)
    eng = engine(cid, d.crs)
    try:
        check(eng, d, rho, "unforged", want_ok=[1, 1, 1])
        for name, stmts, bad in forged_sets(d):
            want = [0 if s in bad else 1 for s in range(3)]
            # (the cells of the unchanged equations come from the cache: at most 5 new oracle equations per variant)
            check(eng, d, rho, name, stmts=stmts, want_ok=want)
    finally:
        eng.close()


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_forgeries_with_one_lane_per_statement(cname, cid, ty):
    """The one-lane final kernel (k_stmt_final; the planner takes it once S fills the chip) on forged input: the unforged
    statements, a forged target in statement 1 and a forged commitment in statement 2, coop_fe = 0."""
    d = data(cname, cid, ty, 3, 5, 2, 2)
    rho = seeded_rho(3, 5, 70 + ty)
    eng = engine(cid, d.crs, {"coop_fe": 0})
    try:
        eng.prof_enable(True)
        eng.prof_reset()
        ok, _ = run_dev(eng, d, d.arrays(), rho)
        names = [p[0] for p in eng.prof_get()]
        eng.prof_enable(False)
        assert ok.all() and "k_stmt_final" in names and "k_stmt_final.coop" not in names, names
        sets = {nm: (st, bad) for nm, st, bad in forged_sets(d)}
        for name in ("target of equation 4: the unsatisfied twin's", "theta[2][0].0 += gen", "statement 2: xcoms[0].1 += gen"):
            stmts, bad = sets[name]
            check(eng, d, rho, name, stmts=stmts, want_ok=[0 if s in bad else 1 for s in range(3)])
    finally:
        eng.close()


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_rho_edges_on_first_and_last_equation(cname, cid, ty):
    """Every edge value, all four cells equal, and the mixed row on the first and on the last equation of a statement
    whose first and last equations are BOTH wrong (their cells' values depend on those exponents); every type, since
    rho reaches the scalar-constant and QuadEqu-target sums and the fixed-base lanes only there.  (The oracle's cells do
    not depend on rho: 15 equations per type go through it once.)"""
    d = data(cname, cid, ty, 3, 5, 2, 2)
    sets = {nm: st for nm, st, _ in forged_sets(d)}
    stmts = [dict(s) for s in d.stmts]
    stmts[1]["theta"] = sets["theta[0][0].0 += gen"][1]["theta"].copy()
    sz = stmtrlc.shape(ty)[3] * 2 * forge.Ctx(cname, d.crs).G1  # the ky theta elements of one equation
    stmts[1]["theta"][4 * sz:] = sets["theta[4][0].0 += gen"][1]["theta"][4 * sz:]
    eng = engine(cid, d.crs)
    try:
        for i, v in enumerate(EDGE_RHO + [None]):
            rho = seeded_rho(3, 5, 80 + i)
            row = np.array(MIXED_ROW if v is None else [v] * 4, dtype=np.uint64)
            rho[1][0] = row
            rho[1][4] = row[::-1]
            check(eng, d, rho, "edge %r" % (v,), stmts=stmts, want_ok=[1, 0, 1], exact=False)
    finally:
        eng.close()


# ---- d. rho is used per equation and per cell ------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,cid", CURVES)
def test_cancelling_targets_within_one_statement(cname, cid):
    """Two PPE targets of ONE statement multiplied by z and 1 / z: accepted with equal rho[.][3], rejected with different
    ones, and the oracle's formula says the same both times."""
    d = data(cname, cid, 0, 3, 5, 2, 2)
    cx = forge.Ctx(cname, d.crs)
    z = ref.gt_pow(cname, cx.gt, cx.fr(0xABCDEF0123456789ABCDEF))
    GT = cx.GT
    stmts = [dict(s) for s in d.stmts]
    t = forge.u8(stmts[1]["target"])
    t[1 * GT:2 * GT] = ref.gt_mul(cname, t[1 * GT:2 * GT], z)
    t[3 * GT:4 * GT] = ref.gt_mul(cname, t[3 * GT:4 * GT], ref.gt_inv(cname, z))
    stmts[1]["target"] = t
    eng = engine(cid, d.crs)
    try:
        rho = seeded_rho(3, 5, 31)
        rho[1][1][3] = rho[1][3][3] = (1 << 63) + 12345
        check(eng, d, rho, "z, 1/z, equal rho", stmts=stmts, want_ok=[1, 1, 1], exact=False)
        each = eng.verify_statement(0, 5, 2, 2, *[stmts[1][k] for k in KEYS])
        assert [int(v) for v in each] == [1, 0, 1, 0, 1]  # (what the exact verifier says of the two equations)
        rho[1][3][3] += 1
        check(eng, d, rho, "z, 1/z, different rho", stmts=stmts, want_ok=[1, 0, 1], exact=False)
    finally:
        eng.close()


# ---- f. the pairing work does not grow with E --------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_pairing_work_does_not_grow_with_E(cname, cid, ty):
    work = {}
    for E in (1, 9):
        d = data(cname, cid, ty, 3, E, 3, 1)
        eng = engine(cid, d.crs)
        try:
            eng.prof_enable(True)
            eng.prof_reset()
            ok, _ = run_dev(eng, d, d.arrays(), seeded_rho(3, E, 5))
            prof = eng.prof_get_work()
            eng.prof_enable(False)
        finally:
            eng.close()
        assert ok.all()
        millers = [nm for nm in prof if nm.startswith("k_miller")]
        assert millers == ["k_miller.srlc"], millers
        assert "k_prep_verify_stmt_rlc" in prof and any(nm.startswith("k_stmt_final") for nm in prof), sorted(prof)
        work[E] = prof["k_miller.srlc"]
    assert work[1] == work[9], work
    lanes, pairs = work[1]
    assert pairs <= 3 * stmtrlc.pair_count(ty, 3, 1)  # (a table-read CRS pair counts below one stepped pair)


# ---- g. errors ------------------------------------------------------------------------------------------------------------------
def test_errors():
    import groth_sahai_rs_amd as gs

    d = data("bls12_381", 0, 0, 1, 1, 1, 1)
    eng = engine(0, d.crs)
    try:
        arrays = d.arrays()
        rho = seeded_rho(1, 1, 1)
        zero = rho.copy()
        zero[0][0][2] = 0
        with pytest.raises(gs.GsError) as ei:
            eng.verify_statements_rlc(0, 1, 1, 1, 1, *arrays, zero)
        assert ei.value.code == 3 and "rho" in str(ei.value)
        # short arrays are refused by the binding (GS_ERR_SHAPE) before a pointer crosses the C ABI
        for i, k in enumerate(KEYS):
            short = list(arrays)
            short[i] = arrays[i][:-1]
            with pytest.raises(gs.GsError) as ei:
                eng.verify_statements_rlc(0, 1, 1, 1, 1, *short, rho)
            assert ei.value.code == 1, k
        with pytest.raises(gs.GsError) as ei:
            eng.verify_statements_rlc(0, 1, 1, 1, 1, *arrays, rho.reshape(-1)[:3])
        assert ei.value.code == 1
        # S = 0 or E = 0: GS_ERR_ARG from the C entries themselves
        buf = np.ones(1 << 16, dtype=np.uint8)
        p = ctypes.c_void_p(buf.ctypes.data)
        z = lambda v: ctypes.c_size_t(v)
        for S, E in ((0, 1), (1, 0)):
            assert eng.lib.gs_verify_statements_rlc(eng.ctx, 0, z(S), z(E), 1, 1, *[p] * 11) == 3, (S, E)
            assert eng.lib.gs_verify_statements_rlc_dev(eng.ctx, 0, z(S), z(E), 1, 1, *[p] * 11) == 3, (S, E)
            with pytest.raises(gs.GsError) as ei:
                eng.verify_statements_rlc(0, S, E, 1, 1, *arrays, rho)
            assert ei.value.code == 3
        # a statement the plan cannot index (32-bit byte strides per statement) is refused, not truncated
        assert eng.lib.gs_verify_statements_rlc_dev(eng.ctx, 0, z(1), z(1 << 24), 4, 4, *[p] * 11) == 1
    finally:
        eng.close()


def test_a_thousand_equations_per_statement():
    """E = 1024 at 4 x 4 is within what the plan indexes (PPE, one statement; the verdict against the exact verifier:
    no oracle at this size)."""
    d = data("bls12_381", 0, 0, 1, 1024, 4, 4)
    eng = engine(0, d.crs)
    try:
        rho = seeded_rho(1, 1024, 2)
        ok, acc = eng.verify_statements_rlc(0, 1, 1024, 4, 4, *d.arrays(), rho)
        assert ok[0] == 1 and eng.gt_finalize(acc.reshape(-1)) == 1
        st = dict(d.stmts[0])
        cx = forge.Ctx("bls12_381", d.crs)
        off = 1023 * 2 * 2 * cx.G1  # theta of the LAST equation
        th = forge.u8(st["theta"])
        th[off:off + cx.G1] = cx.add(1, th[off:off + cx.G1], cx.g1)
        st["theta"] = th
        ok, _ = eng.verify_statements_rlc(0, 1, 1024, 4, 4, *d.arrays([st]), rho)
        assert ok[0] == 0
    finally:
        eng.close()

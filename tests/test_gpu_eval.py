"""gs_eval_* / gs_check_witness_* on the device: what an equation evaluates to at a witness (include/gs_amd.h,
DESIGN.md 6.8), all four types, both curves.

Expectations come from routes that share nothing with the device path, which FOLDS the Gamma term (W_j = A_j + sum_i
Gamma_ij X_i for PPE; c_i, d_j in Fr for the other types):
  * the golden targets and the targets of sparsevec / workload batches: from discrete logarithms;
  * tests/evalvec.term_by_term: the C oracle's primitives, one term of src/statement.rs:17-21 at a time, no folding.
Bytes are compared, never tolerances: every value has ONE representation (canonical limbs, normalised affine points, the
identity all-zero).  Every case makes its own engine and closes it; oracle batches are computed once and shared.
Not tested: the refusal inside a mixed call.  The library refuses the entries while a gs_*_mixed call records its
launches, but nothing a caller can do through the C ABI runs another entry in that window, so no test can reach it."""
import contextlib
import ctypes

import numpy as np
import pytest

import evalvec as ev
import sparsevec as sv
from forge import golden_crs, u8, xg, yg
from gsutil import curve

pytestmark = pytest.mark.gpu

CURVE_IDS = [("bls12_381", 0), ("bn254", 1)]
TYPES = [0, 1, 2, 3]
IN = ("X", "Y", "A", "B", "G")


_ANCHORS = {}


@pytest.fixture(scope="module", autouse=True)
def _anchors():
    """The CRS tables are shared by the contexts of a process that install the same bytes and die with the last of them
    (include/gs_amd.h, gs_set_crs).  One idle engine per CRS of this file keeps them alive between the cases, so that a
    case's own engine does not build them again."""
    yield
    for e in _ANCHORS.values():
        e.close()
    _ANCHORS.clear()


def new_engine(cid, crs=None, opts=None):
    import groth_sahai_rs_amd as gs

    if crs is not None:
        key = (cid, np.asarray(crs).tobytes())
        if key not in _ANCHORS:
            _ANCHORS[key] = gs.Engine(cid, 0)
            _ANCHORS[key].set_crs(crs)
    eng = gs.Engine(cid, 0)
    try:
        for k, v in (opts or {}).items():
            eng.set_option(k, v)
        if crs is not None:
            eng.set_crs(crs)
    except BaseException:
        eng.close()
        raise
    return eng


@contextlib.contextmanager
def engine(cid, crs=None, opts=None):
    eng = new_engine(cid, crs, opts)
    try:
        yield eng
    finally:
        eng.close()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rows(a, N):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.reshape(N, -1)


def bad_rows(got, want, N):
    return [int(e) for e in np.nonzero((rows(got, N) != rows(want, N)).any(axis=1))[0]]


# ---- 1. golden ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_golden_targets(cname, cid):
    """gs_eval_batch (host form, N = 1) on every golden case reproduces its target byte for byte; the check accepts it."""
    c = curve(cname)
    with engine(cid, golden_crs(c)) as eng:
        seen = set()
        for k, case in enumerate(c.golden["cases"]):
            ty, m, n = case["type"], case["m"], case["n"]
            ex, ey = (c.g1 if xg(ty) else c.fr_hex), (c.g2 if yg(ty) else c.fr_hex)
            cat = lambda f, vals: u8(np.concatenate([f(v) for v in vals]))
            X, Y, A, B = cat(ex, case["xvars"]), cat(ey, case["yvars"]), cat(ex, case["a"]), cat(ey, case["b"])
            G = u8(c.fr_mat(case["gamma"]))
            want = u8({0: c.f12, 1: c.g1, 2: c.g2, 3: c.fr_hex}[ty](case["target"]))
            got = eng.eval_batch(ty, 1, m, n, X, Y, A, B, G)
            assert (got.reshape(-1) == want).all(), (cname, "case", k, "type", ty)
            assert eng.check_witness_batch(ty, 1, m, n, X, Y, A, B, G, want).tolist() == [1], (cname, "case", k)
            seen.add(ty)
        assert seen == {0, 1, 2, 3}


# ---- 2. term by term ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 1), (1, 5)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_term_by_term(cname, cid, ty, m, n):
    """N = 3 equations per shape against the unfolded sums of the C oracle's primitives (and the discrete-log targets)."""
    N = 3
    b = ev.dense(cname, ty, m, n, N, 0xE7A100 + 97 * m + n)
    want = np.concatenate([ev.term_by_term(cname, ty, m, n, q) for q in b["eqs"]])
    assert (want == b["target"]).all(), "the two expectations disagree"
    with engine(cid, b["crs"]) as eng:
        got = eng.eval_batch(ty, N, m, n, *(b[k] for k in IN))
        assert bad_rows(got, want, N) == [], (cname, ty, m, n)
        assert eng.check_witness_batch(ty, N, m, n, *(b[k] for k in IN), want).tolist() == [1] * N


# ---- 3. sparse and degenerate statements --------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_sparse_and_degenerate_statements(cname, cid, ty):
    """All 36 patterns of sparsevec (N = 72, 4 x 4): identity variables and constants, sparse Gamma, cancelling sums,
    everything the identity.  The value equals the target of every true statement; the check says 0 exactly on the false
    twins."""
    b = sv.expected(cname, ty)
    N, m, n = b["N"], b["m"], b["n"]
    assert N == 72 and sorted({b["names"][e] for e in b["false"]}) == sorted(sv.FALSE_TWINS)
    arrs = [sv.pack(b, k) for k in IN]
    target = sv.pack(b, "target")
    with engine(cid, b["crs"]) as eng:
        got = eng.eval_batch(ty, N, m, n, *arrs)
        bad = bad_rows(got, target, N)
        assert bad == sorted(b["false"]), (cname, ty, [b["names"][e] for e in bad])
        ok = eng.check_witness_batch(ty, N, m, n, *arrs, target)
        assert ok.tolist() == [0 if e in b["false"] else 1 for e in range(N)], (cname, ty)
        # the device forms on the same arrays
        import torch

        d = [dev(a) for a in arrs]
        tout = torch.zeros(target.size, dtype=torch.uint8, device="cuda:0")
        okd = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
        eng.eval_batch_dev(ty, N, m, n, *d, tout)
        eng.check_witness_batch_dev(ty, N, m, n, *d, dev(target), okd)
        eng.sync()
        assert (tout.cpu().numpy() == got.reshape(-1)).all() and (okd.cpu().numpy() == ok).all()


# ---- workload batches: device-resident, targets from discrete logarithms --------------------------------------------
class Batch:
    """A Workload on its own engine."""

    SEED = 0xE7A1  # one seed, hence ONE CRS per curve, for every batch of this file (the equations differ by type and shape)

    def __init__(self, cid, ty, N, m, n):
        from groth_sahai_rs_amd.workload import Workload

        self.eng = new_engine(cid)
        try:
            self.wl = Workload(self.eng, ty=ty, N=N, m=m, n=n, seed=self.SEED, corrupt_every=0)
            new_engine(cid, self.wl.crs).close()  # (anchors the tables the workload has just built)
        except BaseException:
            self.eng.close()
            raise
        self.cid, self.ty, self.N, self.m, self.n = cid, ty, N, m, n

    def close(self):
        self.eng.close()

    def arrays(self, N=None):
        """the first N equations' X, Y, A, B, Gamma and target (device tensors; views of the batch)"""
        wl, sh = self.wl, self.wl.sh
        N = self.N if N is None else N
        return ([wl.X[:N * self.m * sh["sx"]], wl.Y[:N * self.n * sh["sy"]], wl.A[:N * self.n * sh["sx"]],
                 wl.B[:N * self.m * sh["sy"]], wl.Gamma[:N * self.m * self.n * 32]], wl.target[:N * sh["st"]])

    def evaluate(self, eng, N=None):
        """(value bytes, ok) of the first N equations on `eng`, device forms"""
        import torch

        N = self.N if N is None else N
        ins, target = self.arrays(N)
        out = torch.zeros(target.numel(), dtype=torch.uint8, device="cuda:0")
        ok = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
        eng.eval_batch_dev(self.ty, N, self.m, self.n, *ins, out)
        eng.check_witness_batch_dev(self.ty, N, self.m, self.n, *ins, target, ok)
        eng.sync()
        return out.cpu().numpy(), ok.cpu().numpy()


# ---- 4. forced kernel shapes --------------------------------------------------------------------------------------
FORCED = [("var_tm", 1), ("var_tm", 2), ("var_tm", 4), ("var_tm", 8), ("var_mo", 1), ("var_mo", 2), ("var_mo", 4),
          ("var_w", 4), ("var_w", 5), ("var_w2", 0), ("var_w2", 1), ("red_k", 1), ("red_k", 8), ("miller_ch", 1),
          ("miller_ch", 3), ("miller_ch", 12), ("coop_fe", 0), ("coop_fe", 2), ("endo", 0), ("endo", 1), ("var_tab", 1)]


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_forced_kernel_shapes(cname, cid, ty):
    """N = 65 and N = 130 (one and two wave boundaries), ONE option forced at a time: the bytes equal the unforced bytes
    and the discrete-log targets, and the check accepts every equation.  ("var_tab" acts on the PPE only.)"""
    b = Batch(cid, ty, 130, 4, 4)
    try:
        want = b.wl.target.cpu().numpy()
        base = {}
        for N in (65, 130):
            base[N], ok = b.evaluate(b.eng, N)
            assert bad_rows(base[N], want[:base[N].size], N) == [], (cname, ty, N, "unforced")
            assert ok.tolist() == [1] * N
        for key, val in FORCED:
            if key == "var_tab" and ty != 0:
                continue
            with engine(cid, b.wl.crs, {key: val}) as eng:
                for N in (65, 130):
                    got, ok = b.evaluate(eng, N)
                    assert bad_rows(got, base[N], N) == [], (cname, ty, N, key, val)
                    assert ok.tolist() == [1] * N, (cname, ty, N, key, val)
    finally:
        b.close()


# ---- 5. large arity -----------------------------------------------------------------------------------------------
# wide_prep(m, n) holds from m * n = 1024 on (csrc/gs_amd.hip): 32 x 32 is the smallest square shape; 31 x 33 = 1023 is
# the largest below it with the same number of variables.  70 x 130 PPE: 200 pairs per equation, 17 Miller partials:
# k_cell_fold; n >= 32: the shared window tables.  129 x 128 MSMEG1: 257 terms, 33 partial sums: k_slot_fold.
LARGE = [(ty, 32, 32) for ty in TYPES] + [(ty, 31, 33) for ty in TYPES] + [(0, 70, 130), (1, 129, 128)]


@pytest.mark.parametrize("ty,m,n", LARGE)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_large_arity(cname, cid, ty, m, n):
    N = 2
    b = Batch(cid, ty, N, m, n)
    try:
        b.eng.prof_enable(True)
        b.eng.prof_reset()
        got, ok = b.evaluate(b.eng)
        names = [p[0] for p in b.eng.prof_get()]
        b.eng.prof_enable(False)
        assert bad_rows(got, b.wl.target, N) == [], (cname, ty, m, n, names)
        assert ok.tolist() == [1] * N
        if m * n >= 1024:
            assert ("k_fr_canonical" if ty == 0 else "k_prep_eval.a") in names, names
        else:
            assert "k_prep_eval" in names and "k_prep_eval.a" not in names and "k_fr_canonical" not in names, names
        if (ty, m, n) == (0, 70, 130):
            assert "k_cell_fold" in names and "k_var_tab8.ev1" in names, names
        if (ty, m, n) == (1, 129, 128):
            assert "k_slot_fold.ev1" in names, names
        again, _ = b.evaluate(b.eng)  # unprofiled: the same bytes
        assert (again == got).all()
    finally:
        b.close()


# ---- 6. statements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_statement_equals_replicated_batch(cname, cid, ty):
    """E = 5 equations over ONE copy of X[m], Y[n] equal gs_eval_batch with the variables replicated, host and _dev."""
    import torch

    E, m, n = 5, 2, 3
    b = ev.dense(cname, ty, m, n, E, 0xE7A600 + ty)
    X0, Y0 = b["eqs"][0]["X"], b["eqs"][0]["Y"]
    Xr, Yr = np.tile(X0, E), np.tile(Y0, E)
    with engine(cid, b["crs"]) as eng:
        want = eng.eval_batch(ty, E, m, n, Xr, Yr, b["A"], b["B"], b["G"])
        got = eng.eval_statement(ty, E, m, n, X0, Y0, b["A"], b["B"], b["G"])
        assert bad_rows(got, want, E) == []
        # equation 0 keeps its own witness: its discrete-log target; the others are other values
        assert (got[0] == b["eqs"][0]["target"]).all()
        assert eng.check_witness_statement(ty, E, m, n, X0, Y0, b["A"], b["B"], b["G"], want).tolist() == [1] * E
        assert eng.check_witness_statement(ty, E, m, n, X0, Y0, b["A"], b["B"], b["G"], b["target"]).tolist() == \
            [1, 0, 0, 0, 0]
        d = {k: dev(v) for k, v in dict(X0=X0, Y0=Y0, Xr=Xr, Yr=Yr, A=b["A"], B=b["B"], G=b["G"]).items()}
        o1 = torch.zeros(want.size, dtype=torch.uint8, device="cuda:0")
        o2 = torch.zeros(want.size, dtype=torch.uint8, device="cuda:0")
        ok = torch.full((E,), 7, dtype=torch.uint8, device="cuda:0")
        eng.eval_batch_dev(ty, E, m, n, d["Xr"], d["Yr"], d["A"], d["B"], d["G"], o1)
        eng.eval_statement_dev(ty, E, m, n, d["X0"], d["Y0"], d["A"], d["B"], d["G"], o2)
        eng.check_witness_statement_dev(ty, E, m, n, d["X0"], d["Y0"], d["A"], d["B"], d["G"], dev(b["target"]), ok)
        eng.sync()
        assert (o1.cpu().numpy() == want.reshape(-1)).all() and (o2.cpu().numpy() == want.reshape(-1)).all()
        assert ok.cpu().numpy().tolist() == [1, 0, 0, 0, 0]


# ---- 7. round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_round_trip_with_prover_and_verifier(cname, cid, ty):
    """Evaluate, prove, verify against the EVALUATED target, all enqueued on the context's stream with no sync in
    between: every proof verifies.  With the witness of equation 7 changed, the check says 0 for equation 7 only, and the
    verifier rejects the proof made from that witness against the old target."""
    import torch

    N, m, n = 65, 4, 4
    b = Batch(cid, ty, N, m, n)
    try:
        eng, wl = b.eng, b.wl
        ins, target = b.arrays()
        mine = torch.zeros(target.numel(), dtype=torch.uint8, device="cuda:0")
        ok = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")

        def prove_and_verify(tgt):
            eng.prove_batch_dev(ty, N, m, n, *ins, wl.R, wl.S, wl.T, wl.xcoms, wl.ycoms, wl.pi, wl.theta)
            eng.verify_batch_dev(ty, N, m, n, wl.A, wl.B, wl.Gamma, tgt, wl.xcoms, wl.ycoms, wl.pi, wl.theta, ok)

        eng.eval_batch_dev(ty, N, m, n, *ins, mine)
        prove_and_verify(mine)
        eng.sync()
        assert ok.cpu().numpy().tolist() == [1] * N, (cname, ty)
        assert (mine == target).all()
        # equation 7 gets equation 8's first X variable
        sx = wl.sh["sx"]
        wl.X[7 * m * sx:7 * m * sx + sx] = wl.X[8 * m * sx:8 * m * sx + sx].clone()
        chk = torch.full((N,), 7, dtype=torch.uint8, device="cuda:0")
        eng.check_witness_batch_dev(ty, N, m, n, *ins, mine, chk)
        prove_and_verify(mine)
        eng.sync()
        want = [0 if e == 7 else 1 for e in range(N)]
        assert chk.cpu().numpy().tolist() == want, (cname, ty, "check_witness")
        assert ok.cpu().numpy().tolist() == want, (cname, ty, "verifier")
    finally:
        b.close()


# ---- the mirror: Equation.evaluate / is_satisfied_by / from_witness, Statement ------------------------------------------
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_mirror_evaluate_and_from_witness(cname, cid):
    """On the golden cases: evaluate gives the recorded target, the recorded witness satisfies the equation, from_witness
    builds the equation whose proof verifies, a changed Gamma is not satisfied, and a Statement of same-type equations
    over the shared variables agrees with its equations taken alone."""
    from groth_sahai_rs_amd import mirror
    from test_gpu_mirror import ReplayRng, build

    c = curve(cname)
    g = c.golden["crs"]
    crs = mirror.CRS([c.com1(g["u"][0]), c.com1(g["u"][1])], [c.com2(g["v"][0]), c.com2(g["v"][1])], c.g1(g["g1"]),
                     c.g2(g["g2"]), c.f12(g["gt"]), curve=cid)
    try:
        for case in c.golden["cases"]:
            equ, xvars, yvars = build(c, mirror, case)
            want = np.asarray(equ.target, dtype=np.uint64).reshape(-1)
            assert (equ.evaluate(xvars, yvars, crs) == want).all(), case["name"]
            assert equ.is_satisfied_by(xvars, yvars, crs) is True
            made = type(equ).from_witness(equ.a_consts, equ.b_consts, equ.gamma, xvars, yvars, crs)
            assert (np.asarray(made.target).reshape(-1) == want).all()
            proof = made.commit_and_prove(xvars, yvars, crs, ReplayRng(c, [case["R"], case["S"], case["T"]]))
            assert made.verify(proof, crs)
            other = type(equ)(equ.a_consts, equ.b_consts, [list(row) for row in equ.gamma], equ.target)
            other.gamma[0][0] = c.fr(7) if not (np.asarray(equ.gamma[0][0]) == c.fr(7)).all() else c.fr(8)
            assert other.is_satisfied_by(xvars, yvars, crs) is False, case["name"]
            st = mirror.Statement([equ, other, made])
            vals = st.evaluate(xvars, yvars, crs)
            assert (vals[0] == want).all() and (vals[2] == want).all()
            assert (vals[1] == other.evaluate(xvars, yvars, crs)).all() and not (vals[1] == want).all()
            assert st.is_satisfied_by(xvars, yvars, crs) == [True, False, True]
            with pytest.raises(AssertionError):
                equ.evaluate(xvars + xvars[:1], yvars, crs)
    finally:
        crs.engine.close()


# ---- 8. pair count ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_pair_count(cname, cid):
    """m + n Miller pairs per equation, not 2n + m: gs_prof_get_work of "k_miller.eval" on a dense 4 x 4 PPE batch."""
    N, m, n = 65, 4, 4
    b = Batch(cid, 0, N, m, n)
    try:
        b.eng.prof_enable(True)
        b.eng.prof_reset()
        b.evaluate(b.eng)
        work = b.eng.prof_get_work()
        b.eng.prof_enable(False)
        # (evaluate() runs the entry twice: gs_eval_batch_dev and gs_check_witness_batch_dev)
        lanes, pairs = work["k_miller.eval"]
        assert pairs == 2 * N * (m + n), work
        assert any(k.startswith("k_final_eval") for k in work) and "k_final" not in work, work
    finally:
        b.close()


# ---- 9. status ----------------------------------------------------------------------------------------------------
def _raw(eng, fn, ty, N, m, n, *ptrs):
    """the C entry itself: the binding's own checks are not in the way"""
    p = [ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p(0) for a in ptrs]
    return getattr(eng.lib, fn)(eng.ctx, ty, N, m, n, *p)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_status_codes(cname, cid, ty):
    N, m, n = 3, 2, 3
    b = ev.dense(cname, ty, m, n, N, 0xE7A900 + ty)
    ins = [np.ascontiguousarray(b[k]) for k in IN]
    target = np.ascontiguousarray(b["target"])
    st = target.size // N
    with engine(cid) as eng:  # no CRS
        out = np.full(target.size, 7, np.uint8)
        assert _raw(eng, "gs_eval_batch", ty, N, m, n, *ins, out) == 4
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, target, np.zeros(N, np.uint8)) == 4
        assert (out == 7).all()
    with engine(cid, b["crs"]) as eng:
        out, ok = np.full(target.size, 7, np.uint8), np.full(N, 7, np.uint8)
        # N = 0: a no-op, outputs untouched (null inputs are not looked at)
        assert _raw(eng, "gs_eval_batch", ty, 0, m, n, *ins, out) == 0
        assert _raw(eng, "gs_eval_statement", ty, 0, m, n, None, None, None, None, None, out) == 0
        assert _raw(eng, "gs_check_witness_batch", ty, 0, m, n, *ins, target, ok) == 0
        assert (out == 7).all() and (ok == 7).all()
        # shapes
        assert _raw(eng, "gs_eval_batch", ty, N, 0, n, *ins, out) == 1
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, 0, *ins, target, ok) == 1
        assert _raw(eng, "gs_eval_batch", 4, N, m, n, *ins, out) == 3
        # null pointers
        for k in range(5):
            holed = list(ins)
            holed[k] = None
            assert _raw(eng, "gs_eval_batch", ty, N, m, n, *holed, out) == 3, IN[k]
            assert _raw(eng, "gs_check_witness_statement", ty, N, m, n, *holed, target, ok) == 3, IN[k]
        assert _raw(eng, "gs_eval_batch", ty, N, m, n, *ins, None) == 3
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, None, ok) == 3
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, target, None) == 3
        assert (out == 7).all() and (ok == 7).all()
        # a host output that overlaps an input
        buf = np.zeros(ins[0].size + target.size, np.uint8)
        buf[:ins[0].size] = ins[0]
        inside = buf[ins[0].size - st // 2:ins[0].size - st // 2 + target.size]  # starts inside X
        assert _raw(eng, "gs_eval_batch", ty, N, m, n, buf[:ins[0].size], *ins[1:], inside) == 3
        assert b"overlap" in eng.lib.gs_last_error(eng.ctx)
        tb = np.concatenate([target, np.zeros(N, np.uint8)])
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, tb[:target.size], tb[target.size - 1:][:N]) == 3
        # the calls themselves, and a target with non-canonical limbs: value + modulus in the first field element
        assert _raw(eng, "gs_eval_batch", ty, N, m, n, *ins, out) == 0 and (out == target).all()
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, target, ok) == 0 and ok.tolist() == [1] * N
        c = curve(cname)
        mod, words = (c.r, 4) if ty == 3 else (c.p, c.nq)
        forged = target.copy()
        limbs = forged[st:st + 8 * words].view(np.uint64)  # equation 1
        v = sum(int(x) << (64 * i) for i, x in enumerate(limbs)) + mod
        assert v < 1 << (64 * words)
        limbs[:] = [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(words)]
        assert _raw(eng, "gs_check_witness_batch", ty, N, m, n, *ins, forged, ok) == 0
        assert ok.tolist() == [1, 0, 1], (cname, ty, "a non-canonical target matched")

"""A long-lived context: what a call returns must not depend on the calls before it.

The other GPU tests run one shape in a fresh context.  A gs_ctx keeps grow-only named scratch buffers (prove.pool,
verify.mpart, rlc.t, eqrlc.sums, fin.*, stage.<k>, *.tabws ...), a content-addressed cache of task tables that evicts
past GS_PLAN_CAP entries, planner decisions, an extraction key, dlog tables and a reference on the shared CRS tables.
Here one context serves scripted sequences of calls (tests/ctxhist.py: the table of calls and their oracle-checked
expected bytes), changes its CRS while another context holds the old one, and sees enough shapes to evict.  Every
comparison is byte for byte with what a fresh context gave, which was held to the oracle.

The orders are literal and fixed: a failure names the step and its predecessor."""
import os
import re

import numpy as np
import pytest

import ctxhist as H
from gsutil import REPO

CURVES = H.CURVES

# step: a call of the table | ("opt", key, value) | ("err", "shape" | "arg")
# Each order: a family's grower (N = 1024) before its small calls; another (m, n), another type, the first shape again;
# forged before valid at equal or smaller N and the other way round (stale ok / cellok / frontier / info / accumulators);
# gt_finalize over 8 pairs before 1; host-pointer calls between _dev calls (the stage.<k> slots); a two-part mixed call
# between plain ones (scratch tags, the recorder); refused calls between good ones; planner options switched and back.
ORDER_VERIFIERS = [
    ("prove", 0, 1024, 4, 4),
    ("prove", 0, 5, 4, 4),
    ("prove", 0, 65, 2, 3),
    ("prove", 3, 65, 4, 4),
    ("prove", 0, 5, 4, 4),
    ("verify", 0, 1024, 4, 4, "forged"),
    ("verify", 0, 300, 4, 4, "valid"),
    ("verify", 0, 300, 4, 4, "forged"),
    ("verify_host", 0, 5, 4, 4, "valid"),
    ("verify", 1, 65, 6, 2, "forged"),
    ("verify", 0, 5, 4, 4, "valid"),
    ("err", "shape"),
    ("verify", 0, 5, 4, 4, "forged"),
    ("rlc", 0, 1024, 4, 4, "forged", 8),
    ("rlc", 0, 300, 4, 4, "valid", 1),
    ("opt", "endo", 0),
    ("rlc", 0, 65, 2, 3, "forged", 1),
    ("opt", "endo", 1),
    ("rlc", 2, 65, 2, 3, "valid", 8),
    ("rlc", 0, 300, 4, 4, "valid", 1),
    ("mixed", 65),
    ("locate", 0, 1024, 4, 4, "forged"),
    ("locate", 0, 300, 4, 4, "valid"),
    ("err", "arg"),
    ("locate", 0, 300, 4, 4, "forged"),
    ("locate", 3, 5, 1, 1, "forged"),
    ("prove_host", 0, 5, 4, 4),
    ("locate", 0, 300, 4, 4, "valid"),
    ("opt", "overlap", 0),
    ("prove", 0, 65, 2, 3),
    ("verify", 0, 300, 4, 4, "valid"),
    ("opt", "overlap", 1),
    ("prove", 0, 65, 2, 3),
]
ORDER_FAMILIES = [
    ("eqrlc", 0, 1024, 4, 4, "forged"),
    ("eqrlc", 0, 5, 4, 4, "valid"),
    ("eqrlc", 0, 65, 2, 3, "valid"),
    ("eqrlc", 3, 65, 4, 4, "forged"),
    ("eqrlc", 0, 5, 4, 4, "valid"),
    ("eqrlc", 0, 5, 4, 4, "forged"),
    ("stmtrlc", 0, 8, 128, "forged"),
    ("stmtrlc", 0, 2, 3, "valid"),
    ("stmtrlc", 3, 5, 2, "forged"),
    ("stmtrlc", 0, 2, 3, "forged"),
    ("stmtrlc", 0, 2, 3, "valid"),
    ("rerand", 0, 1024, 4, 4),
    ("rerand", 0, 5, 4, 4),
    ("rerand", 1, 65, 6, 2),
    ("rerand_host", 0, 5, 4, 4),
    ("rerand", 0, 5, 4, 4),
    ("commit", "g1", 1024, 4),
    ("commit", "g1", 5, 4),
    ("commit", "fr_b1", 65, 4),
    ("commit", "g2", 5, 4),
    ("extract", 1, 1024, 4),
    ("extract", 1, 5, 4),
    ("extract", 2, 5, 4),
    ("xscalar", 300),
    ("xscalar", 5),
    ("err", "shape"),
    ("gmul", 1, 1024),
    ("gmul", 1, 65),
    ("gmul", 2, 65),
    ("opt", "endo", 0),
    ("gmul", 1, 65),
    ("opt", "endo", 1),
    ("gtpow", 1024),
    ("gtpow", 5),
    ("mpair", 300, 2),
    ("mpair", 5, 3),
    ("leftmul", 1, 3, 4),
    ("validate", 1, 300),
    ("validate", 2, 65),
    ("validate", 1, 5),
    ("eqrlc", 0, 5, 4, 4, "valid"),
]
ORDER_OPTIONS = [
    ("opt", "var_tab", 1),
    ("verify", 0, 300, 4, 4, "valid"),
    ("opt", "var_tab", -1),
    ("verify", 0, 300, 4, 4, "valid"),
    ("opt", "line_tables", 0),
    ("verify", 0, 300, 4, 4, "forged"),
    ("rlc", 0, 300, 4, 4, "forged", 1),
    ("opt", "line_tables", 1),
    ("rlc", 0, 300, 4, 4, "forged", 1),
    ("opt", "coop_fe", 2),
    ("verify", 0, 5, 4, 4, "valid"),
    ("rlc", 0, 65, 2, 3, "valid", 1),
    ("opt", "coop_fe", 1),
    ("verify", 0, 5, 4, 4, "valid"),
    ("prove", 1, 300, 2, 3),
    ("prove", 1, 1, 1, 1),
    ("verify", 1, 300, 2, 3, "forged"),
    ("verify", 1, 1, 1, 1, "valid"),
    ("verify", 1, 1, 1, 1, "forged"),
    ("prove", 2, 300, 6, 2),
    ("verify", 2, 300, 6, 2, "valid"),
    ("prove", 3, 1, 6, 2),
    ("verify", 3, 1, 6, 2, "forged"),
    ("locate", 2, 300, 6, 2, "forged"),
    ("locate", 1, 1, 1, 1, "valid"),
    ("rlc", 3, 1, 6, 2, "valid", 8),
    ("rlc", 1, 300, 2, 3, "forged", 1),
    ("mixed", 65),
    ("rlc_host", 0, 65, 2, 3, "valid"),
    ("eqrlc", 3, 65, 4, 4, "valid"),
    ("err", "arg"),
    ("eqrlc", 3, 65, 4, 4, "forged"),
    ("rerand", 2, 300, 6, 2),
    ("prove", 1, 300, 2, 3),
]
ORDERS = {"verifiers": ORDER_VERIFIERS, "families": ORDER_FAMILIES, "options": ORDER_OPTIONS}


def refused(W, eng, kind):
    """A call the library refuses before it enqueues anything: the context is left as it was."""
    import ctypes

    import groth_sahai_rs_amd as gs

    call = W.call(("verify", 0, 5, 4, 4, "valid"))
    d = H.device_buffers(call)
    if kind == "shape":
        with pytest.raises(gs.GsError) as ei:  # a wrong-sized array never crosses the ABI
            eng.verify_batch_dev(0, 5, 4, 4, *(d[k] for k in W.VK[:7]), d["theta"][:-8], d["ok"])
        assert ei.value.code == 1
        p = lambda k: ctypes.c_void_p(d[k].data_ptr())
        rc = eng.lib.gs_verify_batch_dev(eng.ctx, 0, ctypes.c_size_t(5), 0, 4, *(p(k) for k in W.VK), p("ok"))
        assert rc == 1, rc  # GS_ERR_SHAPE from the library itself (m = 0)
    else:
        rc_call = W.call(("rlc", 0, 5, 4, 4, "valid", 1))
        d = H.device_buffers(rc_call)
        with pytest.raises(gs.GsError) as ei:
            eng.verify_batch_rlc_dev(0, 5, 4, 4, *(d[k] for k in W.VK), None, d["acc"])
        assert ei.value.code == 3  # GS_ERR_ARG: null rho


def planned(steps):
    """(index, step, options the step's expected bytes are a function of): the ACC_OPTIONS in force at a call of an
    accumulator-bearing family, () everywhere else"""
    cur = {}
    for i, st in enumerate(steps):
        if st[0] == "opt":
            cur[st[1]] = st[2]
        opts = ()
        if st[0] in H.ACC_FAMILIES:
            opts = tuple((k, cur[k]) for k, dflt in sorted(H.ACC_OPTIONS.items()) if cur.get(k, dflt) != dflt)
        yield i, st, opts


def run_order(W, eng, steps, runner=None):
    runner = runner or (lambda call: H.run_plain(eng, call))
    prev = None
    for i, st, opts in planned(steps):
        if st[0] == "opt":
            eng.set_option(st[1], st[2])
        elif st[0] == "err":
            refused(W, eng, st[1])
        else:
            call, want = W.call(st), W.expected(st, opts)
            W.prepare(eng, call)
            got = H.pack(runner(call))
            assert got == want, "step %d %r after %r: %s" % (i, st, prev, H.diff(got, want))
            if opts:  # the option moves acc[0] alone (pack order: acc first): acc[1], verdicts and info stay
                assert got[eng.GT:] == W.expected(st)[eng.GT:], "step %d %r: %r moved more than acc[0]" % (i, st, opts)
        prev = st


def precompute(W, steps):
    W.expected_many([(st, opts) for _, st, opts in planned(steps) if st[0] not in ("opt", "err")] +
                    [(("verify", 0, 5, 4, 4, "valid"), ()), (("rlc", 0, 5, 4, 4, "valid", 1), ())])


# ---- a. scripted sequences -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("cid,cname", CURVES)
def test_sequence_in_one_context(cid, cname, order):
    W = H.world(cid, cname)
    precompute(W, ORDERS[order])
    eng = W.fresh()
    try:
        run_order(W, eng, ORDERS[order])
    finally:
        eng.close()


# ---- b. changing the CRS of a live context ---------------------------------------------------------------------------
_CRS2 = {}


def second_crs(W):
    """Another binding CRS over the same generators (gs_crs_generate, other scalars), a context that keeps its tables
    alive, and the oracle-checked bytes of proving the (PPE, 5, 4, 4) batch under it in that fresh context."""
    import gs_ref_py as ref

    if W.cid not in _CRS2:
        sc = W.fr([v + 7 for v in (0x1234567, 0x89ABCDE, 0xF012345, 0x6789ABC)])
        e2 = W.gs.Engine(W.cid, 0)
        crs2 = e2.crs_generate(W.p1, W.p2, sc)
        assert not (crs2 == W.crs).all()
        e2.set_crs(crs2)
        name = ("prove", 0, 5, 4, 4)
        call = W.call(name)
        out = H.run_plain(e2, call)
        keys = ("X", "Y", "A", "B", "Gamma", "R", "S", "T")
        for e in range(5):
            a = W.cut(0, 5, 4, 4, call.ins, e)
            o = ref.commit_and_prove(W.cname, 0, 4, 4, *(a[k] for k in keys), crs2)
            g = W.cut(0, 5, 4, 4, out, e)
            assert all((o[k] == g[k]).all() for k in o), ("fresh prove under the second CRS", W.cname, e)
        _CRS2[W.cid] = dict(eng=e2, crs=crs2, prove=H.pack(out), out=out)
    return _CRS2[W.cid]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,cname", CURVES)
def test_crs_change_on_live_context(cid, cname):
    import gs_ref_py as ref

    W = H.world(cid, cname)
    P, V, X, XS = ("prove", 0, 5, 4, 4), ("verify", 0, 5, 4, 4, "valid"), ("extract", 1, 5, 4), ("xscalar", 5)
    VF = ("verify", 0, 5, 4, 4, "forged")
    for nm in (P, V, VF, X, XS):
        W.expected(nm)
    C2 = second_crs(W)
    b = W.batch(0, 5, 4, 4)
    a, other = W.fresh(), W.fresh()

    def same(eng, names, where):
        for nm in names:
            call = W.call(nm)
            W.prepare(eng, call)
            got = H.pack(H.run_plain(eng, call))
            assert got == W.expected(nm), "%s: %r: %s" % (where, nm, H.diff(got, W.expected(nm)))

    try:
        same(a, (P, V, X, XS, VF), "first CRS")
        same(other, (P, VF), "second context")
        # ---- the second CRS
        a.set_crs(C2["crs"])
        a._ctxhist_key = False
        got = H.run_plain(a, W.call(P))
        assert H.pack(got) == C2["prove"], "prove under the second CRS: " + H.diff(H.pack(got), C2["prove"])
        vk = dict(A=b["A"], B=b["B"], Gamma=b["Gamma"], target=b["target"])
        ok2 = a.verify_batch(0, 5, 4, 4, *(vk[k] for k in ("A", "B", "Gamma", "target")), got["xcoms"], got["ycoms"],
                             got["pi"], got["theta"])
        assert ok2.all(), ("a proof made under the second CRS", ok2)
        ok1 = a.verify_batch(0, 5, 4, 4, *(W.vargs(b, "valid")[k] for k in W.VK))
        assert not ok1.any(), ("a proof made under the first CRS verifies under the second", ok1)
        v = W.cut(0, 5, 4, 4, W.vargs(b, "valid"), 0)
        assert ref.verify(cname, 0, 4, 4, *(v[k] for k in W.VK), C2["crs"]) == 0
        with pytest.raises(W.gs.GsError) as ei:  # the key went with the CRS it was checked against
            a.extract(1, b["xcoms"])
        assert ei.value.code == 3
        # the dlog table is public data, not tied to the CRS: it still answers
        xs = [0, 1, 255, 256, 40000, (1 << H.DLOG_BITS) - 1]
        pts = a.g_mul_batch(1, W.p1, W.fr(xs).view(np.uint64), broadcast=True)
        out, found = a.dlog(1, pts, H.DLOG_BITS)
        assert found.all() and (out.reshape(-1) == W.fr(xs)).all()
        same(other, (P, VF, V), "second context while the first holds another CRS")
        # ---- back to the first
        a.set_crs(W.crs)
        with pytest.raises(W.gs.GsError) as ei:
            a.extract(1, b["xcoms"])
        assert ei.value.code == 3
        same(a, (P, V, VF, X, XS), "first CRS again")  # (prepare installs the key again; the dlog table is the old one)
        same(other, (P, VF), "second context at the end")
    finally:
        a.close()
        other.close()


# ---- c. eviction from the task-table cache ---------------------------------------------------------------------------
PLAN_CAP = 256
EVICT_MN = [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3), (4, 4), (5, 2), (2, 6)]
# 32 shapes, types interleaved; about 14 distinct tables each (499 were counted over 36 shapes)
EVICT_SHAPES = [(ty, m, n) for m, n in EVICT_MN for ty in (0, 1, 2, 3)]
EVICT_MARGIN = 1.5


def test_plan_cap_is_what_the_eviction_test_assumes():
    src = open(os.path.join(REPO, "groth_sahai_rs_amd", "csrc", "gs_amd.hip")).read()
    m = re.search(r"constexpr\s+size_t\s+GS_PLAN_CAP\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == PLAN_CAP


@pytest.mark.gpu
@pytest.mark.parametrize("cid,cname", CURVES)
def test_eviction_and_rerun(cid, cname, monkeypatch, capfd):
    W = H.world(cid, cname)
    names = lambda ty, m, n: [("prove", ty, 2, m, n), ("verify", ty, 2, m, n, "forged"), ("rlc", ty, 2, m, n, "valid", 1)]
    W.expected_many([(nm, ()) for s in EVICT_SHAPES for nm in names(*s)])
    eng = W.fresh()

    def go(shapes, where):
        for s in shapes:
            for nm in names(*s):
                got = H.pack(H.run_plain(eng, W.call(nm)))
                assert got == W.expected(nm), "%s: %r: %s" % (where, nm, H.diff(got, W.expected(nm)))

    try:
        capfd.readouterr()
        monkeypatch.setenv("GS_PLAN_TRACE", "1")
        go(EVICT_SHAPES, "first pass")
        monkeypatch.delenv("GS_PLAN_TRACE")
        err = capfd.readouterr().err
        tables = set(re.findall(r"^\[plan\] table \S+ \d+ [0-9a-f]{16}$", err, flags=re.M))
        assert len(tables) >= EVICT_MARGIN * PLAN_CAP, (
            "%d distinct task tables: the cache (cap %d) has not evicted with a margin of %.1fx" %
            (len(tables), PLAN_CAP, EVICT_MARGIN))
        print("distinct task tables before the re-runs: %d" % len(tables))
        go(EVICT_SHAPES[:10], "first ten again (evicted)")
        go(EVICT_SHAPES[-10:], "last ten again")
    finally:
        eng.close()

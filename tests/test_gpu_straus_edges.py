"""Every Straus kernel instance -- k_var_multi{4,8}[w5][x2|x4], their two-wave G1 builds, k_var_tab8 -- on the rows of
tests/strausvec.py: the scalar table at every term position, rows that must give the identity, and built collisions in
which the running sum of a lane meets the next table entry (the doubling branch behind the point subroutine's early
return) or its negative, at the top window, a middle window and window 0 of every sub-scalar stream that can be isolated.
gs_mat_left_mul_com1/2 take the bases and scalars directly and follow the forced var_tm / var_w / var_mo / var_w2 /
var_ws_lanes (and var_tab on com1), so every output is compared bit for bit.

All assertions are exact: every component of every row is the reference's [log] generator (oracle/gs_ref.c, and on a
sample the big-integer oracle and the reference's own left_mul); the identity rows are all zero bytes; the profile shows
the forced kernel and no one-term lanes; the outputs under the profile and without it are the same; the call with the
options back at their defaults gives the same bytes on k_var.lm.  tests/test_straus_cpu.py proves on the CPU that the rows
hold what they claim."""
import os
import sys

import numpy as np
import pytest

import strausvec as SV
from gsutil import REPO
from test_gpu_scalar_edges import CG, CURVES, ctx, profiled, same

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu

DEFAULTS = (("endo", 1), ("var_tm", 0), ("var_w", 0), ("var_mo", 0), ("var_tab", 0), ("var_w2", -1), ("var_ws_lanes", 0))
_CASES = {}


class Case:
    """The rows of one (curve, group, k): inputs, expectations, and the planned call's bytes.  Built once, shared by every
    shape, never modified."""

    def __init__(self, K, group, k):
        import gs_ref_py as ref

        cname, eng = K.cname, K.eng
        self.rows = SV.rows(cname, group, k)
        n = len(self.rows)
        self.labels = ["row %d: %s" % (i, rw.label) for i, rw in enumerate(self.rows)]
        self.col = np.concatenate([np.concatenate([K.mul(group, a), K.mul(group, b)]) for a, b in SV.cols(k)])
        self.lhs = K.frs([v for rw in self.rows for v in rw.scalars])
        logs = [SV.row_logs(cname, rw, k) for rw in self.rows]
        self.want = np.stack([np.concatenate([K.mul(group, l0), K.mul(group, l1)]) for l0, l1 in logs])
        self.zero = [i for i, (l0, l1) in enumerate(logs) if l0 == 0 and l1 == 0]
        ident = [i for i, rw in enumerate(self.rows) if rw.kind == "identity" and rw.label != "last term alone"]
        assert set(ident) <= set(self.zero) and len(ident) >= (7 if k >= 2 else 1)
        assert not self.want[self.zero].any() and self.want[[i for i in range(n) if i not in self.zero]].any(axis=1).all()
        # the reference's own left_mul (term by term) on every 40th dense row and on all built rows
        dense = [i for i, rw in enumerate(self.rows) if rw.kind == "table"]
        sample = dense[::40] + [i for i, rw in enumerate(self.rows) if rw.kind == "built"] + ident
        out = ref.left_mul(cname, group, len(sample), k, self.lhs.reshape(n, -1)[sample], self.col)
        same(out, self.want[sample], [self.labels[i] for i in sample])
        K.check_oracle(group, [l for pair in logs[::97] for l in pair])
        for key, val in DEFAULTS:
            eng.set_option(key, val)
        with profiled(eng) as prof:
            self.planned = eng.mat_left_mul(group, n, k, self.lhs, self.col)
        assert prof.ran("k_var.lm") and not prof.ran("k_var_multi*") and not prof.ran("k_var_tab*"), prof.names
        same(self.planned, self.want, self.labels)


def case(K, group, k):
    key = (K.cid, group, k)
    if key not in _CASES:
        _CASES[key] = Case(K, group, k)
    return _CASES[key]


def straus_name(tm, w, mo):
    return "k_var_multi%d%s%s.lm" % (8 if tm > 4 else 4, "w5" if w == 5 else "", "x%d" % mo if mo > 1 else "")


def run_shape(cid, cname, group, k, opts, kernels, launches=None):
    """The rows of (curve, group, k) under the forced options: `kernels` in the profile and no one-term lanes, exact
    outputs with and without the profile, the planned call's bytes.  launches = (kernel, count): that many launches."""
    K = ctx(cid, cname)
    eng = K.eng
    C = case(K, group, k)
    n = len(C.rows)
    try:
        for key, val in opts.items():
            eng.set_option(key, val)
        with profiled(eng) as prof:
            got = eng.mat_left_mul(group, n, k, C.lhs, C.col)
            eng.sync()
            counts = {p[0]: p[2] for p in eng.prof_get()}
        for kern in kernels:
            assert prof.ran(kern), (kern, prof.names)
        assert not prof.ran("k_var.lm") and not prof.ran("k_var.plain.lm"), prof.names
        if launches:
            assert counts[launches[0]] == launches[1], (launches, counts)
        same(got, C.want, C.labels)
        assert not got[C.zero].any()
        again = eng.mat_left_mul(group, n, k, C.lhs, C.col)
        assert (again == got).all()
    finally:
        for key, val in DEFAULTS:
            eng.set_option(key, val)
    with profiled(eng) as prof:
        back = eng.mat_left_mul(group, n, k, C.lhs, C.col)
    assert prof.ran("k_var.lm") and not prof.ran("k_var_multi*") and not prof.ran("k_var_tab*"), prof.names
    assert (back == got).all() and (back == C.planned).all()


# ---- 1. the cross of group size, window width and outputs per lane ------------------------------------------------------
@pytest.mark.parametrize("mo", [1, 2, 4])
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("tm", [2, 4, 8])
@pytest.mark.parametrize("k", [8, 9])
@pytest.mark.parametrize("cid,cname,group", CG)
def test_forced_straus_shapes(cid, cname, group, k, tm, w, mo):
    """k = 8: groups of 8, 4 + 4, four pairs; k = 9: 5 + 4, 3 x 3, four pairs and a one-term group"""
    assert k in SV.KS[tm]
    run_shape(cid, cname, group, k, dict(var_tm=tm, var_w=w, var_mo=mo), [straus_name(tm, w, mo)])


# ---- 2. short groups in the 4- and 8-term instances ---------------------------------------------------------------------
@pytest.mark.parametrize("tm,k", [(8, 1), (8, 2), (4, 1), (4, 5)])
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("cid,cname,group", CG)
def test_short_groups(cid, cname, group, tm, k, w):
    """one and two terms in the 8-term instance, one term and 3 + 2 in the 4-term instance, one and four outputs per lane"""
    assert k in SV.KS[tm]
    for mo in (1, 4):
        run_shape(cid, cname, group, k, dict(var_tm=tm, var_w=w, var_mo=mo), [straus_name(tm, w, mo)])


# ---- 3. the two-wave G1 builds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mo", [1, 4])
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("tm", [4, 8])
@pytest.mark.parametrize("cid,cname", CURVES)
def test_two_wave_builds(cid, cname, tm, w, mo):
    """var_w2 = 1: the G1 lanes built for two waves per SIMD (18 KB of LDS for the digits: at 8 terms they live in the
    private frame).  k = 9: 5 + 4 and 3 x 3."""
    run_shape(cid, cname, 1, 9, dict(var_tm=tm, var_w=w, var_mo=mo, var_w2=1), [straus_name(tm, w, mo)])


# ---- 4. several launches over one workspace -----------------------------------------------------------------------------
@pytest.mark.parametrize("mo", [1, 2, 4])
@pytest.mark.parametrize("w", [4, 5])
@pytest.mark.parametrize("tm", [4, 8])
@pytest.mark.parametrize("cid,cname,group", CG)
def test_workspace_chunks(cid, cname, group, tm, w, mo):
    """var_ws_lanes = 64 (the option takes multiples of 64): every kernel instance in launches of one wave over the same
    table workspace, all but the first with g0 > 0, the last one ragged"""
    k = 9
    lanes = SV.lane_count(len(SV.rows(cname, group, k)), k, tm, mo)
    assert lanes % 64 not in (0, 1)
    name = straus_name(tm, w, mo)
    run_shape(cid, cname, group, k, dict(var_tm=tm, var_w=w, var_mo=mo, var_ws_lanes=64), [name],
              launches=(name, (lanes + 63) // 64))


# ---- 5. shared base tables (8-bit windows) ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SV.KS_TAB)
@pytest.mark.parametrize("cid,cname", CURVES)
def test_shared_base_tables(cid, cname, k):
    """var_tab = 1 on com1: k_tab_build over the 2 k bases (the identity and half identities among them at k = 9), then
    k_var_tab8 in groups of 2, 8 and 5 + 4 terms"""
    run_shape(cid, cname, 1, k, dict(var_tab=1), ["k_tab_build.lm", "k_var_tab8.lm"])


@pytest.mark.parametrize("cid,cname", CURVES)
def test_com2_ignores_shared_base_tables(cid, cname):
    """the engine has no G2 caller for the shared tables: var_tab = 1 leaves com2 on what var_tm says"""
    run_shape(cid, cname, 2, 8, dict(var_tab=1, var_tm=8, var_w=4, var_mo=1), [straus_name(8, 4, 1)])


# ---- 6. endo = 0 keeps the plain lanes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname,group", CG)
def test_plain_lanes_whatever_else_is_set(cid, cname, group):
    K = ctx(cid, cname)
    eng = K.eng
    C = case(K, group, 8)
    try:
        for key, val in (("endo", 0), ("var_tm", 8), ("var_w", 5), ("var_mo", 4), ("var_tab", 1)):
            eng.set_option(key, val)
        with profiled(eng) as prof:
            got = eng.mat_left_mul(group, len(C.rows), 8, C.lhs, C.col)
        assert prof.ran("k_var.plain.lm") and not prof.ran("k_var_multi*") and not prof.ran("k_var_tab*"), prof.names
        same(got, C.want, C.labels)
    finally:
        for key, val in DEFAULTS:
            eng.set_option(key, val)

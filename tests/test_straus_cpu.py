"""The rows of tests/strausvec.py on the CPU (no GPU): the proof of presence for every (curve, group, window width, group
size) that tests/test_gpu_straus_edges.py forces, and every built and identity row through the twin's Straus MSM against
the big-integer oracle -- which says that the rows' claims and the expectations the device file compares with are right
before anything runs on a device."""
import numpy as np
import pytest

import scalarvec as S
import strausvec as SV
import wirevec as V
from gsutil import curve, ptr
from test_twin import twin  # noqa: F401  (the module-scoped fixture that builds and loads the twin)

import gs_oracle as O  # noqa: E402  (wirevec put oracle/ on the path)

CG = [(cname, g) for cname in S.CURVES for g in (1, 2)]
SHAPES = [(W, tm) for W in (4, 5) for tm in (2, 4, 8)] + [(8, 8)]


@pytest.mark.parametrize("W,tm", SHAPES)
@pytest.mark.parametrize("cname,group", CG)
def test_rows_hold_their_classes(cname, group, W, tm):
    assert SV.selfcheck(cname, group, W, tm) == SV.CANNOT[cname, group]


def test_bn254_streams_cannot_be_isolated():
    """what CANNOT says, from the search itself: no built magnitude of a stream s > 0 survives decompose on BN254, every
    one does on BLS12-381"""
    for (cname, group), names in SV.CANNOT.items():
        for W in SV.WIDTHS:
            assert SV.built(cname, group, W)[1] == names
        m = S.model(cname)
        for s in range(1, m.NS[group]):
            hit = [mag for mag in (1, 3, 127, 1 << 20, (1 << 40) + 5) if SV.isolate(cname, group, s, mag) is not None]
            assert (len(hit) == 0) == ("stream%d" % s in names), (cname, group, s, hit)


def check_rows_on_twin(lib, cname, group, k, kinds=("built", "identity")):
    """every row of those kinds, both components, as ONE Straus lane of k terms (jac_msm_straus, W = 4): the oracle's
    [log] generator, and the identity exactly where the logarithm is 0.  Returns the labels of the rows that differ."""
    c = curve(cname)
    oc = V.setc(cname)
    gen = oc.g1 if group == 1 else oc.g2
    mul = O.g1_mul if group == 1 else O.g2_mul
    dec = c.g1_dec if group == 1 else c.g2_dec
    hexes = (lambda pt: None if pt is None else ["%x" % pt[0], "%x" % pt[1]]) if group == 1 else (
        lambda pt: None if pt is None else ["%x" % v for v in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])])
    fn = getattr(lib, "twin_g%d_msm_%s" % (group, cname))
    pts, want = {}, {}

    def point(log):
        if log not in pts:
            V.setc(cname)
            pts[log] = mul(log % c.r, gen) if log % c.r else None
        return pts[log]

    bases = [np.concatenate([V.point_limbs(cname, point(col[comp]), group) for col in SV.cols(k)]) for comp in (0, 1)]
    bad = []
    for row in SV.rows(cname, group, k):
        if row.kind not in kinds:
            continue
        kk = np.concatenate([c.fr(v) for v in row.scalars])
        for comp, log in enumerate(SV.row_logs(cname, row, k)):
            out = np.zeros((2 if group == 1 else 4) * c.nq, dtype=np.uint64)
            fn(k, ptr(bases[comp]), ptr(kk), ptr(out))
            if log not in want:
                want[log] = hexes(point(log))
            if dec(out) != want[log] or (log == 0) != (not out.any()):
                bad.append("%s, component %d" % (row.label, comp))
    return bad


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("cname,group", CG)
def test_built_rows_on_the_twin(twin, cname, group, k):  # noqa: F811
    """k = 8: the quads on P, on Q and on both, the pairs and the identity rows in one 8-term lane; k = 2: the pairs and
    (s, s) on (P, -P) in a lane of their own"""
    assert check_rows_on_twin(twin, cname, group, k) == []

"""Witness extraction with the binding key (gs_extract_g1 / gs_extract_g2, include/gs_amd.h) restated on the big-integer
oracle, independently of the HIP code.  The CRS of make_crs is u0 = (p, a p), u1 = t u0, so

    G1 variable  c = (O, X) + r0 u0 + r1 u1   ->   c.1 - a c.0 = X
    Fr variable  c = x W1 + r u0              ->   c.1 - a c.0 = x p      (the image of x, not x)

and the hiding key (u1.1 = t a p - p) fails the key check u1.1 == a u1.0.  These are the formulas the GPU tests rely on.
Also here, without a GPU: the new entry points are declared, exported and bound, and the ctypes layer refuses buffers of
the wrong length before a pointer is handed over."""
import os
import random
import re
import sys

import numpy as np
import pytest

from gsutil import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402

CURVES = ["bls12_381", "bn254"]
NAMES = ["gs_set_extraction_key", "gs_extract_g1_dev", "gs_extract_g2_dev", "gs_extract_g1", "gs_extract_g2"]


def _set(name):
    O.set_curve(O.BLS12_381 if name == "bls12_381" else O.BN254)


def extract1(c, a1):
    return O.g1_add(c[1], O.g1_neg(O.g1_mul(a1, c[0])))


def extract2(d, a2):
    return O.g2_add(d[1], O.g2_neg(O.g2_mul(a2, d[0])))


def key_check(crs, a1, a2):
    """The four equalities gs_set_extraction_key tests, in its order."""
    return [O.g1_mul(a1, crs["u"][0][0]) == crs["u"][0][1], O.g1_mul(a1, crs["u"][1][0]) == crs["u"][1][1],
            O.g2_mul(a2, crs["v"][0][0]) == crs["v"][0][1], O.g2_mul(a2, crs["v"][1][0]) == crs["v"][1][1]]


def hiding(crs):
    """generator.rs:65-77: u1.1 = t a p - p, v1.1 likewise."""
    h = dict(crs)
    h["u"] = [crs["u"][0], (crs["u"][1][0], O.g1_add(crs["u"][1][1], O.g1_neg(crs["g1"])))]
    h["v"] = [crs["v"][0], (crs["v"][1][0], O.g2_add(crs["v"][1][1], O.g2_neg(crs["g2"])))]
    return h


@pytest.mark.parametrize("name", CURVES)
def test_extraction_recovers_what_was_committed(name):
    _set(name)
    rng = random.Random(31 if name == "bls12_381" else 32)
    fr = lambda: rng.randrange(1, O.R)
    a1, a2, t1, t2 = fr(), fr(), fr(), fr()
    crs = O.make_crs(O.C.g1, O.C.g2, a1, a2, t1, t2)
    assert key_check(crs, a1, a2) == [True] * 4
    X = [O.g1_mul(fr(), O.C.g1), None, O.g1_mul(fr(), O.C.g1)]
    Y = [O.g2_mul(fr(), O.C.g2), None]
    R = [[fr(), fr()], [fr(), fr()], [0, 0]]
    S = [[fr(), fr()], [0, fr()]]
    assert [extract1(c, a1) for c in O.batch_commit_g1(X, crs, R)] == X
    assert [extract2(d, a2) for d in O.batch_commit_g2(Y, crs, S)] == Y
    xs, ys = [fr(), 0, 1], [fr(), O.R - 1]
    c1 = O.batch_commit_scalar_b1(xs, crs, [[fr()], [fr()], [0]])
    c2 = O.batch_commit_scalar_b2(ys, crs, [[fr()], [fr()]])
    assert [extract1(c, a1) for c in c1] == [O.g1_mul(x, O.C.g1) for x in xs]
    assert [extract2(d, a2) for d in c2] == [O.g2_mul(y, O.C.g2) for y in ys]
    # the doubling lane of the GPU tests: X = -2 a rho p makes a c.0 = -c.1, and the result is still X
    r0, r1 = fr(), fr()
    rho = (r0 + r1 * t1) % O.R
    Xd = O.g1_mul((-2 * a1 * rho) % O.R, O.C.g1)
    (c,) = O.batch_commit_g1([Xd], crs, [[r0, r1]])
    assert O.g1_mul(a1, c[0]) == O.g1_neg(c[1]) and extract1(c, a1) == Xd
    # a wrong key fails its own group's checks only
    assert key_check(crs, (a1 + 1) % O.R, a2) == [False, False, True, True]
    assert key_check(crs, a1, (a2 + 1) % O.R) == [True, True, False, False]


@pytest.mark.parametrize("name", CURVES)
def test_hiding_crs_fails_the_key_check(name):
    _set(name)
    rng = random.Random(33)
    fr = lambda: rng.randrange(1, O.R)
    a1, a2, t1, t2 = fr(), fr(), fr(), fr()
    h = hiding(O.make_crs(O.C.g1, O.C.g2, a1, a2, t1, t2))
    assert key_check(h, a1, a2) == [True, False, True, False]
    # and the formula opens nothing there: it yields X - r1 p, which the randomness moves anywhere
    X = O.g1_mul(fr(), O.C.g1)
    r0, r1 = fr(), fr()
    (c,) = O.batch_commit_g1([X], h, [[r0, r1]])
    assert extract1(c, a1) == O.g1_add(X, O.g1_neg(O.g1_mul(r1, O.C.g1))) != X


def test_entry_points_declared_exported_and_bound():
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import SYMBOLS

    src = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = gs.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n
        assert n in SYMBOLS


def test_capi_refuses_wrong_lengths_before_the_c_abi():
    """No GPU needed: the length checks run before any pointer is handed over (GsError code 1)."""
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import Engine

    e = object.__new__(Engine)  # sizes only: no context (there is no GPU here)
    e.FQ, e.FR, e.G1, e.G2, e.GT, e.CRS = 48, 32, 96, 192, 576, 2016
    e.COM1, e.COM2 = 192, 384
    e.ctx = None
    z = lambda n: np.zeros(n, dtype=np.uint8)
    assert e._check_extract("t", 1, z(3 * 192), z(3 * 96)) == 3
    assert e._check_extract("t", 2, z(2 * 384), z(2 * 192)) == 2
    for group, coms in ((1, z(191)), (1, z(193)), (2, z(383)), (2, z(2 * 384 + 192))):
        with pytest.raises(gs.GsError) as ei:
            e.extract(group, coms)
        assert ei.value.code == 1 and "coms" in str(ei.value)
    with pytest.raises(gs.GsError) as ei:
        e.extract_dev(1, z(2 * 192), z(96))  # output too short
    assert ei.value.code == 1 and "out" in str(ei.value)
    with pytest.raises(gs.GsError) as ei:
        e.extract_dev(2, z(2 * 384), z(2 * 192 + 1))
    assert ei.value.code == 1
    for bad in (z(63), z(65), z(32)):
        with pytest.raises(gs.GsError) as ei:
            e.set_extraction_key(bad)
        assert ei.value.code == 1 and "key" in str(ei.value)
    with pytest.raises(gs.GsError) as ei:
        e.extract(3, z(192))
    assert ei.value.code == 3

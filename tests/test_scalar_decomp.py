"""Scalar decomposition and digit recoding on the CPU twin (no GPU): the named scalars of tests/scalarvec.py and 20 000
seeded random ones through endo_digits<C, W> (Barrett division by lambda / |x| on BLS12-381, lattice rounding on BN254,
recode_w_limbs at W = 4, 5 and 8 -- the last the windows of k_var_tab8) and recode_w4, and the whole table through the scalar multiplications and the Straus MSM
built on them, against the big-integer oracle.

What a digit stream must satisfy comes from plain integer arithmetic (range, recombination, sum +-k_j eig^j = k mod r);
the comparison with scalarvec's model, digit for digit, says in addition that the classes the table claims (correction
counts, sign patterns, -2^(W-1) digits, carries) are the ones the device code really walks through."""
import ctypes
import random

import numpy as np
import pytest

import scalarvec as S
import wirevec as V
from gsutil import curve, ptr
from test_twin import twin  # noqa: F401  (the module-scoped fixture that builds and loads the twin)

import gs_oracle as O  # noqa: E402  (wirevec put oracle/ on the path)

CURVES = S.CURVES
NRANDOM = 20000

# What the seeded searches of scalarvec reach (DESIGN.md 4.1 quotes these): Barrett correction counts per division
# stage on BLS12-381, sign patterns of the sub-scalars on BN254.  A change of the constants that moves them shows here.
REACHED = {
    "bls12_381": {1: [[0, 1]], 2: [[0, 1], [0], [0]]},
    "bn254": {1: [(0, 0)], 2: [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 1, 1), (0, 1, 0, 1), (0, 1, 1, 1)]},
}


def words(ks):
    """canonical scalars as rows of 8 u32 words"""
    return np.array([[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for k in ks], dtype=np.uint32)


def all_scalars(cname, seed):
    rnd = random.Random(seed)
    r = curve(cname).r
    return S.scalars(cname) + [rnd.randrange(r) for _ in range(NRANDOM)]


def label(cname, i, k):
    return "%s (%s)" % (S.name_of(cname, k) if i < len(S.table(cname)) else "random #%d" % i, hex(k))


@pytest.mark.parametrize("cname", CURVES)
def test_table_holds_its_classes(cname):
    assert S.selfcheck(cname) == REACHED[cname]


@pytest.mark.parametrize("W", [4, 5, 8])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("cname", CURVES)
def test_endo_digit_streams(twin, cname, group, W):  # noqa: F811
    m = S.model(cname)
    ks = all_scalars(cname, 5000 + 10 * group + W)
    NS, NL, ND = m.NS[group], m.NL[group], S.nd_of(m.NL[group], W)
    kw = words(ks)
    flat = np.full(len(ks) * NS * ND + 3, 99, dtype=np.int8)  # three guard digits behind the last stream
    sg = np.full(len(ks) * NS, 7, dtype=np.uint8)
    fn = getattr(twin, "twin_endo_digits_" + cname)
    fn.restype = ctypes.c_int
    assert fn(group, W, len(ks), ptr(kw), ptr(flat), ptr(sg)) == ND
    assert (flat[-3:] == 99).all()
    dg = flat[:-3].reshape(len(ks), NS, ND).astype(np.int64)
    sg = sg.reshape(len(ks), NS)
    half = 1 << (W - 1)
    assert dg.min() >= -half and dg.max() < half
    assert ((dg[:, :, -1] == 0) | (dg[:, :, -1] == 1)).all()
    assert (sg <= 1).all()
    weights = np.array([1 << (W * i) for i in range(ND)], dtype=object)
    mags = dg.astype(object).dot(weights)  # (scalars, streams) Python integers
    for i, k in enumerate(ks):
        d = m.decompose(group, k)
        got = [int(v) for v in mags[i]]
        assert all(0 <= v < 1 << (32 * NL) for v in got), label(cname, i, k)
        assert m.recombine(group, got, [int(s) for s in sg[i]]) == k, label(cname, i, k)
        assert [int(s) for s in sg[i]] == d.signs and got == d.mags, label(cname, i, k)
        want = [S.recode(v, NL, W) for v in d.mags]
        assert dg[i].tolist() == want, label(cname, i, k)


@pytest.mark.parametrize("cname", CURVES)
def test_plain_recode_w4(twin, cname):  # noqa: F811
    m = S.model(cname)
    ks = all_scalars(cname, 5100)
    ND = (m.nbits + 3) // 4 + 1
    flat = np.full(len(ks) * ND + 3, 99, dtype=np.int8)
    fn = getattr(twin, "twin_recode_w4_" + cname)
    fn.restype = ctypes.c_int
    assert fn(len(ks), ptr(words(ks)), ptr(flat)) == ND
    assert (flat[-3:] == 99).all()
    dg = flat[:-3].reshape(len(ks), ND).astype(np.int64)
    assert dg.min() >= -8 and dg.max() < 8 and (dg[:, -1] == 0).all()  # (the spare digit: scalarvec proves it stays 0)
    vals = dg.astype(object).dot(np.array([1 << (4 * i) for i in range(ND)], dtype=object))
    for i, k in enumerate(ks):
        assert int(vals[i]) == k, label(cname, i, k)
        assert dg[i].tolist() == S.plain_digits(k, m.nbits), label(cname, i, k)


def _hex1(pt):
    return None if pt is None else ["%x" % pt[0], "%x" % pt[1]]


def _hex2(pt):
    return None if pt is None else ["%x" % v for v in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])]


@pytest.mark.parametrize("cname", CURVES)
def test_table_scalar_multiplications_against_oracle(twin, cname):  # noqa: F811
    """jac_smul_any (GLV / GLS path of each curve) on every table scalar, both groups, base 3 * generator."""
    c = curve(cname)
    oc = V.setc(cname)
    P1, P2 = O.g1_mul(3, oc.g1), O.g2_mul(3, oc.g2)
    b1, b2 = V.point_limbs(cname, P1, 1), V.point_limbs(cname, P2, 2)
    f1, f2 = getattr(twin, "twin_g1_smul_" + cname), getattr(twin, "twin_g2_smul_" + cname)
    for case in S.table(cname):
        V.setc(cname)
        out = np.zeros(2 * c.nq, dtype=np.uint64)
        f1(ptr(b1), ptr(c.fr(case.k)), ptr(out))
        assert c.g1_dec(out) == _hex1(O.g1_mul(case.k, P1)), case.name
        out = np.zeros(4 * c.nq, dtype=np.uint64)
        f2(ptr(b2), ptr(c.fr(case.k)), ptr(out))
        assert c.g2_dec(out) == _hex2(O.g2_mul(case.k, P2)), case.name


@pytest.mark.parametrize("nt", [2, 5, 8])
@pytest.mark.parametrize("cname", CURVES)
def test_table_straus_msm_against_oracle(twin, cname, nt):  # noqa: F811
    """jac_msm_straus on rows of nt consecutive table scalars (every scalar once per width, at a different term position
    in each), over bases that include a repeated point, a negated one and the identity.  The bases are known multiples
    m_j of the generator: the oracle's [sum k_j m_j] generator is the expectation."""
    c = curve(cname)
    oc = V.setc(cname)
    r = c.r
    ks = S.scalars(cname)
    mult = [2, 3, 3, r - 3, 0, 5, 7, r - 2][:nt]  # repeated, negated, identity
    pts1 = [O.g1_mul(v, oc.g1) for v in mult]
    pts2 = [O.g2_mul(v, oc.g2) for v in mult]
    B1 = np.concatenate([V.point_limbs(cname, p, 1) for p in pts1])
    B2 = np.concatenate([V.point_limbs(cname, p, 2) for p in pts2])
    f1, f2 = getattr(twin, "twin_g1_msm_" + cname), getattr(twin, "twin_g2_msm_" + cname)
    for row in range(0, len(ks), nt):
        sel = [ks[(row + j) % len(ks)] for j in range(nt)]
        kk = np.concatenate([c.fr(k) for k in sel])
        total = sum(k * v for k, v in zip(sel, mult)) % r
        names = [S.name_of(cname, k) for k in sel]
        out = np.zeros(2 * c.nq, dtype=np.uint64)
        f1(nt, ptr(B1), ptr(kk), ptr(out))
        assert c.g1_dec(out) == _hex1(O.g1_mul(total, oc.g1)), names
        out = np.zeros(4 * c.nq, dtype=np.uint64)
        f2(nt, ptr(B2), ptr(kk), ptr(out))
        assert c.g2_dec(out) == _hex2(O.g2_mul(total, oc.g2)), names

"""The rerandomization formulas of gs_rerandomize_batch (include/gs_amd.h) restated with the big-integer oracle's
primitives, independently of the HIP code:

    c'_i   = c_i + sum_a R'_ia U_x,a                 d'_j = d_j + sum_b S'_jb V_y,b
    pi'    = pi + R'^T iota2(B) + (R'^T Gamma) d + (R'^T Gamma S' - T'^T) V_y
    theta' = theta + S'^T iota1(A) + (S'^T Gamma^T) c + T' U_x

Rerandomizing prove(X, Y, R, S, T) with (R', S', T') gives exactly prove(X, Y, R + R', S + S', T + T' + S'^T Gamma^T R),
commitments included, and the verdict is preserved (the C oracle's verifier on the golden statements)."""
import os
import random
import sys

import numpy as np
import pytest

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402
import gs_ref_py as ref  # noqa: E402

CURVES = ["bls12_381", "bn254"]
TYPES = [O.PPE, O.MSMEG1, O.MSMEG2, O.QUAD]


def _set(name):
    O.set_curve(O.BLS12_381 if name == "bls12_381" else O.BN254)


def rerandomize(equ, xc, yc, pi, theta, R1, S1, T1, crs):
    """The four formulas, literally (c, d are the OLD commitments)."""
    ty = equ["type"]
    xg, yg = ty in (O.PPE, O.MSMEG1), ty in (O.PPE, O.MSMEG2)
    ucol = crs["u"] if xg else [crs["u"][0]]
    vcol = crs["v"] if yg else [crs["v"][0]]
    map_a = [O.lin1(a) for a in equ["a"]] if xg else [O.slin1(a, crs) for a in equ["a"]]
    map_b = [O.lin2(b) for b in equ["b"]] if yg else [O.slin2(b, crs) for b in equ["b"]]
    G = equ["gamma"]
    R1t, S1t = O.transpose(R1), O.transpose(S1)
    xc2 = [O.com1_add(c, r) for c, r in zip(xc, O.com1_left_mul(ucol, R1))]
    yc2 = [O.com2_add(d, s) for d, s in zip(yc, O.com2_left_mul(vcol, S1))]
    psi = O.fr_matmul(R1t, G)
    omega = O.fr_matadd(O.fr_matmul(psi, S1), O.fr_matneg(O.transpose(T1)))
    pi2 = [O.com2_add(O.com2_add(O.com2_add(p, a), b), c)
           for p, a, b, c in zip(pi, O.com2_left_mul(map_b, R1t), O.com2_left_mul(yc, psi), O.com2_left_mul(vcol, omega))]
    phi = O.fr_matmul(S1t, O.transpose(G))
    th2 = [O.com1_add(O.com1_add(O.com1_add(t, a), b), c)
           for t, a, b, c in zip(theta, O.com1_left_mul(map_a, S1t), O.com1_left_mul(xc, phi), O.com1_left_mul(ucol, T1))]
    return xc2, yc2, pi2, th2


def combined(R, S, T, R1, S1, T1, gamma):
    """R + R', S + S', T'' = T + T' + S'^T Gamma^T R"""
    cross = O.fr_matmul(O.fr_matmul(O.transpose(S1), O.transpose(gamma)), R)
    return O.fr_matadd(R, R1), O.fr_matadd(S, S1), O.fr_matadd(O.fr_matadd(T, T1), cross)


def _crs(rng):
    k = lambda: rng.randrange(1, O.R)
    return O.make_crs(O.C.g1, O.C.g2, k(), k(), k(), k())


def _random_statement(ty, m, n, rng):
    xg, yg = ty in (O.PPE, O.MSMEG1), ty in (O.PPE, O.MSMEG2)
    fr = lambda: rng.randrange(O.R)
    px = lambda: O.g1_mul(fr(), O.C.g1) if xg else fr()
    py = lambda: O.g2_mul(fr(), O.C.g2) if yg else fr()
    X, Y = [px() for _ in range(m)], [py() for _ in range(n)]
    equ = {"type": ty, "a": [px() for _ in range(n)], "b": [py() for _ in range(m)],
           "gamma": [[fr() for _ in range(n)] for _ in range(m)], "target": None}
    kx, ky = (2 if xg else 1), (2 if yg else 1)
    mat = lambda r, c: [[fr() for _ in range(c)] for _ in range(r)]
    return equ, X, Y, (mat(m, kx), mat(n, ky), mat(ky, kx)), (mat(m, kx), mat(n, ky), mat(ky, kx))


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("shape", [(1, 1), (2, 3)])
def test_rerandomized_equals_fresh_proof(name, ty, shape):
    """rerandomize(prove(R, S, T), R', S', T') == prove(R + R', S + S', T + T' + S'^T Gamma^T R)"""
    _set(name)
    rng = random.Random(1000 * ty + 10 * shape[0] + shape[1] + (7 if name == "bn254" else 0))
    crs = _crs(rng)
    m, n = shape
    equ, X, Y, (R, S, T), (R1, S1, T1) = _random_statement(ty, m, n, rng)
    old = O.commit_and_prove(equ, X, Y, R, S, T, crs)
    got = rerandomize(equ, *old, R1, S1, T1, crs)
    want = O.commit_and_prove(equ, X, Y, *combined(R, S, T, R1, S1, T1, equ["gamma"]), crs)
    assert got[0] == want[0] and got[1] == want[1], "commitments"
    assert got[2] == want[2], "pi"
    assert got[3] == want[3], "theta"
    # zero randomness is the identity
    z = lambda M: [[0] * len(r) for r in M]
    assert rerandomize(equ, *old, z(R1), z(S1), z(T1), crs) == tuple(old)


def _dec_case(c, case):
    """A golden statement in the oracle's representation."""
    ty = case["type"]
    xg, yg = ty in (0, 1), ty in (0, 2)
    fr = lambda s: int(s, 16)
    px = (lambda v: O.dec_g1(v)) if xg else fr
    py = (lambda v: O.dec_g2(v)) if yg else fr
    tgt = {0: O.dec_f12, 1: O.dec_g1, 2: O.dec_g2, 3: fr}[ty](case["target"])
    equ = {"type": ty, "a": [px(v) for v in case["a"]], "b": [py(v) for v in case["b"]],
           "gamma": [[fr(s) for s in row] for row in case["gamma"]], "target": tgt}
    mat = lambda M: [[fr(s) for s in row] for row in M]
    g = c.golden["crs"]
    crs = {"u": [(O.dec_g1(a), O.dec_g1(b)) for a, b in g["u"]], "v": [(O.dec_g2(a), O.dec_g2(b)) for a, b in g["v"]],
           "g1": O.dec_g1(g["g1"]), "g2": O.dec_g2(g["g2"]), "gt": O.dec_f12(g["gt"])}
    return equ, [px(v) for v in case["xvars"]], [py(v) for v in case["yvars"]], mat(case["R"]), mat(case["S"]), \
        mat(case["T"]), crs


def _c_verify(c, case, xc, yc, pi, theta):
    """The C oracle's verifier (oracle/gs_ref.c, the reference's evaluation order) on oracle-form outputs."""
    ty = case["type"]
    xg, yg = ty in (0, 1), ty in (0, 2)
    e1 = lambda p: c.g1(O.enc_g1(p))
    e2 = lambda q: c.g2(O.enc_g2(q))
    cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in xs])
    g = c.golden["crs"]
    crs = cat([c.com1(g["u"][0]), c.com1(g["u"][1]), c.com2(g["v"][0]), c.com2(g["v"][1]), c.g1(g["g1"]), c.g2(g["g2"]),
               c.f12(g["gt"])])
    ex = c.g1 if xg else c.fr_hex
    ey = c.g2 if yg else c.fr_hex
    tgt = {0: c.f12, 1: c.g1, 2: c.g2, 3: c.fr_hex}[ty](case["target"])
    return ref.verify(c.name, ty, case["m"], case["n"], cat([ex(v) for v in case["a"]]), cat([ey(v) for v in case["b"]]),
                      c.fr_mat(case["gamma"]), tgt, cat([cat([e1(a), e1(b)]) for a, b in xc]),
                      cat([cat([e2(a), e2(b)]) for a, b in yc]), cat([cat([e2(a), e2(b)]) for a, b in pi]),
                      cat([cat([e1(a), e1(b)]) for a, b in theta]), crs)


@pytest.mark.parametrize("name", CURVES)
def test_verdict_preserved(name):
    """Every type: the rerandomized golden proof verifies; a corrupted pi is still rejected after rerandomization."""
    c = curve(name)
    _set(name)
    rng = random.Random(99)
    for case in c.golden["cases"][:4]:  # the reference's statements, all four types
        equ, X, Y, R, S, T, crs = _dec_case(c, case)
        old = O.commit_and_prove(equ, X, Y, R, S, T, crs)
        assert _c_verify(c, case, *old) == 1, case["name"]
        kx, ky = len(R[0]), len(S[0])
        mat = lambda r, k: [[rng.randrange(O.R) for _ in range(k)] for _ in range(r)]
        R1, S1, T1 = mat(case["m"], kx), mat(case["n"], ky), mat(ky, kx)
        new = rerandomize(equ, *old, R1, S1, T1, crs)
        assert new[0] != old[0] and new[2] != old[2]
        assert _c_verify(c, case, *new) == 1, case["name"]
        bad_pi = [O.com2_add(old[2][0], (None, O.C.g2))] + list(old[2][1:])
        assert _c_verify(c, case, old[0], old[1], bad_pi, old[3]) == 0, case["name"]
        bad = rerandomize(equ, old[0], old[1], bad_pi, old[3], R1, S1, T1, crs)
        assert _c_verify(c, case, *bad) == 0, case["name"]

"""Proof simulation with the hiding CRS's trapdoor (gs_simulate_*, include/gs_amd.h) restated on the big-integer oracle,
independently of the HIP code: tests/simvec.py holds the formulas, this file holds them against the reference's own
verifier and prover (oracle/gs_oracle.py: O.verify, O.prove, O.batch_commit_*).

  1. O.verify accepts the model's output for RANDOM A, B, Gamma and a RANDOM target: no witness is known to the test.
  2. For a satisfied equation, O.prove under the hiding CRS equals the model at the coordinates of simvec.honest_coordinates,
     every element (perfect zero-knowledge, bit for bit).
  3. The model's commitments are O.batch_commit_* of the zero witness.
  4. mirror.equivocate opens a hiding scalar commitment to another value; on the binding CRS it does not.
  5. The key check's identities hold on the hiding CRS and fail on the binding CRS of the same scalars.

Also here, without a GPU: the five new entry points are declared, exported and bound, and the ctypes layer refuses
buffers of the wrong length before a pointer is handed over."""
import os
import random
import re

import numpy as np
import pytest

import simvec
from gsutil import REPO, curve
from simvec import MSMEG1, MSMEG2, QUAD, O

CURVES = ["bls12_381", "bn254"]
TYPES = [MSMEG1, MSMEG2, QUAD]
SHAPES = [(1, 1), (2, 3)]
NAMES = ["gs_set_simulation_key", "gs_simulate_batch_dev", "gs_simulate_batch", "gs_simulate_statement_dev",
         "gs_simulate_statement"]


def _set(name):
    O.set_curve(O.BLS12_381 if name == "bls12_381" else O.BN254)


def _setup(name, seed):
    _set(name)
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, O.R)
    a1, a2, t1, t2 = fr(), fr(), fr(), fr()
    return rng, fr, (a1, a2, t1, t2), simvec.make_hiding_crs(O.C.g1, O.C.g2, a1, a2, t1, t2)


def _constants(ty, m, n, fr):
    """random a (n), b (m), Gamma in the type's own domains"""
    a = [O.g1_mul(fr(), O.C.g1) for _ in range(n)] if simvec.xg(ty) else [fr() for _ in range(n)]
    b = [O.g2_mul(fr(), O.C.g2) for _ in range(m)] if simvec.yg(ty) else [fr() for _ in range(m)]
    return a, b, [[fr() for _ in range(n)] for _ in range(m)]


def _mats(ty, m, n, fr):
    kx, ky = simvec.kxy(ty)
    mat = lambda p, q: [[fr() for _ in range(q)] for _ in range(p)]
    return mat(m, kx), mat(n, ky), mat(ky, kx)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("name", CURVES)
def test_verifier_accepts_simulated_proofs_of_random_statements(name, ty, shape):
    m, n = shape
    rng, fr, (a1, a2, t1, t2), crs = _setup(name, 100 * ty + m)
    a, b, G = _constants(ty, m, n, fr)
    target = {MSMEG1: lambda: O.g1_mul(fr(), O.C.g1), MSMEG2: lambda: O.g2_mul(fr(), O.C.g2), QUAD: fr}[ty]()
    equ = dict(type=ty, a=a, b=b, gamma=G, target=target)
    Rc, Sc, Tf = _mats(ty, m, n, fr)
    xc, yc, pi, theta = simvec.simulate(equ, crs, t1, t2, Rc, Sc, Tf)
    assert O.verify(equ, xc, yc, pi, theta, crs)
    # 3. the commitments are those of the zero witness with R = Rc, S = Sc
    zx = [None] * m if simvec.xg(ty) else [0] * m
    zy = [None] * n if simvec.yg(ty) else [0] * n
    assert xc == (O.batch_commit_g1 if simvec.xg(ty) else O.batch_commit_scalar_b1)(zx, crs, Rc)
    assert yc == (O.batch_commit_g2 if simvec.yg(ty) else O.batch_commit_scalar_b2)(zy, crs, Sc)
    if shape != (1, 1):
        return
    # and the proof is bound to its statement: another target is rejected (one verification more: the small shape only)
    other = dict(equ, target=(target + 1) % O.R if ty == QUAD else
                 (O.g1_add(target, O.C.g1) if ty == MSMEG1 else O.g2_add(target, O.C.g2)))
    assert not O.verify(other, xc, yc, pi, theta, crs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("name", CURVES)
def test_honest_proof_equals_simulated_proof(name, ty, shape):
    m, n = shape
    rng, fr, (a1, a2, t1, t2), crs = _setup(name, 200 * ty + n)
    a, b, G = _constants(ty, m, n, fr)
    xs, ys = [fr() for _ in range(m)], [fr() for _ in range(n)]  # X_i = xs_i g1 on a group-valued side
    X = [O.g1_mul(x, O.C.g1) for x in xs] if simvec.xg(ty) else xs
    Y = [O.g2_mul(y, O.C.g2) for y in ys] if simvec.yg(ty) else ys
    r = O.R
    gsum = sum(xs[i] * G[i][j] * ys[j] for i in range(m) for j in range(n))
    if ty == MSMEG1:  # sum_j y_j A_j + sum_i b_i X_i + sum_ij Gamma_ij y_j X_i
        target = O.g1_mul((sum(b[i] * xs[i] for i in range(m)) + gsum) % r, O.C.g1)
        for j in range(n):
            target = O.g1_add(target, O.g1_mul(ys[j], a[j]))
    elif ty == MSMEG2:
        target = O.g2_mul((sum(a[j] * ys[j] for j in range(n)) + gsum) % r, O.C.g2)
        for i in range(m):
            target = O.g2_add(target, O.g2_mul(xs[i], b[i]))
    else:
        target = (sum(a[j] * ys[j] for j in range(n)) + sum(xs[i] * b[i] for i in range(m)) + gsum) % r
    equ = dict(type=ty, a=a, b=b, gamma=G, target=target)
    R, S, T = _mats(ty, m, n, fr)
    hxc, hyc, hpi, hth = O.commit_and_prove(equ, X, Y, R, S, T, crs)
    Rc, Sc, Tf = simvec.honest_coordinates(ty, r, t1, t2, a, b, G, xs, ys, R, S, T)
    xc, yc, pi, theta = simvec.simulate(equ, crs, t1, t2, Rc, Sc, Tf)
    assert xc == hxc and yc == hyc
    assert pi == hpi
    assert theta == hth


@pytest.mark.parametrize("name", CURVES)
def test_equivocation_opens_a_hiding_scalar_commitment_to_another_value(name):
    from groth_sahai_rs_amd import mirror

    rng, fr, (a1, a2, t1, t2), hid = _setup(name, 77)
    bind = O.make_crs(O.C.g1, O.C.g2, a1, a2, t1, t2)
    c = curve(name)
    for group, t in ((1, t1), (2, t2)):
        commit = O.batch_commit_scalar_b1 if group == 1 else O.batch_commit_scalar_b2
        for x, x_new in ((fr(), fr()), (fr(), 0), (0, O.R - 1)):
            rr = fr()
            r_new = c.fr_dec(mirror.equivocate(c.fr(x), c.fr(rr), c.fr(x_new), c.fr(t), curve=c.curve_id))
            assert r_new == (rr + (x - x_new) * t) % O.R
            assert commit([x_new], hid, [[r_new]]) == commit([x], hid, [[rr]])
            assert commit([x_new], bind, [[r_new]]) != commit([x], bind, [[rr]])


@pytest.mark.parametrize("name", CURVES)
def test_key_identities_hold_on_the_hiding_crs_only(name):
    rng, fr, (a1, a2, t1, t2), hid = _setup(name, 78)
    bind = O.make_crs(O.C.g1, O.C.g2, a1, a2, t1, t2)
    assert simvec.key_identities(hid, t1, t2) == [True] * 4
    # the binding CRS of the same scalars: W.0 = t key0.0 still holds, W.1 is off by the generator
    assert simvec.key_identities(bind, t1, t2) == [True, False, True, False]
    assert simvec.key_identities(hid, (t1 + 1) % O.R, t2) == [False, False, True, True]
    assert simvec.key_identities(hid, t1, (t2 + 1) % O.R) == [True, True, False, False]


def test_simulating_a_ppe_is_refused_by_the_model():
    with pytest.raises(ValueError):
        simvec.coefficients(simvec.PPE, 7, 1, 1, [], [], [[1]], None, [[1, 1]], [[1, 1]], [[1, 1], [1, 1]])


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
    N, m, n = 2, 2, 3
    good = dict(A=z(N * n * 96), B=z(N * m * 32), Gamma=z(N * m * n * 32), target=z(N * 96), Rc=z(N * m * 2 * 32),
                Sc=z(N * n * 32), Tf=z(N * 2 * 32))
    for k in good:
        for delta in (-1, 32):
            bad = dict(good)
            bad[k] = z(good[k].size + delta)
            with pytest.raises(gs.GsError) as ei:
                e.simulate_batch(gs.GS_MSMEG1, N, m, n, **bad)
            assert ei.value.code == 1, k
    # a Statement takes ONE copy of Rc, Sc: the batch's sizes are refused
    with pytest.raises(gs.GsError) as ei:
        e.simulate_statement(gs.GS_MSMEG1, N, m, n, **good)
    assert ei.value.code == 1
    outs = dict(xcoms=z(N * m * 192), ycoms=z(N * n * 384), pi=z(N * 2 * 384), theta=z(N * 192))
    for k in outs:
        bad = dict(outs)
        bad[k] = z(outs[k].size - 1)
        with pytest.raises(gs.GsError) as ei:
            e.simulate_batch_dev(gs.GS_MSMEG1, N, m, n, *good.values(), **bad)
        assert ei.value.code == 1, k
    with pytest.raises(gs.GsError) as ei:
        e.simulate_batch_dev(gs.GS_MSMEG1, N, m, n, *good.values(), None, None, None, outs["theta"])
    assert ei.value.code == 3
    for bad in (z(63), z(65), z(32)):
        with pytest.raises(gs.GsError) as ei:
            e.set_simulation_key(bad)
        assert ei.value.code == 1 and "key" in str(ei.value)

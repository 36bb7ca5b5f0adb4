"""gs_eval_* / gs_check_witness_* without a GPU: the symbols, the binding's size checks, and the algebra of the plan.

The device path never evaluates an equation term by term (include/gs_amd.h).  It folds the Gamma term:
    PPE      W_j = A_j + sum_i Gamma_ij X_i,           value = prod_j e(W_j, Y_j) prod_i e(X_i, B_i)
    MSMEG1   c_i = b_i + sum_j Gamma_ij y_j,           value = sum_j y_j A_j + sum_i c_i X_i
    MSMEG2   d_j = a_j + sum_i x_i Gamma_ij,           value = sum_i x_i B_i + sum_j d_j Y_j
    QuadEqu  the same c_i,                             value = sum_j a_j y_j + sum_i x_i c_i
Here the folded forms are held against the term-by-term left-hand sides of src/statement.rs:17-21 with the big-integer
oracle (oracle/gs_oracle.py), in pure Python, on BN254 at (m, n) = (2, 3): unequal, so that a transposed Gamma shows."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from gsutil import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402

NAMES = ["gs_eval_batch_dev", "gs_eval_batch", "gs_eval_statement_dev", "gs_eval_statement",
         "gs_check_witness_batch_dev", "gs_check_witness_batch", "gs_check_witness_statement_dev",
         "gs_check_witness_statement"]


def test_library_exports_the_eight_entries():
    from groth_sahai_rs_amd.capi import SYMBOLS, lib_path

    lib = ctypes.CDLL(lib_path())
    for nm in NAMES:
        assert nm in SYMBOLS, nm
        assert hasattr(lib, nm), nm
    header = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    for nm in NAMES:
        assert "int %s(gs_ctx*" % nm in header, nm


def _engine():
    from groth_sahai_rs_amd.capi import Engine

    e = object.__new__(Engine)  # sizes only: no context (there is no GPU here); BLS12-381
    e.FQ, e.FR, e.G1, e.G2, e.GT, e.CRS = 48, 32, 96, 192, 576, 2016
    e.COM1, e.COM2 = 192, 384
    return e


def test_binding_refuses_short_buffers_before_the_abi():
    """Every array of the eight entries is sized from (type, N, m, n, statement or not) before a pointer crosses the ABI:
    a wrong length is GS_ERR_SHAPE, a missing array GS_ERR_ARG.  The fake engine has no context and no library: a call
    that got past the checks would raise AttributeError, not GsError."""
    import groth_sahai_rs_amd as gs

    e = _engine()
    z = lambda k: np.zeros(k, dtype=np.uint8)
    N, m, n = 3, 2, 1
    for ty, sx, sy, st in ((0, 96, 192, 576), (1, 96, 32, 96), (2, 32, 192, 192), (3, 32, 32, 32)):
        for stmt in (False, True):
            V = 1 if stmt else N
            good = dict(X=z(V * m * sx), Y=z(V * n * sy), A=z(N * n * sx), B=z(N * m * sy), Gamma=z(N * m * n * 32))
            ev = "gs_eval_statement" if stmt else "gs_eval_batch"
            ck = "gs_check_witness_statement" if stmt else "gs_check_witness_batch"
            for name in good:
                bad = dict(good)
                bad[name] = z(good[name].size - 32)
                with pytest.raises(gs.GsError) as ei:
                    e._eval(ev, ty, N, m, n, **bad)
                assert ei.value.code == 1 and name in str(ei.value), (ty, stmt, name)
            # a statement's X is ONE copy: the batch-sized array is refused, and the other way round
            other = dict(good, X=z((N if stmt else 1) * m * sx))
            with pytest.raises(gs.GsError) as ei:
                e._eval(ev, ty, N, m, n, **other)
            assert ei.value.code == 1 and "X" in str(ei.value)
            for out, code in ((z(N * st - 1), 1), (z(N * st + st), 1)):
                with pytest.raises(gs.GsError) as ei:
                    e._eval(ev, ty, N, m, n, out=out, **good)
                assert ei.value.code == code and "target_out" in str(ei.value)
            with pytest.raises(gs.GsError) as ei:
                e._eval(ck, ty, N, m, n, target=z(N * st - 1), out=z(N), **good)
            assert ei.value.code == 1 and "target" in str(ei.value)
            with pytest.raises(gs.GsError) as ei:
                e._eval(ck, ty, N, m, n, target=z(N * st), out=z(N - 1), **good)
            assert ei.value.code == 1 and "ok" in str(ei.value)
            with pytest.raises(gs.GsError) as ei:
                e._eval(ck, ty, N, m, n, target=None, out=z(N), **good)
            assert ei.value.code == 3
            with pytest.raises(gs.GsError) as ei:  # a _dev form allocates nothing
                e._eval(ev + "_dev", ty, N, m, n, out=None, **good)
            assert ei.value.code == 3
            with pytest.raises(gs.GsError):
                e._eval(ev, ty, N, 0, n, **good)  # empty variable list
            with pytest.raises(gs.GsError):
                e._eval(ev, 7, N, m, n, **good)  # unknown type


# ---- the algebra ----------------------------------------------------------------------------------------------------
M, N_ = 2, 3


def _statement(ty, rng):
    xg, yg = ty in (O.PPE, O.MSMEG1), ty in (O.PPE, O.MSMEG2)
    fr = lambda: rng.randrange(1, O.R)
    px = lambda: O.g1_mul(fr(), O.C.g1) if xg else fr()
    py = lambda: O.g2_mul(fr(), O.C.g2) if yg else fr()
    return dict(X=[px() for _ in range(M)], Y=[py() for _ in range(N_)], a=[px() for _ in range(N_)],
                b=[py() for _ in range(M)], G=[[fr() for _ in range(N_)] for _ in range(M)])


@pytest.fixture(scope="module")
def bn254():
    O.set_curve(O.BN254)
    yield
    O.set_curve(O.BLS12_381)


def _sum(add, terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = add(acc, t)
    return acc


def test_ppe_fold_equals_the_term_by_term_product(bn254):
    s = _statement(O.PPE, random.Random(0xE7A1))
    X, Y, a, b, G = (s[k] for k in ("X", "Y", "a", "b", "G"))
    # statement.rs:17: prod_j e(a_j, Y_j) prod_i e(X_i, b_i) prod_ij e(X_i, Y_j)^gamma_ij, one pairing per term
    terms = [O.pairing(a[j], Y[j]) for j in range(N_)] + [O.pairing(X[i], b[i]) for i in range(M)]
    terms += [O.f12_pow(O.pairing(X[i], Y[j]), G[i][j]) for i in range(M) for j in range(N_)]
    want = _sum(O.f12_mul, terms)
    W = [_sum(O.g1_add, [a[j]] + [O.g1_mul(G[i][j], X[i]) for i in range(M)]) for j in range(N_)]
    got = O.multi_pairing(W + X, Y + b)  # m + n pairs
    assert O.f12_flat(got) == O.f12_flat(want)
    # the transposed fold is a different value: the shape (2, 3) cannot hide it
    Wt = [_sum(O.g1_add, [a[j]] + [O.g1_mul(G[i][(j + 1) % N_], X[i]) for i in range(M)]) for j in range(N_)]
    assert O.f12_flat(O.multi_pairing(Wt + X, Y + b)) != O.f12_flat(want)


def test_msmeg1_fold_equals_the_term_by_term_sum(bn254):
    s = _statement(O.MSMEG1, random.Random(0xE7A2))
    X, y, a, b, G = (s[k] for k in ("X", "Y", "a", "b", "G"))
    terms = [O.g1_mul(y[j], a[j]) for j in range(N_)] + [O.g1_mul(b[i], X[i]) for i in range(M)]
    terms += [O.g1_mul(G[i][j] * y[j] % O.R, X[i]) for i in range(M) for j in range(N_)]
    want = _sum(O.g1_add, terms)
    c = [(b[i] + sum(G[i][j] * y[j] for j in range(N_))) % O.R for i in range(M)]
    got = _sum(O.g1_add, [O.g1_mul(y[j], a[j]) for j in range(N_)] + [O.g1_mul(c[i], X[i]) for i in range(M)])
    assert got == want


def test_msmeg2_fold_equals_the_term_by_term_sum(bn254):
    s = _statement(O.MSMEG2, random.Random(0xE7A3))
    x, Y, a, b, G = (s[k] for k in ("X", "Y", "a", "b", "G"))
    terms = [O.g2_mul(a[j], Y[j]) for j in range(N_)] + [O.g2_mul(x[i], b[i]) for i in range(M)]
    terms += [O.g2_mul(G[i][j] * x[i] % O.R, Y[j]) for i in range(M) for j in range(N_)]
    want = _sum(O.g2_add, terms)
    d = [(a[j] + sum(x[i] * G[i][j] for i in range(M))) % O.R for j in range(N_)]
    got = _sum(O.g2_add, [O.g2_mul(x[i], b[i]) for i in range(M)] + [O.g2_mul(d[j], Y[j]) for j in range(N_)])
    assert got == want


def test_quad_fold_equals_the_term_by_term_sum(bn254):
    s = _statement(O.QUAD, random.Random(0xE7A4))
    x, y, a, b, G = (s[k] for k in ("X", "Y", "a", "b", "G"))
    want = (sum(a[j] * y[j] for j in range(N_)) + sum(x[i] * b[i] for i in range(M)) +
            sum(x[i] * G[i][j] * y[j] for i in range(M) for j in range(N_))) % O.R
    c = [(b[i] + sum(G[i][j] * y[j] for j in range(N_))) % O.R for i in range(M)]
    assert (sum(a[j] * y[j] for j in range(N_)) + sum(x[i] * c[i] for i in range(M))) % O.R == want

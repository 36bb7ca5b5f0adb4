"""Fault localisation of the batched verifier, without a GPU: the descent model (tests/locatevec.py) against brute force
on a toy group, and the presence of the feature at every layer (header, library, ctypes binding)."""
import os
import random
import re

import pytest

import locatevec
from gsutil import REPO

P = (1 << 61) - 1  # a Mersenne prime: the toy group is (Z/P)*, written multiplicatively
G = 3
mul = lambda a, b: a * b % P
eq = lambda a, b: a == b


def toy_pairs(N, bad, rng):
    """(W, T) per leaf: W = g^0 on a good leaf, g^random (never one) on a bad one; T = one."""
    out = []
    for e in range(N):
        w = 1
        if e in bad:
            while w == 1:
                w = pow(G, rng.randrange(1, P - 1), P)
        out.append((w, 1))
    return out


@pytest.mark.parametrize("K", [2, 4, 8])
def test_model_reports_exactly_the_bad_set(K):
    rng = random.Random(1000 + K)
    for N in range(1, 71):
        sets = [set(), {rng.randrange(N)}, set(range(N)), {N - 1}, {0}]
        sets += [set(rng.sample(range(N), rng.randrange(0, N + 1))) for _ in range(3)]
        for bad in sets:
            pairs = toy_pairs(N, bad, rng)
            ok, n_bad, n_checks = locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K)
            assert [e for e in range(N) if ok[e] == 0] == sorted(bad), (N, K, bad)
            assert n_bad == len(bad)
            assert n_checks == locatevec.checks_formula(bad, N, K), (N, K, bad)
            # brute force: a leaf is reported iff it fails on its own (random exponents do not cancel)
            assert ok == [0 if w != t else 1 for w, t in pairs]


@pytest.mark.parametrize("K", [2, 4, 8])
def test_model_counts_on_the_extremes(K):
    for N in (1, 2, K, K + 1, K * K, K * K + 1, 65):
        sizes = locatevec.level_sizes(N, K)
        good = locatevec.descend(lambda level, index: True, N, K)
        assert good == ([1] * N, 0, 1)
        ok, n_bad, n_checks = locatevec.descend(lambda level, index: False, N, K)
        assert ok == [0] * N and n_bad == N
        assert n_checks == sum(sizes)  # every node of the tree once


@pytest.mark.parametrize("K", [2, 4, 8])
def test_cancelling_pair_inside_one_group_is_not_seen(K):
    rng = random.Random(7)
    N = 70
    z = pow(G, rng.randrange(2, P - 1), P)
    zi = pow(z, P - 2, P)
    # both in the leaf group [K, 2K): the group's node passes, so does everything above it
    pairs = toy_pairs(N, set(), rng)
    pairs[K], pairs[K + 1] = (z, 1), (zi, 1)
    assert locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K) == ([1] * N, 0, 1)
    # with a third, independent fault elsewhere the pair stays hidden and the third is found
    pairs[N - 3] = (pow(G, 12345, P), 1)
    ok, n_bad, _ = locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K)
    assert [e for e in range(N) if not ok[e]] == [N - 3] and n_bad == 1
    # split across two children of the ROOT (63 | 64 for every K here) with a third fault that makes the root fail: no
    # node on either path holds both halves, so both are reached and fail
    assert all(K ** (len(locatevec.level_sizes(N, K)) - 2) == 64 for K in (2, 4, 8))
    pairs = toy_pairs(N, set(), rng)
    pairs[63], pairs[64] = (z, 1), (zi, 1)
    pairs[N - 3] = (pow(G, 12345, P), 1)
    ok, n_bad, _ = locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K)
    assert [e for e in range(N) if not ok[e]] == [63, 64, N - 3] and n_bad == 3
    # split, and nothing else wrong: the root passes and nobody looks
    pairs[N - 3] = (1, 1)
    assert locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K) == ([1] * N, 0, 1)
    # split across two LEAF groups (K - 1 | K) only: the node two levels up holds both halves and passes, so the pair
    # stays hidden there too -- "found when split" needs the split to reach up to a failing node
    pairs = toy_pairs(N, set(), rng)
    pairs[K - 1], pairs[K] = (z, 1), (zi, 1)
    pairs[N - 3] = (pow(G, 12345, P), 1)
    ok, n_bad, _ = locatevec.descend(locatevec.from_pairs(pairs, K, mul, eq), N, K)
    assert [e for e in range(N) if not ok[e]] == [N - 3] and n_bad == 1


# ---- the feature is there, at every layer ------------------------------------------------------------------------------
NAMES = ["gs_verify_batch_rlc_locate_dev", "gs_verify_batch_rlc_locate"]


def test_header_declares_the_entry_points():
    src = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert '"locate_k"' in src


def test_library_exports_the_entry_points():
    import groth_sahai_rs_amd as gs

    lib = gs.load_library()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name


def test_engine_has_both_methods():
    from groth_sahai_rs_amd.capi import Engine

    assert callable(getattr(Engine, "verify_batch_rlc_locate", None))
    assert callable(getattr(Engine, "verify_batch_rlc_locate_dev", None))

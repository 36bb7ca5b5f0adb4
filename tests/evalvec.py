"""Inputs and expectations of tests/test_gpu_eval.py: dense equations with targets from discrete logarithms
(sparsevec.make_equation: the points come from the C oracle, the target from the logarithms, never from the engine), and
the left-hand sides of src/statement.rs:17-21 computed ONE TERM AT A TIME with the C oracle's exported primitives
(ref_g1_mul, ref_g1_add, ref_g2_mul, ref_g2_add, ref_multi_pairing, ref_gt_mul), the way the reference's own tests write
them (tests/prover.rs:50-52): no folding of the Gamma term anywhere."""
import random

import numpy as np

import sparsevec as sv
from forge import u8, xg, yg
from sparsevec import ref

KEYS = ("X", "Y", "A", "B", "G", "target")
_DENSE = {}


def dense(cname, ty, m, n, count, seed):
    """`count` dense equations of one shape: dict of the concatenated arrays X, Y, A, B, G, target (+ crs, eqs).
    Computed once per argument list and shared; callers leave it unchanged."""
    key = (cname, ty, m, n, count, seed)
    if key not in _DENSE:
        from gpubatch import pool

        binding, _ = sv.crs(cname)
        rng = random.Random(seed)
        seeds = [rng.getrandbits(64) for _ in range(count)]
        eqs = list(pool().map(lambda e: sv.make_equation(cname, ty, m, n, sv.PATTERNS[0], random.Random(seeds[e])),
                              range(count)))
        b = dict(cname=cname, ty=ty, m=m, n=n, N=count, crs=binding, eqs=eqs)
        b.update({k: np.concatenate([q[k] for q in eqs]) for k in KEYS})
        _DENSE[key] = b
    return _DENSE[key]


def term_by_term(cname, ty, m, n, eq):
    """The value of one equation (arrays X, Y, A, B, G of ONE equation) as target bytes, one term at a time."""
    _, cx = sv.crs(cname)
    sx, sy = (cx.G1 if xg(ty) else cx.FR), (cx.G2 if yg(ty) else cx.FR)
    cut = lambda a, sz: [u8(a[i * sz:(i + 1) * sz]) for i in range(a.size // sz)]
    X, A, Y, B, G = cut(eq["X"], sx), cut(eq["A"], sx), cut(eq["Y"], sy), cut(eq["B"], sy), cut(eq["G"], cx.FR)
    assert (len(X), len(Y), len(A), len(B), len(G)) == (m, n, n, m, m * n)
    if ty == 3:
        x, y, a, b, g = (cx.fr_ints(np.concatenate(v)) for v in (X, Y, A, B, G))
        t = sum(a[j] * y[j] for j in range(n)) + sum(x[i] * b[i] for i in range(m))
        t += sum(x[i] * g[i * n + j] * y[j] for i in range(m) for j in range(n))
        return cx.fr(t % cx.r)
    if ty == 0:
        pair = lambda p, q: ref.multi_pairing(cname, 1, p, q)
        terms = [pair(A[j], Y[j]) for j in range(n)] + [pair(X[i], B[i]) for i in range(m)]
        terms += [pair(ref.g_mul(cname, 1, X[i], G[i * n + j]), Y[j]) for i in range(m) for j in range(n)]
        acc = terms[0]
        for t in terms[1:]:
            acc = ref.gt_mul(cname, acc, t)
        return u8(acc)
    group = 1 if ty == 1 else 2
    mul = lambda p, k: ref.g_mul(cname, group, p, k)
    if ty == 1:  # sum_j y_j A_j + sum_i b_i X_i + sum_ij gamma_ij y_j X_i
        terms = [mul(A[j], Y[j]) for j in range(n)] + [mul(X[i], B[i]) for i in range(m)]
        terms += [mul(mul(X[i], G[i * n + j]), Y[j]) for i in range(m) for j in range(n)]
    else:  # sum_j a_j Y_j + sum_i x_i B_i + sum_ij gamma_ij x_i Y_j
        terms = [mul(Y[j], A[j]) for j in range(n)] + [mul(B[i], X[i]) for i in range(m)]
        terms += [mul(mul(Y[j], G[i * n + j]), X[i]) for i in range(m) for j in range(n)]
    acc = terms[0]
    for t in terms[1:]:
        acc = ref.g_add(cname, group, acc, t)
    return u8(acc)

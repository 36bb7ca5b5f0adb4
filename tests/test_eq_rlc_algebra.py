"""The folding behind gs_verify_equation_rlc, pinned on the C oracle without a GPU: for N proofs of ONE
equation the random linear combination sum_e sum_ab rho_e,ab (lhs_e - rhs_e)_ab, taken ACROSS the proofs wherever the
other argument of a pair is a constant or a CRS element, is a multi-pairing with 2n pairs per proof (2n + 2kx with the
pi term kept per proof) and a number of batch-level pairs that does not depend on N.

The inputs are arbitrary subgroup elements, not proofs, so the combined value is not one: an identity that only held on
valid proofs would not pass.  rho rows carry the edge values of the 64-bit exponents and the mixed row (the rows of
test_gpu_stmt_rlc.py)."""
import random

import numpy as np
import pytest

import eqrlc
import forge
from forge import ref

EDGE_RHO = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
MIXED_ROW = [(1 << 64) - 1, 1, 1 << 32, (1 << 63) + 5]
CASES = [(ty, N, m, n) for ty in (0, 1, 2, 3) for N in (1, 2, 3) for m, n in ((1, 1), (2, 3))]


def arbitrary_batch(cname, ty, N, m, n, seed):
    c = forge.curve(cname)
    crs = forge.golden_crs(c)
    cx = forge.Ctx(cname, crs)
    rng = random.Random(seed)
    xg, yg, kx, ky = eqrlc.shape(ty)
    pts = lambda group, cnt: np.concatenate([cx.mul(group, cx.gen(group), rng.randrange(1, cx.r)) for _ in range(cnt)])
    frs = lambda cnt: np.concatenate([cx.fr(rng.randrange(0, cx.r)) for _ in range(cnt)])
    if ty == 0:
        target = ref.gt_pow(cname, cx.gt, cx.fr(rng.randrange(1, cx.r)))
    else:
        target = pts(1, 1) if ty == 1 else pts(2, 1) if ty == 2 else frs(1)
    const = dict(A=pts(1, n) if xg else frs(n), B=pts(2, m) if yg else frs(m), G=frs(m * n), target=target)
    proofs = [dict(xcoms=pts(1, 2 * m), ycoms=pts(2, 2 * n), pi=pts(2, kx * 2), theta=pts(1, ky * 2)) for _ in range(N)]
    return crs, const, proofs


def edge_rho(N, seed):
    rng = random.Random(seed)
    rho = [[rng.randrange(1, 1 << 64) for _ in range(4)] for _ in range(N)]
    rho[0] = list(MIXED_ROW)
    if N > 1:
        rho[-1] = [EDGE_RHO[(seed + k) % len(EDGE_RHO)] for k in (0, 3, 4, 5)]
    if N > 2:
        rho[1] = [EDGE_RHO[-1]] * 4  # with the mixed row: sums beyond 2^64
    return rho


@pytest.mark.parametrize("ty,N,m,n", CASES)
def test_folded_multi_pairing_equals_the_literal_combination(ty, N, m, n):
    cname = "bn254"
    crs, const, proofs = arbitrary_batch(cname, ty, N, m, n, 300 + 10 * ty + N)
    rho = edge_rho(N, 5 + ty + N)
    W, T, oks = eqrlc.literal(cname, ty, m, n, const, proofs, rho, crs)
    assert not any(oks)  # arbitrary elements: no proof holds
    assert (W != eqrlc.gt_one(cname)).any()
    if ty == 0:  # the one target power of the batch is the product of the per-proof powers
        c = forge.curve(cname)
        r11 = eqrlc.sum_rho(rho)[3]
        assert (ref.gt_pow(cname, forge.u8(const["target"]), forge.u8(c.fr(r11 % c.r))) == T).all()
    for fold_pi in (False, True):
        per_proof, per_batch = eqrlc.folded_pairs(cname, ty, m, n, const, proofs, rho, crs, fold_pi)
        want_pp, want_pb = eqrlc.pair_counts(ty, m, n, fold_pi)
        assert len(per_proof) == N * want_pp and len(per_batch) == want_pb
        F = eqrlc.folded_value(cname, per_proof + per_batch)
        assert (F == W).all(), ("folded multi-pairing != prod (lhs / rhs')^rho", fold_pi)


def test_the_pair_counts_of_a_4_by_4_PPE():
    """8 N + 12 pairs against the 20 N of gs_verify_batch_rlc, with pi folded"""
    pp, pb = eqrlc.pair_counts(0, 4, 4, True)
    assert (pp, pb) == (8, 12)
    assert eqrlc.pair_counts(0, 4, 4, False) == (12, 8)


def test_sum_of_rho_is_carried_exactly():
    """2^16 rows of 2^64 - 1: the halves' sums stay below 2^64 and the assembled value is the integer sum (the 128-bit
    reduction's contract: k_prep_verify_eq_rlc adds the 32-bit halves of every exponent in 64-bit counters)"""
    N, v = 1 << 16, (1 << 64) - 1
    rs = eqrlc.sum_rho([[v, 1, v - 1, 1 << 63]] * N)
    assert rs == [N * v, N, N * (v - 1), N << 63]
    assert rs[0] >= 1 << 79 and rs[0] < 1 << 80
    # the device's own order of operations, in 64-bit words: w0 = lo + (hi << 32) mod 2^64, w1 = (hi >> 32) + carry
    M = (1 << 64) - 1
    lo, hi = N * (v & 0xFFFFFFFF), N * (v >> 32)
    w0 = (lo + ((hi << 32) & M)) & M
    w1 = (hi >> 32) + (1 if w0 < lo else 0)
    assert w0 + (w1 << 64) == N * v

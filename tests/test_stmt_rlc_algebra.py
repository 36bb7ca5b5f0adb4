"""The folding behind gs_verify_statements_rlc, pinned on the C oracle without a GPU: for a statement of
E equations over shared commitments the random linear combination sum_e sum_ab rho_e,ab (lhs_e - rhs_e)_ab, taken
ACROSS the equations before pairing, is a multi-pairing whose pair count does not depend on E.

The inputs are arbitrary group elements, not proofs, so the combined value is not one: an identity that only held on
satisfied equations would not pass.  rho rows carry the edge values of the 64-bit exponents and the mixed row."""
import random

import numpy as np
import pytest

import forge
import stmtrlc
from forge import ref

EDGE_RHO = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
MIXED_ROW = [(1 << 64) - 1, 1, 1 << 32, (1 << 63) + 5]
# the four types at E = 2, 1 x 1, and a PPE 2 x 1 at E = 3
CASES = [(0, 2, 1, 1), (1, 2, 1, 1), (2, 2, 1, 1), (3, 2, 1, 1), (0, 3, 2, 1)]


def arbitrary_statement(cname, ty, E, m, n, seed):
    c = forge.curve(cname)
    crs = forge.golden_crs(c)
    cx = forge.Ctx(cname, crs)
    rng = random.Random(seed)
    xg, yg, kx, ky = stmtrlc.shape(ty)
    pts = lambda group, cnt: np.concatenate([cx.mul(group, cx.gen(group), rng.randrange(1, cx.r)) for _ in range(cnt)])
    frs = lambda cnt: np.concatenate([cx.fr(rng.randrange(0, cx.r)) for _ in range(cnt)])
    if ty == 0:
        target = np.concatenate([ref.gt_pow(cname, cx.gt, cx.fr(rng.randrange(1, cx.r))) for _ in range(E)])
    else:
        target = pts(1, E) if ty == 1 else pts(2, E) if ty == 2 else frs(E)
    st = dict(A=pts(1, E * n) if xg else frs(E * n), B=pts(2, E * m) if yg else frs(E * m), G=frs(E * m * n),
              target=target, xcoms=pts(1, 2 * m), ycoms=pts(2, 2 * n), pi=pts(2, E * kx * 2), theta=pts(1, E * ky * 2))
    return crs, st


def edge_rho(E, seed):
    rng = random.Random(seed)
    rho = [[rng.randrange(1, 1 << 64) for _ in range(4)] for _ in range(E)]
    rho[0] = list(MIXED_ROW)
    rho[-1] = [EDGE_RHO[(seed + k) % len(EDGE_RHO)] for k in (0, 3, 4, 5)]
    return rho


@pytest.mark.parametrize("ty,E,m,n", CASES)
def test_folded_multi_pairing_equals_the_literal_combination(ty, E, m, n):
    cname = "bn254"
    crs, st = arbitrary_statement(cname, ty, E, m, n, 77 + ty)
    rho = edge_rho(E, 5 + ty)
    W, T, L, oks = stmtrlc.literal(cname, ty, m, n, E, st, rho, crs)
    assert not any(oks)  # arbitrary elements: no equation holds, no cell is trivially one
    assert (L != stmtrlc.gt_one(cname)).any()
    pairs = stmtrlc.folded_pairs(cname, ty, m, n, E, st, rho, crs)
    xg, yg, kx, ky = stmtrlc.shape(ty)
    # the pair count of the issue, 2n + 2m + 2kx + 2ky, for every type at these shapes -- plus, for MSMEG2 alone, the
    # two pairs of its G2 targets against W1.a (item 5 of the folding: -W1.a is the partner of no other pair)
    assert len(pairs) == 2 * n + 2 * m + 2 * kx + 2 * ky + (2 if ty == 2 else 0)
    assert len(pairs) == stmtrlc.pair_count(ty, m, n)
    F = stmtrlc.folded_value(cname, pairs)
    assert (F == W).all(), "folded multi-pairing != prod (lhs / rhs')^rho"
    # with the PPE targets on the other side of the comparison: F / T = prod (lhs / rhs)^rho
    assert (ref.gt_mul(cname, F, ref.gt_inv(cname, T)) == L).all()


def test_pair_count_does_not_depend_on_E():
    cname = "bn254"
    counts = set()
    for E in (1, 4):
        crs, st = arbitrary_statement(cname, 0, E, 1, 1, 9)
        counts.add(len(stmtrlc.folded_pairs(cname, 0, 1, 1, E, st, edge_rho(E, 1), crs)))
    assert counts == {stmtrlc.pair_count(0, 1, 1)} == {12}

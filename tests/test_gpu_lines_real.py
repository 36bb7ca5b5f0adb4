"""Real-form Miller lines on the device (csrc/gs_pairing.cuh `Line`: lines scaled to a real y coefficient, the sparse
products f12_mul_by_014r / _034r, line tables divided by ly, the lane-pair exchange of five Fq) against the C oracle.

  * gs_multi_pairing_batch (the single-accumulator loop, stepped lines): 130 products -- two full waves and a partial
    one -- of k = 1 and k = 3 pairs, identity arguments in some pairs, bit-exact with oracle/gs_ref.c.
  * verify at N = 66 with the Miller form forced to the twin lane, the lane pair over LDS and the lane pair over DPP, for
    1 x 1 and 2 x 3 statements (odd numbers of stepping triples: the partial round's select path), PPE and QuadEqu, both
    curves, CRS line tables on and off, one corrupted proof per batch: proofs bit-exact and verdicts as the oracle's
    (tests/gpubatch.py)."""
import os
import sys

import numpy as np
import pytest

from gpubatch import pool, run_batch
from gsutil import REPO, curve

pytestmark = pytest.mark.gpu

MILLER_KERNEL = {1: "k_miller.twin", 2: "k_miller.pair", 3: "k_miller.pairdpp"}


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cname,cid", [("bls12_381", 0), ("bn254", 1)])
def test_multi_pairing_batch_bit_exact(cname, cid, k):
    import groth_sahai_rs_amd as gs

    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gs_ref_py as ref

    c = curve(cname)
    e = gs.Engine(cid, 0)
    try:
        n = 130
        rng = np.random.default_rng(4100 + k)
        rs = lambda cnt: np.stack([c.fr(int.from_bytes(rng.bytes(40), "little") % c.r) for _ in range(cnt)])
        g1, g2 = c.g1(c.golden["g1_smul"][0]["out"]), c.g2(c.golden["g2_smul"][0]["out"])
        P = e.g_mul_batch(1, g1, rs(n * k), broadcast=True).reshape(n, k, -1).copy()
        Q = e.g_mul_batch(2, g2, rs(n * k), broadcast=True).reshape(n, k, -1).copy()
        # identities: G1 in products 3 and 64 (first pair), G2 in 65 and 129 (last pair), both in 7: with k = 1 the whole
        # product is 1, with k = 3 the pair is skipped
        P[3, 0] = 0
        P[64, 0] = 0
        Q[65, k - 1] = 0
        Q[129, k - 1] = 0
        P[7, 0] = 0
        Q[7, 0] = 0
        out = e.multi_pairing_batch(n, k, P.reshape(-1), Q.reshape(-1))
        want = list(pool().map(lambda i: ref.multi_pairing(cname, k, P[i].reshape(-1), Q[i].reshape(-1)), range(n)))
        bad = [i for i in range(n) if not (out[i].view(np.uint8).reshape(-1) == want[i]).all()]
        assert not bad, bad[:8]
        if k == 1:
            one = c.f12(["1"] + ["0"] * 11).view(np.uint8)
            assert (out[3].view(np.uint8).reshape(-1) == one).all()
    finally:
        e.close()


@pytest.mark.parametrize("tables", [1, 0])
@pytest.mark.parametrize("twin", [1, 2, 3])
@pytest.mark.parametrize("m,n", [(1, 1), (2, 3)])
@pytest.mark.parametrize("ty", [0, 3])
@pytest.mark.parametrize("cname,cid", [("bls12_381", 0), ("bn254", 1)])
def test_verify_forced_miller_forms(cname, cid, ty, m, n, twin, tables):
    N = 66  # two waves per task in the twin form (the second ragged), three in the lane-pair forms
    o = dict(miller_twin=twin, line_tables=tables)
    run_batch(cid, cname, ty, N, m, n, (0, 33, 65), opts=o, expect=[MILLER_KERNEL[twin]], seed=9400 + 10 * ty + m,
              corrupt_every=N, rlc=False)

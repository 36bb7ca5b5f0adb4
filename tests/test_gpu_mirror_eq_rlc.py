"""mirror.verify_equation_rlc (groth_sahai_rs_amd/mirror.py) on the GPU: N showings of one equation -- a proof and its
rerandomizations -- pass ONE combined check, and a batch with one forged showing is rejected.  rho is drawn from the
caller's generator when none is given (the low limb of rng.fr(), or rng.u64() when it has one)."""
import copy

import numpy as np
import pytest

from test_gpu_mirror_stmt_rlc import Rng, ZeroFirstRng, equation, setup  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("idx", [4, 5, 6, 7])  # the dense 2 x 2 golden statement of every type
def test_showings_of_one_equation(setup, idx):
    c, mirror, crs = setup
    equ, xvars, yvars = equation(c, mirror, c.golden["cases"][idx])
    rng = Rng(21 + idx)
    first = equ.commit_and_prove(xvars, yvars, crs, rng)
    shown = [first] + [mirror.rerandomize(equ, first, crs, rng) for _ in range(4)]
    assert all(equ.verify(cp, crs) for cp in shown)
    draws = Rng(5)
    assert mirror.verify_equation_rlc(equ, shown, crs, draws) is True
    assert draws.draws == 4 * len(shown)  # one exponent per cell of every proof
    assert mirror.verify_equation_rlc(equ, shown, crs, ZeroFirstRng(6)) is True
    assert mirror.verify_equation_rlc(equ, shown[2:3], crs, Rng(7)) is True
    rho = np.arange(1, 4 * len(shown) + 1, dtype=np.uint64)  # given exponents: no draw
    assert mirror.verify_equation_rlc(equ, shown, crs, rho=rho) is True
    # one forged showing: a commitment-shaped value of the right length in place of a theta
    bad = copy.deepcopy(shown)
    bad[3].equ_proofs[0].theta[0] = shown[3].xcoms.coms[0]
    assert equ.verify(bad[3], crs) is False
    assert mirror.verify_equation_rlc(equ, bad, crs, Rng(8)) is False
    # the equation moved after the proofs were made
    forged = copy.deepcopy(equ)
    forged.gamma[0][0] = c.fr(12345)
    assert mirror.verify_equation_rlc(forged, shown, crs, Rng(9)) is False
    with pytest.raises(AssertionError):  # lengths from the wire are checked before the C ABI, as in verify()
        p3 = copy.deepcopy(shown)
        p3[1].equ_proofs[0].pi = p3[1].equ_proofs[0].pi[:-1]
        mirror.verify_equation_rlc(equ, p3, crs, Rng(10))

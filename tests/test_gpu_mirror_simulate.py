"""mirror.generate_crs_with_trapdoor, <Equation>.simulate, Statement.simulate and mirror.equivocate
(groth_sahai_rs_amd/mirror.py) on the GPU: under the hiding CRS the trapdoor answers the golden equations of the three
simulated types WITHOUT their witnesses -- also after their targets were moved, when no witness the test knows satisfies
them -- and opens a scalar commitment to another value."""
import copy

import numpy as np
import pytest

from gsutil import curve
from test_gpu_mirror_stmt_rlc import Rng, equation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hiding():
    from groth_sahai_rs_amd import mirror

    c = curve("bls12_381")
    g = c.golden["crs"]
    crs, trapdoor = mirror.generate_crs_with_trapdoor(c.g1(g["g1"]), c.g2(g["g2"]), Rng(401))
    return c, mirror, crs, trapdoor


def moved(c, equ):
    """the same constants with another target of the type's kind"""
    other = copy.deepcopy(equ)
    g = c.golden["crs"]
    other.target = {1: lambda: c.g1(g["g1"]), 2: lambda: c.g2(g["g2"]), 3: lambda: c.fr(424242)}[equ.TYPE]()
    assert not (np.asarray(other.target) == np.asarray(equ.target)).all()
    return other


def test_trapdoor_crs_is_the_hiding_crs_of_the_same_draws(hiding):
    c, mirror, crs, trapdoor = hiding
    g = c.golden["crs"]
    plain = mirror.generate_crs(c.g1(g["g1"]), c.g2(g["g2"]), Rng(401), hiding=True)
    bind = mirror.generate_crs(c.g1(g["g1"]), c.g2(g["g2"]), Rng(401))
    for a, b in zip(plain.u + plain.v, crs.u + crs.v):
        assert (a == b).all()
    assert (bind.u[0] == crs.u[0]).all() and not (bind.u[1] == crs.u[1]).all()
    assert trapdoor.shape == (8,) and trapdoor.dtype == np.uint64
    bind.engine.close()
    plain.engine.close()


@pytest.mark.parametrize("idx", [5, 6, 7])  # the dense 2 x 2 golden statement of MSMEG1, MSMEG2, QuadEqu
def test_simulated_proofs_verify_without_a_witness(hiding, idx):
    c, mirror, crs, trapdoor = hiding
    equ, _, _ = equation(c, mirror, c.golden["cases"][idx])
    other = moved(c, equ)
    rng = Rng(30 + idx)
    cp = equ.simulate(crs, trapdoor, rng)
    kx, ky = equ._kxky()
    assert rng.draws == 2 * kx + 2 * ky + kx * ky  # Rc, Sc, Tf
    assert len(cp.xcoms.coms) == 2 and len(cp.ycoms.coms) == 2 and len(cp.equ_proofs) == 1
    assert equ.verify(cp, crs) is True
    cq = other.simulate(crs, trapdoor, rng)
    assert other.verify(cq, crs) is True
    assert other.verify(cp, crs) is False and equ.verify(cq, crs) is False  # each proof is bound to its statement
    assert equ.verify(mirror.rerandomize(equ, cp, crs, rng), crs) is True
    # a statement of three equations over ONE simulated commitment set
    st = mirror.Statement([equ, other, copy.deepcopy(equ)])
    sp = st.simulate(crs, trapdoor, Rng(60 + idx))
    assert st.verify(sp, crs) == [True] * 3
    assert mirror.Statement([other, equ, equ]).verify(sp, crs) == [False, False, True]


def test_refusals(hiding):
    import groth_sahai_rs_amd as gs

    c, mirror, crs, trapdoor = hiding
    ppe, _, _ = equation(c, mirror, c.golden["cases"][4])
    with pytest.raises(gs.GsError) as ei:
        ppe.simulate(crs, trapdoor, Rng(1))
    assert ei.value.code == 3 and "PPE" in str(ei.value)
    quad, _, _ = equation(c, mirror, c.golden["cases"][7])
    with pytest.raises(gs.GsError) as ei:  # a wrong trapdoor
        quad.simulate(crs, trapdoor[::-1].copy(), Rng(2))
    assert ei.value.code == 3
    g = c.golden["crs"]
    bind = mirror.generate_crs(c.g1(g["g1"]), c.g2(g["g2"]), Rng(401))
    with pytest.raises(gs.GsError) as ei:  # the binding CRS of the same draws has no trapdoor
        quad.simulate(bind, trapdoor, Rng(3))
    assert ei.value.code == 3 and "binding" in str(ei.value)
    bind.engine.close()
    crs.engine.set_simulation_key(None)
    with pytest.raises(gs.GsError):
        crs.engine.simulate_batch(3, 1, 2, 2, *(np.zeros(k * 32, np.uint8) for k in (2, 2, 4, 1, 2, 2, 1)))


def test_equivocation_on_the_device(hiding):
    c, mirror, crs, trapdoor = hiding
    rng = Rng(77)
    for kind, t in (("fr_b1", trapdoor[:4]), ("fr_b2", trapdoor[4:])):
        x, r, x_new = rng.fr(), rng.fr(), rng.fr()
        r_new = mirror.equivocate(x, r, x_new, t)
        assert (crs.engine.commit(kind, x, r) == crs.engine.commit(kind, x_new, r_new)).all()
        assert not (crs.engine.commit(kind, x_new, r) == crs.engine.commit(kind, x, r)).all()

"""mirror.Statement.verify_rlc and mirror.MixedStatement.verify_rlc (groth_sahai_rs_amd/mirror.py) on the GPU: the combined
check accepts what verify() accepts on every equation and rejects a statement with one forged equation.  rho is drawn
from the caller's generator (the low limb of rng.fr(), or rng.u64() when it has one)."""
import copy

import numpy as np
import pytest

from gsutil import curve

pytestmark = pytest.mark.gpu


class Rng:
    def __init__(self, seed):
        self.r = np.random.default_rng(seed)
        self.draws = 0

    def fr(self):
        v = self.r.integers(0, 1 << 62, size=4, dtype=np.uint64)
        v[3] &= np.uint64((1 << 60) - 1)  # < r as a Montgomery representative
        self.draws += 1
        return v


class ZeroFirstRng(Rng):
    """a generator whose first 64-bit draw is zero: it must be drawn again, never used"""

    def u64(self):
        self.draws += 1
        return 0 if self.draws == 1 else int(self.r.integers(1, 1 << 63))


@pytest.fixture(scope="module")
def setup():
    from groth_sahai_rs_amd import mirror

    c = curve("bls12_381")
    g = c.golden["crs"]
    crs = mirror.CRS([c.com1(g["u"][0]), c.com1(g["u"][1])], [c.com2(g["v"][0]), c.com2(g["v"][1])], c.g1(g["g1"]),
                     c.g2(g["g2"]), c.f12(g["gt"]))
    return c, mirror, crs


def equation(c, mirror, k):
    ty = k["type"]
    ex = c.g1 if ty in (0, 1) else c.fr_hex
    ey = c.g2 if ty in (0, 2) else c.fr_hex
    cls = [mirror.PPE, mirror.MSMEG1, mirror.MSMEG2, mirror.QuadEqu][ty]
    tgt = {0: c.f12, 1: c.g1, 2: c.g2, 3: c.fr_hex}[ty](k["target"])
    return cls([ex(v) for v in k["a"]], [ey(v) for v in k["b"]], [[c.fr_hex(s) for s in row] for row in k["gamma"]], tgt), \
        [ex(v) for v in k["xvars"]], [ey(v) for v in k["yvars"]]


@pytest.mark.parametrize("idx", [4, 5, 6, 7])  # the dense 2 x 2 golden statement of every type
def test_statement_verify_rlc(setup, idx):
    c, mirror, crs = setup
    equ, xvars, yvars = equation(c, mirror, c.golden["cases"][idx])
    st = mirror.Statement([equ, copy.deepcopy(equ), copy.deepcopy(equ)])
    proof = st.commit_and_prove(xvars, yvars, crs, Rng(11 + idx))
    assert st.verify(proof, crs) == [True] * 3
    rng = Rng(5)
    assert st.verify_rlc(proof, crs, rng) is True
    assert rng.draws == 4 * 3  # one exponent per cell of every equation
    assert st.verify_rlc(proof, crs, ZeroFirstRng(6)) is True
    # one forged equation: the middle equation's Gamma moved after the proof was made
    forged = copy.deepcopy(equ)
    forged.gamma[0][0] = c.fr(12345)
    bad = mirror.Statement([equ, forged, equ])
    assert bad.verify(proof, crs) == [True, False, True]
    assert bad.verify_rlc(proof, crs, Rng(7)) is False
    # the proof of one equation replaced by a commitment-shaped value of the right length
    p2 = copy.deepcopy(proof)
    p2.equ_proofs[2].theta[0] = proof.xcoms.coms[0]
    assert st.verify(p2, crs) == [True, True, False]
    assert st.verify_rlc(p2, crs, Rng(8)) is False
    with pytest.raises(AssertionError):  # lengths from the wire are checked before the C ABI, as in verify()
        p3 = copy.deepcopy(proof)
        p3.equ_proofs[0].pi = p3.equ_proofs[0].pi[:-1]
        st.verify_rlc(p3, crs, Rng(9))


def mixed_statement(mirror):
    """Two SATISFIED equations of each of the four types over one list of variables (tests/stmtutil.py), as mirror
    objects under the CRS the inputs were made for: (crs, equations, xg, yg, xs, ys)"""
    import groth_sahai_rs_amd as gs
    from stmtutil import StatementInputs

    mg, ng, ms, ns = 2, 3, 2, 1
    eng = gs.Engine(0, 0)
    try:
        st = StatementInputs(eng, mg=mg, ng=ng, ms=ms, ns=ns, seed=8300)
        parts = [st.part(ty, 2) for ty in range(4)]
        words = lambda a, cnt: [x.copy() for x in np.ascontiguousarray(a).view(np.uint8).reshape(cnt, -1).view(np.uint64)]
        raw = np.ascontiguousarray(st.crs).view(np.uint8).reshape(-1)
        o, pieces = 0, []
        for sz in (eng.COM1, eng.COM1, eng.COM2, eng.COM2, eng.G1, eng.G2, eng.GT):
            pieces.append(raw[o:o + sz].view(np.uint64).copy())
            o += sz
        xg, yg = words(st.vars["xg"], mg), words(st.vars["yg"], ng)
        xs, ys = words(st.vars["xs"], ms), words(st.vars["ys"], ns)
    finally:
        eng.close()
    crs = mirror.CRS(pieces[:2], pieces[2:4], pieces[4], pieces[5], pieces[6])
    cls = [mirror.PPE, mirror.MSMEG1, mirror.MSMEG2, mirror.QuadEqu]
    equs = []
    for e in range(2):  # the types interleaved
        for p in parts:
            m, n = p["m"], p["n"]
            a, b, g, t = words(p["A"], 2 * n), words(p["B"], 2 * m), words(p["Gamma"], 2 * m * n), words(p["target"], 2)
            gam = [[g[(e * m + i) * n + j] for j in range(n)] for i in range(m)]
            equs.append(cls[p["ty"]](a[e * n:(e + 1) * n], b[e * m:(e + 1) * m], gam, t[e]))
    return crs, equs, xg, yg, xs, ys


def test_mixed_statement_verify_rlc():
    from groth_sahai_rs_amd import mirror

    crs, equs, xg, yg, xs, ys = mixed_statement(mirror)
    assert [e.TYPE for e in equs] == [0, 1, 2, 3, 0, 1, 2, 3]  # all four types, two equations each
    st = mirror.MixedStatement(equs)
    proof = st.commit_and_prove(xg, yg, xs, ys, crs, Rng(2))
    assert st.verify(proof, crs) == [True] * len(equs)
    rng = Rng(3)
    assert st.verify_rlc(proof, crs, rng) is True
    assert rng.draws == 4 * len(equs)
    # type by type: the pi of the type's two proofs exchanged -- both equations fail, the combined check rejects
    for ty in range(4):
        bad = copy.deepcopy(proof)
        bad.equ_proofs[ty].pi, bad.equ_proofs[4 + ty].pi = proof.equ_proofs[4 + ty].pi, proof.equ_proofs[ty].pi
        assert st.verify(bad, crs) == [i not in (ty, 4 + ty) for i in range(len(equs))]
        assert st.verify_rlc(bad, crs, Rng(4 + ty)) is False
    # one forged QuadEqu target: only a scalar of the statement is wrong, the verdict of the whole statement is false
    forged = list(equs)
    forged[7] = copy.deepcopy(equs[7])
    forged[7].target = curve("bls12_381").fr(424242)
    fs = mirror.MixedStatement(forged)
    assert fs.verify(proof, crs) == [i != 7 for i in range(len(equs))]
    assert fs.verify_rlc(proof, crs, Rng(9)) is False

"""The forged-proof builder (tests/forge.py) against the oracles, without a GPU: the variants are what they claim to be
(well-formed, different from the original, accepted or rejected by the reference's verification equation as intended,
wrong in exactly one ComT cell where they say so), so that tests/test_gpu_soundness.py can hold the GPU verifiers to the
oracle's verdict on them.

Kept as a regression test of the builder: in the golden case ppe_ragged_3x1 the row of Gamma and the B entry of the
third x variable are zero, the equation does not look at xcoms[2], and the REFERENCE accepts every forgery of it.  The
rule for a verifier is therefore "its verdict equals the oracle's on every variant", never "every forgery is
rejected"."""
import multiprocessing
import os
import random
from concurrent.futures import ProcessPoolExecutor

import pytest

import forge
from gpubatch import pool
from gsutil import curve

CURVES = ["bls12_381", "bn254"]
CELLS = [(0, 0), (0, 1), (1, 0), (1, 1)]
TRAP = (0x1234567890ABCDEF1122334455667788, 0x0FEDCBA987654321AABBCCDDEEFF0011, 0x5DEECE66D5DEECE66D, 0x2545F4914F6CDD1D2545F491)


def _variants(cname, case, seed):
    """All variants of one golden case: everything under the golden CRS, the trapdoor kinds under a binding and a hiding
    CRS of the test's own over the same generators.  -> list of (eq, variant)"""
    c = curve(cname)
    rng = random.Random(seed)
    eq = forge.golden_eq(cname, case)
    out = [(eq, v) for v in forge.build(eq, rng, other=forge.other_of(eq, rng))]
    g = c.golden["crs"]
    for hiding, crs in zip((False, True), forge.crs_pair(cname, c.g1(g["g1"]), c.g2(g["g2"]), *TRAP)):
        eq2 = forge.golden_eq(cname, case, crs=crs, rng=rng)
        assert forge.oracle_verdict(eq2, eq2) == 1, (case["name"], "honest proof under the test's CRS", hiding)
        out += [(eq2, v) for v in forge.build(eq2, rng, trap=TRAP, hiding=hiding)
                if v["kind"] in ("cell", "accepted_bindcancel")]
    assert forge.oracle_verdict(eq, eq) == 1, case["name"]
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_variants_are_what_they_claim(cname):
    c = curve(cname)
    kinds = {k: 0 for k in forge.KINDS}
    share = {}  # type -> [rejected, all] over the variants not named "accepted"
    for ci, case in enumerate(c.golden["cases"]):
        vs = _variants(cname, case, 100 + ci)
        res = list(pool().map(lambda ev: forge.oracle_cells(*ev), vs))
        print("%s %s: %d variants" % (cname, case["name"], len(vs)))
        dense = "ragged" not in case["name"]
        for (eq, v), (ok, lhs, rhs, _) in zip(vs, res):
            where = (cname, case["name"], v["name"])
            kinds[v["kind"]] += 1
            assert not forge.same_bytes(eq, v), where
            assert forge.on_curve(cname, eq["ty"], v), where
            assert ok == int((lhs == rhs).all()), where
            if v["accepted"]:
                assert ok == 1, where
                continue
            sh = share.setdefault(eq["ty"], [0, 0])
            sh[0] += ok == 0
            sh[1] += 1
            if dense:
                assert ok == 0, where
            elif v["name"].startswith("xcoms[2]"):
                assert ok == 1, where  # the slot the ragged equation does not look at
            else:
                assert ok == 0, where
            if v["kind"] == "cell":
                bad = [CELLS[i] for i in range(4) if (lhs[i] != rhs[i]).any()]
                assert bad == [v["cell"]], (where, bad)
    print(cname, "variants per kind:", kinds)
    assert all(kinds.values()), kinds
    for ty, (rej, tot) in sorted(share.items()):
        print("%s type %d: %d of %d forged variants rejected by the oracle" % (cname, ty, rej, tot))
        assert rej >= 0.9 * tot, (cname, ty, rej, tot)


def test_single_cell_kinds_cover_the_cells():
    """PPE: every cell is isolated, through pi and through theta.  MSMEG1: all four through pi; MSMEG2: all four through
    theta; QuadEqu: none (forge.py's header gives the reason)."""
    c = curve("bn254")
    want = {forge.PPE: 2, forge.MSMEG1: 1, forge.MSMEG2: 1, forge.QUAD: 0}
    for case in c.golden["cases"][:4]:
        cells = [v["cell"] for _, v in _variants("bn254", case, 7) if v["kind"] == "cell"]
        assert sorted(cells) == sorted(CELLS * want[case["type"]]), (case["name"], cells)


def _bigint(job):
    return forge.bigint_verdict(*job)


@pytest.mark.slow
@pytest.mark.parametrize("cname", CURVES)
def test_c_oracle_and_bigint_oracle_agree(cname):
    """One variant of every kind on the 2x1 golden case of each type: oracle/gs_ref.c and gs_oracle.verify give the same
    verdict.  (Not more: a big-integer verify of a 2x1 equation takes seconds.)"""
    c = curve(cname)
    jobs, want, names = [], [], []
    for ci, case in enumerate(c.golden["cases"][:4]):
        assert (case["m"], case["n"]) == (2, 1)
        seen = set()
        for eq, v in _variants(cname, case, 200 + ci):
            if v["kind"] in seen:
                continue
            seen.add(v["kind"])
            jobs.append((cname, eq["ty"], eq["m"], eq["n"], {k: v[k] for k in forge.INPUTS}, eq["crs"]))
            want.append(forge.oracle_verdict(eq, v))
            names.append((case["name"], v["name"]))
    with ProcessPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)),
                             mp_context=multiprocessing.get_context("fork")) as ex:
        got = list(ex.map(_bigint, jobs))
    bad = [(nm, w, g) for nm, w, g in zip(names, want, got) if w != g]
    assert not bad, bad
    assert 0 in want and 1 in want

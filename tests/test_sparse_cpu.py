"""Sparse and degenerate statements on the CPU (no GPU): the proof of presence of tests/sparsevec.py for all eight
(curve, type) pairs, and the branches of the twin and lane-pair Miller loops and of the final exponentiation that only
an identity reaches, through the host compile of the device headers (tests/twin/host_twin.cpp).

What is covered here.  Every triple (Q, P0, P1) of a Miller task takes a state out of
    full | P0 dead | P1 dead | both P dead | Q dead          (dead = the identity)
and twin_multi_pairing_two_<curve> runs multi_miller2 (mode 1) or multi_miller_pair on two host threads (mode 2) on
DISTINCT component arrays, with live / qok formed as the device kernels form them; both accumulators, after the final
exponentiation, are compared with gs_ref_py.multi_pairing over the triples live for that component (GT one for none).
  * np = 2 (even nstep) and np = 3 (odd nstep: the last round has one line), all stepping: EXHAUSTIVE, 25 + 125 state
    vectors, both curves, both modes.  In the pair mode the two triples of a round then meet in every pair of states:
    the two-product branch next to the select branch (own_ok && par_ok on one lane only), both lanes selecting with
    opposite selections, a dead Q stepped from (0, 0, 1) whose line still crosses the exchange.
  * np = 4, two stepping and two reading line tables: 25 vectors in which every pair of states occurs on the stepping
    round and every state at both table positions (`Q dead` included: the device tabulates CRS points only, the loop
    must still never consume the table of a dead Q); the stepping triples sit in front of or behind the tabulated ones
    in the caller's order.
  * all-dead runs for np = 2, 3 (inside the exhaustive sets: every triple `Q dead`, every triple `both P dead`) and 4.
The whole file takes 44 s on eight cores, so the np = 3 set is NOT thinned."""
import itertools

import numpy as np
import pytest

import sparsevec as sv
from gsutil import curve, ptr
from test_twin import CURVES, twin  # noqa: F401  (the fixture that builds and loads the host twin)

import gs_ref_py as ref  # noqa: E402  (sparsevec has put oracle/ on the path)

STATES = ("full", "p0_dead", "p1_dead", "both_p_dead", "q_dead")
TYPES = (0, 1, 2, 3)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname", CURVES)
def test_selfcheck(cname, ty):
    """The named batch holds what it claims, by the C oracle; the claims a type cannot hold are the pinned ones."""
    assert sv.selfcheck(cname, ty) == sorted(sv.CANNOT[ty])


def test_batch_layout():
    assert sv.P == 36 and sv.N == 72 and len(set(nm for nm, _, _, _ in sv.PATTERNS)) == sv.P
    assert sv.FALSE_TWINS == ("false_everything_identity", "false_RST_zero", "false_cancel_x")


# ---- Miller loops on triples with dead members --------------------------------------------------------------------
_PTS = {}


def _points(cname):
    """8 distinct (P0, P1, Q): multiples of the golden generators, by the oracle"""
    if cname not in _PTS:
        c = curve(cname)
        fr = lambda v: sv.u8(c.fr(v))
        g1, g2 = sv.u8(c.g1(c.golden["g1_smul"][0]["out"])), sv.u8(c.g2(c.golden["g2_smul"][0]["out"]))
        _PTS[cname] = [(ref.g_mul(cname, 1, g1, fr(3 + 7 * k)), ref.g_mul(cname, 1, g1, fr(1000003 + 11 * k)),
                        ref.g_mul(cname, 2, g2, fr(5 + 13 * k))) for k in range(8)]
    return _PTS[cname]


def _run_case(twin, cname, states, mask, modes=(1, 2)):  # noqa: F811
    c = curve(cname)
    pts = _points(cname)
    FQ, FR, G1, G2, GT, CRS = ref.sizes(cname)
    z1, z2 = np.zeros(G1, np.uint8), np.zeros(G2, np.uint8)
    p0 = [z1 if s in ("p0_dead", "both_p_dead") else pts[k][0] for k, s in enumerate(states)]
    p1 = [z1 if s in ("p1_dead", "both_p_dead") else pts[k][1] for k, s in enumerate(states)]
    q = [z2 if s == "q_dead" else pts[k][2] for k, s in enumerate(states)]
    one = np.zeros(GT, np.uint8)
    one[:FQ] = sv.u8(c.fq(1))
    want = []
    for comp in (p0, p1):
        live = [k for k in range(len(states)) if comp[k].any() and q[k].any()]
        want.append(ref.multi_pairing(cname, len(live), np.concatenate([comp[k] for k in live]),
                                      np.concatenate([q[k] for k in live])) if live else one)
    P0, P1, Q = np.concatenate(p0), np.concatenate(p1), np.concatenate(q)
    f = getattr(twin, "twin_multi_pairing_two_" + cname)
    for mode in modes:
        out = np.zeros(2 * GT, np.uint8)
        f(len(states), ptr(P0), ptr(P1), ptr(Q), mask, ptr(out), mode)
        for a in (0, 1):
            assert (out[a * GT:(a + 1) * GT] == want[a]).all(), (cname, "pair" if mode == 2 else "twin", states, mask,
                                                                 "accumulator %d" % a)


@pytest.mark.parametrize("cname", CURVES)
@pytest.mark.parametrize("np_", [2, 3])
def test_stepping_triples_every_state_vector(twin, cname, np_):  # noqa: F811
    """np = 2 (one full round) and np = 3 (a full round and the one-line round of an odd count), every vector of states."""
    for states in itertools.product(STATES, repeat=np_):
        _run_case(twin, cname, states, 0)


def np4_cases():
    """(states in the caller's order, mask): the two stepping triples take every pair of states; the two tabulated ones
    every state at both table positions; stepping triples first (mask 0b1100) or last (0b0011)."""
    out = []
    for i, (s0, s1) in enumerate(itertools.product(STATES, repeat=2)):
        t0, t1 = STATES[i % 5], STATES[(i // 5 + i) % 5]
        out.append(((s0, s1, t0, t1), 0b1100) if i % 2 == 0 else ((t0, t1, s0, s1), 0b0011))
    return out


def test_np4_cover():
    cases = np4_cases()
    step = {(c[0][:2] if c[1] == 0b1100 else c[0][2:]) for c in cases}
    assert step == set(itertools.product(STATES, repeat=2))
    for pos in (0, 1):
        assert {(c[0][2 + pos] if c[1] == 0b1100 else c[0][pos]) for c in cases} == set(STATES)


@pytest.mark.parametrize("cname", CURVES)
def test_two_stepping_two_tabulated_triples(twin, cname):  # noqa: F811
    for states, mask in np4_cases():
        _run_case(twin, cname, states, mask)
    for states, mask in ((("both_p_dead",) * 4, 0b1100), (("q_dead", "q_dead", "both_p_dead", "both_p_dead"), 0b1100)):
        _run_case(twin, cname, states, mask)  # all-dead runs: both accumulators stay 1


# ---- final exponentiation of f = 1 --------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_final_exponentiation_of_one(twin, cname):  # noqa: F811
    """f = 1 (the Miller value of an all-identity cell): through final_exp on one lane, through f^x alone (on BLS12-381 the
    compressed squarings, whose shared inversion meets z2 = 0 and falls back to the uncompressed run), and through the
    three-thread cooperative form -- between two runs of a non-trivial f, whose results must not change (on the device the
    neighbours of a cooperative group in the wave hold other cells)."""
    c = curve(cname)
    FQ, FR, G1, G2, GT, CRS = ref.sizes(cname)
    one = np.zeros(GT, np.uint8)
    one[:FQ] = sv.u8(c.fq(1))
    mp, coop, expx = (getattr(twin, nm + cname) for nm in ("twin_multi_pairing_", "twin_coop_", "twin_exp_by_x_"))
    p0, _, q = _points(cname)[0]
    out = np.ones(GT, np.uint8)
    mp(1, ptr(np.zeros(G1, np.uint8)), ptr(q), ptr(out), 1)  # P = O: multi_miller leaves f = 1, final_exp follows
    assert (out == one).all()
    mp(1, ptr(p0), ptr(np.zeros(G2, np.uint8)), ptr(out), 1)
    assert (out == one).all()
    out = np.zeros(GT, np.uint8)
    expx(ptr(one), ptr(out))
    assert (out == one).all()
    e = c.golden["pairing"][0]
    miller = np.zeros(GT, np.uint8)
    mp(1, ptr(c.g1(e["p"])), ptr(c.g2(e["q"])), ptr(miller), 0)
    for what in (0, 1):
        seq = [miller, one, miller, one] if what else [sv.u8(c.f12(e["out"])), one, sv.u8(c.f12(e["out"])), one]
        res = []
        for f in seq:
            out3 = np.zeros(3 * GT, np.uint8)
            coop(what, ptr(f), ptr(out3))
            lanes = out3.reshape(3, GT)
            assert (lanes[1] == lanes[0]).all() and (lanes[2] == lanes[0]).all(), (cname, what)
            res.append(lanes[0].copy())
        assert (res[1] == one).all() and (res[3] == one).all(), (cname, what)
        assert (res[0] == res[2]).all()
        if what:
            assert c.f12_dec(res[0].view(np.uint64)) == e["out"]
        else:
            want = np.zeros(GT, np.uint8)
            expx(ptr(seq[0]), ptr(want))
            assert (res[0] == want).all()

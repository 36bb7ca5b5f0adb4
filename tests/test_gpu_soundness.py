"""Both verifiers against the oracle on WELL-FORMED forged proofs (tests/forge.py).

The rejection tests of the rest of the suite flip a bit in a coordinate: the point leaves the curve and any verifier that
reads it rejects.  Here every element of every input is a subgroup point or a canonical scalar, so that only the
Groth-Sahai equation can tell: every slot of the commitments and of the proof moved, negated, zeroed or swapped, every
constant, Gamma entry and target changed to another valid value, somebody else's honest proof, valid proofs that differ
from the prover's output (accepted), and -- on a hiding CRS whose trapdoors the test knows -- proofs that are wrong in
exactly ONE cell of the ComT comparison.  The rule is "the GPU verdict equals the verdict of oracle/gs_ref.c on every
entry" (the reference itself accepts forgeries of a slot the equation does not look at: golden ppe_ragged_3x1).

  exact verifier   gs_verify_batch[_dev], gs_verify_mixed_dev, gs_verify_statement, gs_multi_verify_batch: ok[e] per entry,
                   under the planner's own shapes and under forced kernel shapes (tests/test_gpu_variants.py SHAPES);
  batched verifier gs_verify_batch_rlc[_dev], gs_multi_verify_batch_rlc with FIXED, seeded rho (a test of arithmetic; the
                   CSPRNG contract of the header is about production): with Q[e][c] = lhs[e][c] / rhs'[e][c] from
                   ref_verify_cells (rhs' = the right-hand side without the PPE target) the header's convention
                   "FE(acc[0]) == acc[1]" means FE(acc[0]) = W = prod_{e,c} Q[e][c]^rho[e][c] (c = 2a + b) and
                   acc[1] = prod_e target_e^rho[e][3] (PPE; one otherwise).  acc[1] is compared byte for byte; acc[0] is an
                   un-exponentiated Miller value, not unique, and is compared through gs_gt_finalize(1, (acc[0], W)).
No tolerance anywhere: verdicts are bits.

Single-cell variants: PPE all four cells (through pi and through theta), MSMEG1 all four through pi, MSMEG2 all four
through theta, QuadEqu none (forge.py's header has the algebra).

The large-arity fold path (k_cell_fold, 334 x 334) gets three variants only: one oracle verify at that size was timed
at 15.7 s (8-core box, the oracle's own threads included).
Cofactor points (BLS12-381, endo = 0 only): H = [r]P of the cofactor subgroup of E(Fp) added to one xcoms and one theta
element.  The pairing's G1 argument is defined modulo r E(Fp) and the order of H is coprime to r, so the verdict does
not change; confirmed on the CPU first (oracle/gs_ref.c returns 1 on such an input), then required of both verifiers.

Wall time (same MI355X box, whole `-m gpu` suite, budget 900 s): 362 s before this file, 410 s with it (measured before
the four cofactor tests, 4 s, were added); `-m "not gpu"` suite on an 8-core box: 92 s before tests/test_forge_cpu.py,
234 s with it."""
import fnmatch
import random

import numpy as np
import pytest

import forge
from gpubatch import pool
from gsutil import curve
from test_gpu_variants import MILLER_KERNEL, SHAPES

pytestmark = pytest.mark.gpu

CURVES = [("bls12_381", 0), ("bn254", 1)]
TYPES = [0, 1, 2, 3]
TRAP = (0x1234567890ABCDEF1122334455667788, 0x0FEDCBA987654321AABBCCDDEEFF0011, 0x5DEECE66D5DEECE66D, 0x2545F4914F6CDD1D2545F491)
NMIN = 130  # a task has full and ragged waves
# forced shapes: every Miller kernel, line_tables 0 / 1, coop_fe 0 / 2, var_tab = 1
FORCED = ["twin6_straus8x2w5_lane", "single1_plain_coop_notab_overlap", "pair3_straus2_lane_overlap",
          "pair5dpp_straus4_coop_notab", "pair12_tab8_lane"]


# ---- building the batches -------------------------------------------------------------------------------------------
class Batch:
    """Entries (each the eight verifier inputs) of one type and shape under one CRS, with the oracle's cells."""

    def __init__(self, eq, entries):
        self.eq, self.entries, self.N = eq, entries, len(entries)
        self.cname, self.ty, self.m, self.n, self.crs = eq["cname"], eq["ty"], eq["m"], eq["n"], eq["crs"]
        distinct = {id(v): v for v in entries}
        res = dict(zip(distinct, pool().map(lambda v: forge.oracle_cells(eq, v), distinct.values())))
        self.cells = [res[id(v)] for v in entries]
        self.want = np.array([c[0] for c in self.cells], dtype=np.uint8)

    def arr(self, key, lo=0, hi=None):
        return np.concatenate([v[key] for v in self.entries[lo:hi]])

    def args(self, lo=0, hi=None):
        return tuple(self.arr(k, lo, hi) for k in forge.INPUTS)

    def names(self, idx):
        return [self.entries[i].get("name", "original") for i in idx]


def interleave(eq, variants, nmin=NMIN):
    """original, v, v, original, v, v, ... original: the list repeated until there are nmin entries"""
    out = []
    while len(out) < nmin:
        for i, v in enumerate(variants):
            if i % 2 == 0:
                out.append(eq)
            out.append(v)
    out.append(eq)
    return out


_EQ = {}


def drawn_equation(cname, cid, ty, m, n, hiding):
    """Equation 0 of a Workload batch (statement and witness drawn on the GPU as multiples of the CRS generators), proved
    by the C ORACLE under a CRS of the test's own over the same generators, and all its variants; equation 1 supplies
    `other`.  -> (eq, variants)"""
    key = (cname, ty, m, n, hiding)
    if key not in _EQ:
        import groth_sahai_rs_amd as gs
        from groth_sahai_rs_amd.workload import Workload

        eng = gs.Engine(cid, 0)
        wl = Workload(eng, ty=ty, N=2, m=m, n=n, seed=4242 + cid, corrupt_every=0)
        eng.sync()
        sh = wl.sh
        host = lambda t, per, e: t.cpu().numpy()[e * per:(e + 1) * per].copy()
        crs = forge.crs_pair(cname, wl.g1_gen, wl.g2_gen, *TRAP)[1 if hiding else 0]
        rng = random.Random(31 * ty + cid + (1000 if hiding else 0))
        eqs = []
        for e in (0, 1):
            eq = dict(cname=cname, ty=ty, m=m, n=n, crs=crs, X=host(wl.X, m * sh["sx"], e), Y=host(wl.Y, n * sh["sy"], e),
                      A=host(wl.A, n * sh["sx"], e), B=host(wl.B, m * sh["sy"], e), G=host(wl.Gamma, m * n * 32, e),
                      target=host(wl.target, sh["st"], e))
            eq.update(forge.prove(eq, *forge.rand_mats(eq, rng)))
            eqs.append(eq)
        eng.close()
        vs = forge.build(eqs[0], rng, other=eqs[1], trap=TRAP, hiding=hiding)
        _EQ[key] = (eqs[0], vs)
    return _EQ[key]


def golden_ragged(cname, hiding):
    key = (cname, "ragged", hiding)
    if key not in _EQ:
        c = curve(cname)
        case = [k for k in c.golden["cases"] if k["name"] == "ppe_ragged_3x1"][0]
        g = c.golden["crs"]
        rng = random.Random(77)
        crs = forge.crs_pair(cname, c.g1(g["g1"]), c.g2(g["g2"]), *TRAP)[1 if hiding else 0]
        eq = forge.golden_eq(cname, case, crs=crs, rng=rng)
        _EQ[key] = (eq, forge.build(eq, rng, other=forge.other_of(eq, rng), trap=TRAP, hiding=hiding))
    return _EQ[key]


_BATCH = {}


def full_batch(cname, cid, ty, m, n, hiding):
    key = (cname, ty, m, n, hiding)
    if key not in _BATCH:
        eq, vs = golden_ragged(cname, hiding) if (m, n) == (3, 1) else drawn_equation(cname, cid, ty, m, n, hiding)
        _BATCH[key] = Batch(eq, interleave(eq, vs))
    return _BATCH[key]


def engine(cid, crs, opts=None):
    import groth_sahai_rs_amd as gs

    eng = gs.Engine(cid, 0)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    eng.set_crs(crs)
    return eng


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def check_verdicts(b, ok, what):
    ok = np.asarray(ok).reshape(-1)
    bad = np.nonzero(ok != b.want)[0]
    assert bad.size == 0, (what, b.cname, b.ty, [(int(i), nm, int(b.want[i])) for i, nm in zip(bad[:6], b.names(bad[:6]))])


def verify_dev(eng, b):
    import torch

    t = [dev(a) for a in b.args()]
    ok = torch.zeros(b.N, dtype=torch.uint8, device="cuda:0")
    eng.verify_batch_dev(b.ty, b.N, b.m, b.n, *t, ok)
    eng.sync()
    return ok.cpu().numpy()


# ---- exact verifier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hiding", [False, True], ids=["binding", "hiding"])
@pytest.mark.parametrize("ty,m,n", [(0, 4, 4), (1, 4, 4), (2, 4, 4), (3, 4, 4), (0, 3, 1), (0, 8, 3)])
@pytest.mark.parametrize("cname,cid", CURVES)
def test_exact_verdicts_follow_the_oracle(cname, cid, ty, m, n, hiding):
    """Dense 4 x 4 of every type, the ragged golden 3 x 1 and an 8 x 3 PPE: the original and all its variants in ONE batch;
    host entry and device entry."""
    b = full_batch(cname, cid, ty, m, n, hiding)
    assert b.N >= NMIN and b.want[0] == 1 and b.want[-1] == 1 and (b.want == 0).any()
    if hiding and ty != 3:  # one variant per cell, all four cells
        assert {v.get("cell") for v in b.entries} >= {(0, 0), (0, 1), (1, 0), (1, 1)}
    eng = engine(cid, b.crs)
    try:
        check_verdicts(b, eng.verify_batch(b.ty, b.N, b.m, b.n, *b.args()), "gs_verify_batch")
        check_verdicts(b, verify_dev(eng, b), "gs_verify_batch_dev")
    finally:
        eng.close()


@pytest.mark.parametrize("shape", FORCED)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_exact_verdicts_under_forced_kernel_shapes(cname, cid, ty, shape):
    """The dense 4 x 4 batch (hiding CRS: the single-cell variants are in it) through every Miller kernel, stepped and
    table-read CRS lines, one-lane and cooperative final exponentiation, shared window tables; the profile names what
    ran."""
    o = SHAPES[shape]
    b = full_batch(cname, cid, ty, 4, 4, True)
    eng = engine(cid, b.crs, o)
    try:
        eng.prof_enable(True)
        eng.prof_reset()
        ok = verify_dev(eng, b)
        names = [p[0] for p in eng.prof_get()]
        eng.prof_enable(False)
        expect = [MILLER_KERNEL[o["miller_twin"]], "k_final.coop" if o["coop_fe"] == 2 else "k_final"]
        if o.get("var_tab") == 1:
            expect += ["k_tab_build.vg1", "k_var_tab8.vg1"]
        for want in expect:
            assert any(fnmatch.fnmatchcase(nm, want) for nm in names), (want, names)
        check_verdicts(b, ok, shape)
    finally:
        eng.close()


@pytest.mark.parametrize("cname,cid", CURVES)
def test_mixed_entry_one_part_per_type(cname, cid):
    import torch

    bs = [full_batch(cname, cid, ty, 4, 4, True) for ty in TYPES]
    eng = engine(cid, bs[0].crs)
    try:
        parts = []
        for b in bs:
            assert (b.crs == bs[0].crs).all()
            A, B, G, target, xc, yc, pi, th = (dev(a) for a in b.args())
            parts.append(dict(ty=b.ty, N=b.N, m=b.m, n=b.n, A=A, B=B, Gamma=G, target=target, xcoms=xc, ycoms=yc, pi=pi,
                              theta=th, ok=torch.zeros(b.N, dtype=torch.uint8, device="cuda:0")))
        eng.verify_mixed_dev(parts)
        eng.sync()
        for b, p in zip(bs, parts):
            check_verdicts(b, p["ok"].cpu().numpy(), "gs_verify_mixed_dev")
    finally:
        eng.close()


@pytest.mark.parametrize("cname,cid", CURVES)
def test_multi_three_shards_on_one_device(cname, cid):
    import groth_sahai_rs_amd as gs

    b = full_batch(cname, cid, 0, 4, 4, True)
    me = gs.MultiEngine(cid, devices=(0, 0, 0), shared_devices=True)
    try:
        me.set_crs(b.crs)
        check_verdicts(b, me.verify_batch(b.ty, b.N, b.m, b.n, *b.args()), "gs_multi_verify_batch")
    finally:
        me.close()


@pytest.mark.parametrize("cname,cid", CURVES)
def test_statement_with_a_forged_shared_commitment(cname, cid):
    """E equations over ONE list of commitments: a forged (well-formed) commitment must turn the verdict of every equation
    that uses it the way the oracle says, and of no other."""
    import gs_ref_py as ref
    from stmtutil import StatementInputs

    import groth_sahai_rs_amd as gs

    eng = gs.Engine(cid, 0)
    try:
        st = StatementInputs(eng, mg=3, ng=2, seed=6160)
        E = 5
        p = st.part(0, E)
        m, n = p["m"], p["n"]
        G = p["Gamma"].copy().reshape(E, m * n, 32)
        G[1, 0:n] = 0  # equation 1 does not look at x0 ...
        B = p["B"].copy().reshape(E, m, eng.G2)
        B[1, 0] = 0    # ... at all
        p["Gamma"], p["B"] = G.reshape(-1), B.reshape(-1)
        cx = forge.Ctx(cname, st.crs)
        # (the target of equation 1 loses the terms of x0: rebuild it with the oracle's pairing)
        cut = lambda a, e, sz: forge.u8(a)[e * sz:(e + 1) * sz]
        eqs = []
        for e in range(E):
            eq = dict(cname=cname, ty=0, m=m, n=n, crs=forge.u8(st.crs), X=forge.u8(p["X"]), Y=forge.u8(p["Y"]),
                      A=cut(p["A"], e, n * eng.G1), B=cut(p["B"], e, m * eng.G2), G=cut(p["Gamma"], e, m * n * 32),
                      target=cut(p["target"], e, eng.GT))
            out = ref.commit_and_prove(cname, 0, m, n, eq["X"], eq["Y"], eq["A"], eq["B"], eq["G"], forge.u8(p["R"]),
                                       forge.u8(p["S"]), cut(p["T"], e, 4 * 32), cx.crs)
            eq.update(out)
            if e == 1:  # target := lhs of cell (1,1) / rhs' of the honest proof = what the changed statement evaluates to
                _, lhs, _, rhs_nt = forge.oracle_cells(eq, eq)
                eq["target"] = ref.gt_mul(cname, lhs[3], ref.gt_inv(cname, rhs_nt[3]))
            eqs.append(eq)
        xc, yc = eqs[0]["xcoms"], eqs[0]["ycoms"]
        assert all((q["xcoms"] == xc).all() and (q["ycoms"] == yc).all() for q in eqs)
        cat = lambda k: np.concatenate([q[k] for q in eqs])
        run = lambda xc_, yc_: eng.verify_statement(0, E, m, n, cat("A"), cat("B"), cat("G"), cat("target"), xc_, yc_,
                                                    cat("pi"), cat("theta"))
        assert run(xc, yc).all()
        forged_x = xc.copy()
        forged_x[:eng.G1] = cx.add(1, xc[:eng.G1], cx.g1)  # xcoms[0].0 += gen
        forged_y = yc.copy()
        forged_y[eng.G2:2 * eng.G2] = cx.neg(2, yc[eng.G2:2 * eng.G2])  # ycoms[0].1 negated
        for what, fx, fy in (("xcoms[0].0 += gen", forged_x, yc), ("ycoms[0].1 negated", xc, forged_y)):
            want = [forge.oracle_verdict(q, dict(q, xcoms=fx, ycoms=fy)) for q in eqs]
            got = run(fx, fy)
            assert [int(v) for v in got] == want, (what, want, got)
            if fx is forged_x:
                assert want == [0, 1, 0, 0, 0], want  # equation 1 does not use x0
    finally:
        eng.close()


@pytest.mark.parametrize("cname,cid", CURVES[:1])
def test_large_arity_fold_path(cname, cid):
    """m = n = 334 (the reference's large bench shape): a pi slot, the LAST xcoms slot and one Gamma entry, through
    k_cell_fold.  Honest proof by the C oracle."""
    import torch

    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.workload import Workload

    m = n = 334
    eng = gs.Engine(cid, 0)
    try:
        wl = Workload(eng, ty=0, N=1, m=m, n=n, seed=3340, corrupt_every=0)
        eng.sync()
        host = lambda t: t.cpu().numpy().copy()
        eq = dict(cname=cname, ty=0, m=m, n=n, crs=forge.u8(wl.crs), X=host(wl.X), Y=host(wl.Y), A=host(wl.A), B=host(wl.B),
                  G=host(wl.Gamma), target=host(wl.target))
        import gs_ref_py as ref

        eq.update(ref.commit_and_prove(cname, 0, m, n, eq["X"], eq["Y"], eq["A"], eq["B"], eq["G"], host(wl.R), host(wl.S),
                                       host(wl.T), eq["crs"]))
        cx = forge.Ctx(cname, eq["crs"])

        def moved(key, group, slot):
            a, sz = eq[key].copy(), cx.size(group)
            a[slot * sz:(slot + 1) * sz] = cx.add(group, a[slot * sz:(slot + 1) * sz], cx.gen(group))
            return a

        gi = (m - 1) * n + 7
        g = eq["G"].copy()
        g[gi * 32:(gi + 1) * 32] = cx.fr(cx.fr_ints(g[gi * 32:(gi + 1) * 32])[0] + 1)
        vs = [dict(eq, name="pi[1].0 += gen", pi=moved("pi", 2, 2)),
              dict(eq, name="xcoms[333].1 += gen", xcoms=moved("xcoms", 1, 2 * m - 1)),
              dict(eq, name="Gamma[333][7] += 1", G=g)]
        b = Batch(eq, [eq, vs[0], vs[1], eq, vs[2]])
        assert list(b.want) == [1, 0, 0, 1, 0], b.want
        eng.prof_enable(True)
        eng.prof_reset()
        t = [dev(a) for a in b.args()]
        ok = torch.zeros(b.N, dtype=torch.uint8, device="cuda:0")
        eng.verify_batch_dev(0, b.N, m, n, *t, ok)
        eng.sync()
        names = [p[0] for p in eng.prof_get()]
        eng.prof_enable(False)
        assert "k_cell_fold" in names, names
        check_verdicts(b, ok.cpu().numpy(), "large arity")
    finally:
        eng.close()


# ---- batched verifier -------------------------------------------------------------------------------------------------
EDGE_RHO = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]


def seeded_rho(N, seed):
    """Fixed exponents: random rows (all four cells different) with rows of edge values, all four cells equal, on the
    first entries -- originals and variants alike -- and again at the end."""
    rho = np.random.default_rng(seed).integers(1, 1 << 64, size=(N, 4), dtype=np.uint64, endpoint=False)
    for i, v in enumerate(EDGE_RHO):
        rho[i % N] = v
        rho[(N - 1 - i) % N] = v
    mixed = np.array([(1 << 64) - 1, 1, 1 << 32, (1 << 63) + 5], dtype=np.uint64)
    rho[len(EDGE_RHO) % N] = mixed
    return rho


def gt_one(cname):
    c = curve(cname)
    return forge.u8(c.f12(["1"] + ["0"] * 11))


def oracle_rlc(b, rho, lo=0, hi=None):
    """(W, T) = (prod Q[e][c]^rho[e][c], prod target_e^rho[e][3] or one) over entries [lo, hi) with ref_gt_pow"""
    import gs_ref_py as ref

    cn, c = b.cname, curve(b.cname)
    hi = b.N if hi is None else hi
    one = gt_one(cn)

    def entry(e):
        _, lhs, rhs, rhs_nt = b.cells[e]
        den = rhs_nt if b.ty == 0 else rhs
        w = one
        for k in range(4):
            if (lhs[k] != den[k]).any():
                q = ref.gt_mul(cn, lhs[k], ref.gt_inv(cn, den[k]))
                w = ref.gt_mul(cn, w, ref.gt_pow(cn, q, forge.u8(c.fr(int(rho[e][k])))))
        t = ref.gt_pow(cn, b.entries[e]["target"], forge.u8(c.fr(int(rho[e][3])))) if b.ty == 0 else one
        return w, t

    W, T = one, one
    for w, t in pool().map(entry, range(lo, hi)):
        W, T = ref.gt_mul(cn, W, w), ref.gt_mul(cn, T, t)
    return W, T


def check_rlc(eng, b, rho, what, want_ok=None):
    """One batch through the host and the device entry against the oracle's W and T.  -> (ok_all, acc)"""
    import torch

    import gs_ref_py as ref

    GT = eng.GT
    W, T = oracle_rlc(b, rho)
    ok_all, acc = eng.verify_batch_rlc(b.ty, b.N, b.m, b.n, *b.args(), rho)
    acc = np.array(acc, dtype=np.uint8).copy()
    where = (what, b.cname, b.ty)
    assert (acc[GT:] == T).all(), (where, "acc[1] != prod target^rho[3]")
    assert eng.gt_finalize(np.concatenate([acc[:GT], W])) == 1, (where, "FE(acc[0]) != W")
    assert eng.gt_finalize(np.concatenate([acc[:GT], ref.gt_mul(b.cname, W, forge.Ctx(b.cname, b.crs).gt)])) == 0, where
    assert ok_all == int((W == T).all()), (where, "verdict", ok_all)
    assert eng.gt_finalize(acc) == ok_all, where
    if want_ok is not None:
        assert ok_all == want_ok, (where, ok_all)
    dacc = torch.zeros(2 * GT, dtype=torch.uint8, device="cuda:0")
    t = [dev(a) for a in b.args()]
    eng.verify_batch_rlc_dev(b.ty, b.N, b.m, b.n, *t, dev(rho.view(np.int64).reshape(-1)), dacc)
    eng.sync()
    assert (dacc.cpu().numpy() == acc).all(), (where, "host and _dev accumulators differ")
    return ok_all, acc


def valid_batch(cname, cid, ty):
    """originals and the accepted variants only (binding CRS: the cancelling kind is among them)"""
    key = (cname, ty, "valid")
    if key not in _BATCH:
        eq, vs = drawn_equation(cname, cid, ty, 4, 4, False)
        _BATCH[key] = Batch(eq, interleave(eq, [v for v in vs if v["accepted"]]))
    return _BATCH[key]


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_batched_accumulators_follow_the_oracle(cname, cid, ty):
    """Batches that mix originals and variants (all kinds, hiding CRS), and a batch of valid proofs only."""
    b = full_batch(cname, cid, ty, 4, 4, True)
    eng = engine(cid, b.crs)
    try:
        check_rlc(eng, b, seeded_rho(b.N, 900 + ty), "forged", want_ok=0)
        v = valid_batch(cname, cid, ty)
        assert v.N >= NMIN and v.want.all()
        eng.set_crs(v.crs)
        check_rlc(eng, v, seeded_rho(v.N, 950 + ty), "valid", want_ok=1)
    finally:
        eng.close()


@pytest.mark.parametrize("cname,cid", CURVES)
def test_batched_cancelling_pairs(cname, cid):
    """Two PPE targets multiplied by z and 1/z: with equal rho[.][3] the oracle's formula and the GPU accept the batch,
    with different ones both reject.  The same with the two single-cell variants of one pi column (cells (1,b) and (0,b)
    are off by e(p1,p2)^-w and e(p1,p2)^w): equal exponents in those two cells cancel."""
    import gs_ref_py as ref

    v = valid_batch(cname, cid, 0)
    cx = forge.Ctx(cname, v.crs)
    z = ref.gt_pow(cname, cx.gt, cx.fr(0xABCDEF0123456789ABCDEF))
    e1, e2 = 3, v.N - 2
    ents = list(v.entries)
    ents[e1] = dict(ents[e1], name="target * z", target=ref.gt_mul(cname, ents[e1]["target"], z))
    ents[e2] = dict(ents[e2], name="target / z", target=ref.gt_mul(cname, ents[e2]["target"], ref.gt_inv(cname, z)))
    b = Batch(v.eq, ents)
    assert b.want[e1] == 0 and b.want[e2] == 0 and b.want.sum() == b.N - 2
    eng = engine(cid, b.crs)
    try:
        rho = seeded_rho(b.N, 31)
        rho[e1][3] = rho[e2][3] = (1 << 63) + 12345
        check_rlc(eng, b, rho, "z, 1/z, equal rho", want_ok=1)
        rho[e2][3] += 1
        check_rlc(eng, b, rho, "z, 1/z, different rho", want_ok=0)
        # single-cell pair on the hiding CRS
        eq, vs = drawn_equation(cname, cid, 0, 4, 4, True)
        col = [x for x in vs if x["kind"] == "cell" and "pi[.].1" in x["name"]]
        lo = [x for x in col if x["cell"] == (1, 1)][0]
        hi = [x for x in col if x["cell"] == (0, 1)][0]
        ents = interleave(eq, [x for x in vs if x["accepted"]])
        ents[5], ents[70] = lo, hi
        b2 = Batch(eq, ents)
        assert b2.want.sum() == b2.N - 2
        eng.set_crs(b2.crs)
        rho = seeded_rho(b2.N, 32)
        rho[5][3] = rho[70][1] = (1 << 32) + 7
        check_rlc(eng, b2, rho, "cells (1,1) and (0,1), equal rho", want_ok=1)
        rho[70][1] += 1
        check_rlc(eng, b2, rho, "cells (1,1) and (0,1), different rho", want_ok=0)
    finally:
        eng.close()


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_batched_split_invariance_with_forged_entries(cname, cid, ty):
    """Accumulators of [0, k) and [k, N) finalize to the whole batch's verdict and to the oracle's W of each half; the
    same through gs_multi_verify_batch_rlc with three shards."""
    import groth_sahai_rs_amd as gs

    for b, want in ((full_batch(cname, cid, ty, 4, 4, True), 0), (valid_batch(cname, cid, ty), 1)):
        rho = seeded_rho(b.N, 400 + ty)
        eng = engine(cid, b.crs)
        try:
            GT = eng.GT
            whole, _ = eng.verify_batch_rlc(b.ty, b.N, b.m, b.n, *b.args(), rho)
            assert whole == want
            for k in (1, 64, b.N - 1):
                accs = []
                for lo, hi in ((0, k), (k, b.N)):
                    _, acc = eng.verify_batch_rlc(b.ty, hi - lo, b.m, b.n, *b.args(lo, hi), rho[lo:hi])
                    acc = np.array(acc, dtype=np.uint8).copy()
                    W, T = oracle_rlc(b, rho, lo, hi)
                    assert (acc[GT:] == T).all(), (cname, ty, k, lo)
                    assert eng.gt_finalize(np.concatenate([acc[:GT], W])) == 1, (cname, ty, k, lo)
                    accs.append(acc)
                assert eng.gt_finalize(np.concatenate(accs)) == whole, (cname, ty, k)
        finally:
            eng.close()
        me = gs.MultiEngine(cid, devices=(0, 0, 0), shared_devices=True)
        try:
            me.set_crs(b.crs)
            ok_all, pairs = me.verify_batch_rlc(b.ty, b.N, b.m, b.n, *b.args(), rho)
            assert ok_all == want, (cname, ty, "gs_multi_verify_batch_rlc")
            pairs = np.array(pairs, dtype=np.uint8).reshape(3, 2, -1)
            for i in range(3):
                lo, hi = me.shard(b.N, i)
                W, T = oracle_rlc(b, rho, lo, hi)
                assert (pairs[i][1] == T).all(), (cname, ty, "shard", i)
            W, _ = oracle_rlc(b, rho)
            eng = engine(cid, b.crs)
            try:  # the product of the shards' acc[0] against the whole batch's W
                one = gt_one(cname)
                assert eng.gt_finalize(np.concatenate([pairs[0][0], W, pairs[1][0], one, pairs[2][0], one])) == 1
            finally:
                eng.close()
        finally:
            me.close()


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("cname,cid", CURVES)
def test_batched_verifier_without_endomorphisms(cname, cid, ty):
    """gs_set_option("endo", 0) reaches the batched verifier: plain double-and-add lanes only (no k_var_multi* kernel),
    the same acc[1], verdict and W check as with endo = 1; also through the shards of gs_multi."""
    import groth_sahai_rs_amd as gs

    for b, want in ((full_batch(cname, cid, ty, 4, 4, True), 0), (valid_batch(cname, cid, ty), 1)):
        rho = seeded_rho(b.N, 700 + ty)
        accs = {}
        for endo in (1, 0):
            eng = engine(cid, b.crs, {"endo": endo})
            try:
                eng.prof_enable(True)
                eng.prof_reset()
                _, accs[endo] = check_rlc(eng, b, rho, "endo = %d" % endo, want_ok=want)
                names = sorted({p[0] for p in eng.prof_get()})
                eng.prof_enable(False)
                multi = [nm for nm in names if nm.startswith("k_var_multi")]
                if endo:
                    assert multi, names  # (the check below would be empty if the name had changed)
                else:
                    assert not multi, names
                    assert any(nm.startswith("k_var.plain") for nm in names), names
            finally:
                eng.close()
        GT = accs[0].size // 2
        assert (accs[0][GT:] == accs[1][GT:]).all()
        me = gs.MultiEngine(cid, devices=(0, 0, 0), shared_devices=True)
        try:
            me.set_crs(b.crs)
            me.set_option("endo", 0)
            ok_all, _ = me.verify_batch_rlc(b.ty, b.N, b.m, b.n, *b.args(), rho)
            assert ok_all == want
        finally:
            me.close()


@pytest.mark.parametrize("ty", TYPES)
def test_cofactor_points_without_endomorphisms(ty):
    """BLS12-381: a point of the cofactor subgroup of E(Fp) added to one commitment and one theta element changes no
    pairing value.  With endo = 0 (plain double-and-add: rho (C + H) = rho C + rho H) the exact and the batched verdict
    equal the oracle's, which is 1."""
    from test_gpu_subgroup import curve_points

    cname, cid = CURVES[0]
    c = curve(cname)
    v = valid_batch(cname, cid, ty)
    cx = forge.Ctx(cname, v.crs)
    P = curve_points(cname, 1, 1, 1234)[0]
    Pb = forge.u8(np.concatenate([c.fq(P[0]), c.fq(P[1])]))
    H = cx.add(1, cx.mul(1, Pb, c.r - 1), Pb)  # [r]P: order divides the cofactor
    assert H.any() and cx.add(1, cx.mul(1, H, c.r - 1), H).any(), "H must lie outside the r-torsion"

    def shifted(key, slot):
        a = v.eq[key].copy()
        a[slot * cx.G1:(slot + 1) * cx.G1] = cx.add(1, a[slot * cx.G1:(slot + 1) * cx.G1], H)
        return a

    vs = [dict(v.eq, name="xcoms[1].1 += H", xcoms=shifted("xcoms", 3)),
          dict(v.eq, name="theta[0].0 += H", theta=shifted("theta", 0)),
          dict(v.eq, name="xcoms[3].0, theta[0].1 += H", xcoms=shifted("xcoms", 6), theta=shifted("theta", 1))]
    ents = list(v.entries)
    for i, x in zip((0, 1, 64, 65, v.N - 1), vs + vs):
        ents[i] = x
    b = Batch(v.eq, ents)
    assert b.want.all(), b.want  # the premise, by the oracle
    eng = engine(cid, b.crs, {"endo": 0})
    try:
        check_verdicts(b, eng.verify_batch(b.ty, b.N, b.m, b.n, *b.args()), "cofactor, gs_verify_batch, endo = 0")
        check_verdicts(b, verify_dev(eng, b), "cofactor, gs_verify_batch_dev, endo = 0")
        check_rlc(eng, b, seeded_rho(b.N, 800 + ty), "cofactor, endo = 0", want_ok=1)
    finally:
        eng.close()

"""gs_set_simulation_key / gs_simulate_batch / gs_simulate_statement on the GPU (include/gs_amd.h): whoever drew t1, t2 of
a hiding CRS answers every equation without a witness.  Every check is against tests/simvec.py (the formulas, on the C
oracle's arithmetic; tests/test_sim_algebra.py holds the same formulas against the reference's verifier and prover) AND
against the library's own verifiers under the hiding CRS.  The CRS comes from forge.crs_pair, so the test knows the
trapdoor.  Shapes: 1 x 1, 2 x 3, 3 x 1 (odd, both orientations), N = 65 (a wave and one lane), 40 x 30 (m n above the
wide-preparation threshold of the prover, several Straus groups per output)."""
import os
import random
import sys

import numpy as np
import pytest

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu

CURVES = [(0, "bls12_381"), (1, "bn254")]
MSMEG1, MSMEG2, QUAD = 1, 2, 3
TYPES = [MSMEG1, MSMEG2, QUAD]
TRAP = dict(a1=0x1234567, a2=0x7654321, t1=0xABCDEF0123, t2=0x3210FEDCBA)
OUTS = ("xcoms", "ycoms", "pi", "theta")


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Sim:
    """One engine per curve on a hiding CRS whose trapdoor the test knows, the key installed."""

    def __init__(self, cid, cname):
        import forge
        import groth_sahai_rs_amd as gs
        import gs_ref_py as ref

        self.cid, self.cname, self.c, self.ref = cid, cname, curve(cname), ref
        self.r = self.c.r
        g = self.c.golden["crs"]
        self.g1, self.g2 = u8(self.c.g1(g["g1"])), u8(self.c.g2(g["g2"]))
        rnd = random.Random(5100 + cid)
        self.t1, self.t2 = rnd.randrange(2, self.r), rnd.randrange(2, self.r)
        self.binding, self.hiding = forge.crs_pair(cname, self.g1, self.g2, TRAP["a1"], TRAP["a2"], self.t1, self.t2)
        self.key = self.frs([self.t1, self.t2])
        self.eng = gs.Engine(cid, 0)
        self.eng.set_crs(self.hiding)
        self.eng.set_simulation_key(self.key)

    def frs(self, vals):
        if len(vals) == 0:
            return np.zeros(0, dtype=np.uint8)
        return u8(np.concatenate([self.c.fr(v % self.r) for v in vals]))

    def pts(self, group, ks):
        """k gen for every k (k = 0: the identity, all-zero bytes), by the C oracle"""
        gen = self.g1 if group == 1 else self.g2
        return np.concatenate([self.ref.g_mul(self.cname, group, gen, self.frs([k])) for k in ks])


_S = {}
PLANNED = dict(endo=1, var_tm=0, var_w=0, red_k=0)


def sim(cid, cname):
    if cid not in _S:
        _S[cid] = Sim(cid, cname)
    return _S[cid]


def xg(ty):
    return ty == MSMEG1


def yg(ty):
    return ty == MSMEG2


def kxy(ty):
    return (2 if xg(ty) else 1), (2 if yg(ty) else 1)


class Case:
    """N equations of one type and shape as lists of integers per equation (group-valued constants and targets by their
    discrete logarithms), with the byte arrays the entry points take and the model's outputs."""

    def __init__(self, K, ty, N, m, n, seed):
        self.K, self.ty, self.N, self.m, self.n = K, ty, N, m, n
        rnd = random.Random(seed)
        fr = lambda: rnd.randrange(1, K.r)
        kx, ky = kxy(ty)
        mat = lambda p, q: [[fr() for _ in range(q)] for _ in range(p)]
        self.a = [[fr() for _ in range(n)] for _ in range(N)]
        self.b = [[fr() for _ in range(m)] for _ in range(N)]
        self.G = [mat(m, n) for _ in range(N)]
        self.t = [fr() for _ in range(N)]
        self.Rc = [mat(m, kx) for _ in range(N)]
        self.Sc = [mat(n, ky) for _ in range(N)]
        self.Tf = [mat(ky, kx) for _ in range(N)]

    def arrays(self, shared=False):
        """A, B, Gamma, target, Rc, Sc, Tf in bytes; shared: ONE copy of Rc, Sc (equation 0's)"""
        K, ty, flat = self.K, self.ty, lambda M: [v for row in M for v in row]
        cat = lambda xs: [v for x in xs for v in x]
        A = K.pts(1, cat(self.a)) if xg(ty) else K.frs(cat(self.a))
        B = K.pts(2, cat(self.b)) if yg(ty) else K.frs(cat(self.b))
        tg = K.pts(1, self.t) if ty == MSMEG1 else K.pts(2, self.t) if ty == MSMEG2 else K.frs(self.t)
        V = 1 if shared else self.N
        return dict(A=A, B=B, Gamma=K.frs(cat(flat(g) for g in self.G)), target=tg,
                    Rc=K.frs(cat(flat(r) for r in self.Rc[:V])), Sc=K.frs(cat(flat(s) for s in self.Sc[:V])),
                    Tf=K.frs(cat(flat(t) for t in self.Tf)))

    def model(self, arr, shared=False):
        """the model's outputs for every equation, concatenated per array"""
        import simvec
        from gpubatch import pool

        K, ty, m, n = self.K, self.ty, self.m, self.n
        eng = K.eng
        sx, sy = (eng.G1 if xg(ty) else 32), (eng.G2 if yg(ty) else 32)
        st = eng.G1 if ty == MSMEG1 else eng.G2 if ty == MSMEG2 else 32
        cut = lambda a, e, sz: a[e * sz:(e + 1) * sz]

        def one(e):
            v = 0 if shared else e
            return simvec.simulate_bytes(K.cname, K.hiding, ty, m, n, K.t1, K.t2, cut(arr["A"], e, n * sx),
                                         cut(arr["B"], e, m * sy), cut(arr["Gamma"], e, m * n * 32),
                                         cut(arr["target"], e, st), self.Rc[v], self.Sc[v], self.Tf[e])

        outs = list(pool().map(one, range(self.N)))
        V = 1 if shared else self.N
        return dict(xcoms=np.concatenate([o["xcoms"] for o in outs[:V]]),
                    ycoms=np.concatenate([o["ycoms"] for o in outs[:V]]),
                    pi=np.concatenate([o["pi"] for o in outs]), theta=np.concatenate([o["theta"] for o in outs]))


def same(got, want, what):
    for k in OUTS:
        assert got[k].size == want[k].size, (what, k)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, k, "first differing byte", int(bad[0]), "of", got[k].size)


def verifies(K, cs, arr, out, rlc=True):
    eng = K.eng
    v = (arr["A"], arr["B"], arr["Gamma"], arr["target"], out["xcoms"], out["ycoms"], out["pi"], out["theta"])
    ok = eng.verify_batch(cs.ty, cs.N, cs.m, cs.n, *v)
    assert ok.all(), ("gs_verify_batch", np.nonzero(ok == 0)[0][:8])
    if rlc:
        rnd = random.Random(991)
        rho = np.array([rnd.randrange(1, 1 << 64) for _ in range(4 * cs.N)], dtype=np.uint64)
        ok_all, _ = eng.verify_batch_rlc(cs.ty, cs.N, cs.m, cs.n, *v, rho)
        assert ok_all == 1, "gs_verify_batch_rlc"


def run(K, cs, arr=None, rlc=True, what=""):
    arr = cs.arrays() if arr is None else arr
    out = K.eng.simulate_batch(cs.ty, cs.N, cs.m, cs.n, **arr)
    same(out, cs.model(arr), what)
    verifies(K, cs, arr, out, rlc)
    return arr, out


# ---- 1. parity with the model, and the verifiers' verdicts ----------------------------------------------------------------
PARITY = [(ty, N, m, n) for ty in TYPES for (N, m, n) in ((1, 1, 1), (2, 2, 3), (9, 3, 1), (65, 1, 1))] + \
         [(ty, 2, 40, 30) for ty in (MSMEG1, QUAD)]


@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty,N,m,n", PARITY)
def test_parity_and_verdicts(cid, cname, ty, N, m, n):
    K = sim(cid, cname)
    run(K, Case(K, ty, N, m, n, 1000 * ty + 10 * N + m), what=(cname, ty, N, m, n))


# ---- 2. honest = simulated, byte for byte ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_honest_proof_equals_simulated_proof(cid, cname, ty):
    import simvec

    K = sim(cid, cname)
    eng, r, N, m, n = K.eng, K.r, 2, 2, 3
    cs = Case(K, ty, N, m, n, 2000 + ty)
    rnd = random.Random(2100 + ty)
    kx, ky = kxy(ty)
    mat = lambda p, q: [[rnd.randrange(1, r) for _ in range(q)] for _ in range(p)]
    xs = [[rnd.randrange(1, r) for _ in range(m)] for _ in range(N)]  # X_i = xs_i g1 where X is group-valued
    ys = [[rnd.randrange(1, r) for _ in range(n)] for _ in range(N)]
    R, S, T = [mat(m, kx) for _ in range(N)], [mat(n, ky) for _ in range(N)], [mat(ky, kx) for _ in range(N)]
    for e in range(N):  # the satisfied target, as the discrete logarithm Case.arrays() takes
        a, b, G = cs.a[e], cs.b[e], cs.G[e]
        cs.t[e] = (sum(a[j] * ys[e][j] for j in range(n)) + sum(xs[e][i] * b[i] for i in range(m)) +
                   sum(xs[e][i] * G[i][j] * ys[e][j] for i in range(m) for j in range(n))) % r
        # scalar constants enter honest_coordinates as themselves, group-valued ones do not enter at all
        cs.Rc[e], cs.Sc[e], cs.Tf[e] = simvec.honest_coordinates(ty, r, K.t1, K.t2, a, b, G, xs[e], ys[e], R[e], S[e],
                                                                 T[e])
    arr = cs.arrays()
    flat = lambda Ms: K.frs([v for M in Ms for row in M for v in row])
    cat = lambda xs_: [v for x in xs_ for v in x]
    X = K.pts(1, cat(xs)) if xg(ty) else K.frs(cat(xs))
    Y = K.pts(2, cat(ys)) if yg(ty) else K.frs(cat(ys))
    honest = eng.prove_batch(ty, N, m, n, X, Y, arr["A"], arr["B"], arr["Gamma"], flat(R), flat(S), flat(T))
    simulated = eng.simulate_batch(ty, N, m, n, **arr)
    same(simulated, honest, "simulated against gs_prove_batch under the hiding CRS")
    verifies(K, cs, arr, simulated)


# ---- 3. the commitments are gs_commit_* of the zero witness ---------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_commitments_are_those_of_the_zero_witness(cid, cname, ty):
    K = sim(cid, cname)
    eng, N, m, n = K.eng, 3, 2, 3
    cs = Case(K, ty, N, m, n, 3000 + ty)
    arr = cs.arrays()
    out = eng.simulate_batch(ty, N, m, n, **arr)
    zx = np.zeros(N * m * (eng.G1 if xg(ty) else 32), np.uint8)
    zy = np.zeros(N * n * (eng.G2 if yg(ty) else 32), np.uint8)
    assert (u8(eng.commit("g1" if xg(ty) else "fr_b1", zx, arr["Rc"])) == out["xcoms"]).all()
    assert (u8(eng.commit("g2" if yg(ty) else "fr_b2", zy, arr["Sc"])) == out["ycoms"]).all()
    nocoms = eng.simulate_batch(ty, N, m, n, want_coms=False, **arr)  # xcoms / ycoms may be NULL
    assert nocoms["xcoms"] is None and (nocoms["pi"] == out["pi"]).all() and (nocoms["theta"] == out["theta"]).all()


# ---- 4. a simulated proof is rerandomized like any other ------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_rerandomized_simulated_proof_verifies(cid, cname, ty):
    K = sim(cid, cname)
    eng, N, m, n = K.eng, 2, 2, 3
    cs = Case(K, ty, N, m, n, 4000 + ty)
    arr = cs.arrays()
    out = eng.simulate_batch(ty, N, m, n, **arr)
    fresh = Case(K, ty, N, m, n, 4100 + ty).arrays()
    rr = eng.rerandomize_batch(ty, N, m, n, arr["A"], arr["B"], arr["Gamma"], out["xcoms"], out["ycoms"], out["pi"],
                               out["theta"], fresh["Rc"], fresh["Sc"], fresh["Tf"])
    assert (rr["pi"] != out["pi"]).any() and (rr["xcoms"] != out["xcoms"]).any()
    verifies(K, cs, arr, rr)


# ---- 5. host form = _dev form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_host_form_equals_dev_form(cid, cname, ty):
    import torch

    K = sim(cid, cname)
    eng, N, m, n = K.eng, 5, 2, 3
    cs = Case(K, ty, N, m, n, 5000 + ty)
    arr = cs.arrays()
    host = eng.simulate_batch(ty, N, m, n, **arr)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in arr.items()}
    outs = {k: torch.zeros(host[k].size, dtype=torch.uint8, device="cuda") for k in OUTS}
    eng.simulate_batch_dev(ty, N, m, n, *dev.values(), *outs.values())
    eng.sync()
    same({k: v.cpu().numpy() for k, v in outs.items()}, host, "_dev against host")


# ---- 6. Statement: E = 5 over one commitment set --------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_statement_equals_batch_calls_and_verifies(cid, cname, ty):
    import torch

    K = sim(cid, cname)
    eng, E, m, n = K.eng, 5, 2, 3
    cs = Case(K, ty, E, m, n, 6000 + ty)
    arr = cs.arrays(shared=True)
    st = eng.simulate_statement(ty, E, m, n, **arr)
    same(st, cs.model(arr, shared=True), "statement against the model")
    for e in range(E):  # five batch calls with the same Rc, Sc
        one = Case(K, ty, 1, m, n, 0)
        one.a, one.b, one.G, one.t, one.Tf = [cs.a[e]], [cs.b[e]], [cs.G[e]], [cs.t[e]], [cs.Tf[e]]
        one.Rc, one.Sc = [cs.Rc[0]], [cs.Sc[0]]
        o = eng.simulate_batch(ty, 1, m, n, **one.arrays())
        assert (o["xcoms"] == st["xcoms"]).all() and (o["ycoms"] == st["ycoms"]).all()
        for k, per in (("pi", st["pi"].size // E), ("theta", st["theta"].size // E)):
            assert (o[k] == st[k][e * per:(e + 1) * per]).all(), (k, e)
    ok = eng.verify_statement(ty, E, m, n, arr["A"], arr["B"], arr["Gamma"], arr["target"], st["xcoms"], st["ycoms"],
                              st["pi"], st["theta"])
    assert ok.all()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in arr.items()}
    outs = {k: torch.zeros(st[k].size, dtype=torch.uint8, device="cuda") for k in OUTS}
    eng.simulate_statement_dev(ty, E, m, n, *dev.values(), *outs.values())
    eng.sync()
    same({k: v.cpu().numpy() for k, v in outs.items()}, st, "statement: _dev against host")


# ---- 7. edges, one batch per type: every equation is one edge -------------------------------------------------------------
def edge_case(K, ty, seed):
    """(Case, names): 2 x 3 equations, equation k carries edge names[k]"""
    import simvec

    m, n, r = 2, 3, K.r
    names = ["gamma_zero", "ab_zero", "identity_consts", "identity_target", "V_identity", "Rc_zero", "Sc_zero",
             "theta_coefficient_zero", "Tf_zero", "equal_consts", "opposite_consts", "plain"]
    cs = Case(K, ty, len(names), m, n, seed)
    at = names.index
    cs.G[at("gamma_zero")] = [[0] * n for _ in range(m)]
    e = at("ab_zero")  # the scalar constants (a group-valued side's constants: the identity, next edge)
    cs.a[e], cs.b[e] = [0] * n, [0] * m
    e = at("identity_consts")
    if xg(ty):
        cs.a[e] = [0] * n
    if yg(ty):
        cs.b[e] = [0] * m
    cs.t[at("identity_target")] = 0
    # V = sum_j Sc_j A_j - t2 T (MSMEG1) / sum_i Rc_i B_i - t1 T (MSMEG2) is the identity
    e = at("V_identity")
    if ty == MSMEG1:
        cs.t[e] = sum(cs.Sc[e][j][0] * cs.a[e][j] for j in range(n)) * pow(K.t2, -1, r) % r
    if ty == MSMEG2:
        cs.t[e] = sum(cs.Rc[e][i][0] * cs.b[e][i] for i in range(m)) * pow(K.t1, -1, r) % r
    kx, ky = kxy(ty)
    cs.Rc[at("Rc_zero")] = [[0] * kx for _ in range(m)]
    cs.Sc[at("Sc_zero")] = [[0] * ky for _ in range(n)]
    cs.Tf[at("Tf_zero")] = [[0] * kx for _ in range(ky)]
    # Tf such that the first fixed-base coefficient of the element that carries the sums is zero (theta for MSMEG1, pi
    # for MSMEG2 and QuadEqu): that coefficient is (sum - Tf[0][0])
    e = at("theta_coefficient_zero")
    th, pi, _, _ = simvec.coefficients(ty, r, K.t1, K.t2, cs.a[e], cs.b[e], cs.G[e], cs.t[e], cs.Rc[e], cs.Sc[e],
                                       cs.Tf[e])
    cs.Tf[e][0][0] = (cs.Tf[e][0][0] + (th[0][0] if ty == MSMEG1 else pi[0][0])) % r
    th, pi, _, _ = simvec.coefficients(ty, r, K.t1, K.t2, cs.a[e], cs.b[e], cs.G[e], cs.t[e], cs.Rc[e], cs.Sc[e],
                                       cs.Tf[e])
    assert (th[0][0] if ty == MSMEG1 else pi[0][0]) == 0
    # the Straus collisions: two equal constants with equal scalars, and two opposite ones
    for name, sign in (("equal_consts", 1), ("opposite_consts", -1)):
        e = at(name)
        if ty == MSMEG1:
            cs.a[e][1] = sign * cs.a[e][0] % r
            cs.Sc[e][1] = list(cs.Sc[e][0])
        if ty == MSMEG2:
            cs.b[e][1] = sign * cs.b[e][0] % r
            cs.Rc[e][1] = list(cs.Rc[e][0])
    return cs, names


@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_edges(cid, cname, ty):
    K = sim(cid, cname)
    cs, names = edge_case(K, ty, 7000 + ty)
    arr, out = run(K, cs, what=("edges", names))
    eng = K.eng
    e = names.index("Rc_zero")  # identity commitments are all-zero bytes
    per = cs.m * eng.COM1
    assert not out["xcoms"][e * per:(e + 1) * per].any()
    e = names.index("Sc_zero")
    per = cs.n * eng.COM2
    assert not out["ycoms"][e * per:(e + 1) * per].any()
    if ty == QUAD:  # Tf = 0: theta is the identity
        e = names.index("Tf_zero")
        assert not out["theta"][e * eng.COM1:(e + 1) * eng.COM1].any()


# ---- 8. forced kernel shapes ----------------------------------------------------------------------------------------------
FORCED = [dict(endo=0), dict(var_tm=1), dict(var_tm=8), dict(var_w=5, var_tm=4), dict(red_k=1)]


@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_forced_shapes(cid, cname, ty):
    K = sim(cid, cname)
    cs = Case(K, ty, 3, 2, 3, 8000 + ty)
    arr = cs.arrays()
    want = cs.model(arr)
    try:
        for opts in FORCED:
            for k, v in dict(PLANNED, **opts).items():
                K.eng.set_option(k, v)
            same(K.eng.simulate_batch(ty, cs.N, cs.m, cs.n, **arr), want, opts)
    finally:
        for k, v in PLANNED.items():
            K.eng.set_option(k, v)


@pytest.mark.parametrize("cid,cname", CURVES)
def test_kernel_names(cid, cname):
    K = sim(cid, cname)
    eng = K.eng
    cs = Case(K, MSMEG1, 2, 2, 3, 8500)
    arr = cs.arrays()
    eng.prof_enable(True)
    eng.prof_reset()
    try:
        eng.simulate_batch(MSMEG1, 2, 2, 3, **arr)
        eng.sync()
        names = [p[0] for p in eng.prof_get()]
    finally:
        eng.prof_enable(False)
    for want in ("k_prep_sim", "k_fix.sm1", "k_fix.sm2", "k_red.sm1", "k_red.sm2"):
        assert want in names, (want, names)
    assert any(nm.startswith("k_var") and nm.endswith(".sm1") for nm in names), names
    assert not any(nm.startswith("k_var") and nm.endswith(".sm2") for nm in names), names  # pi is fixed-base here


# ---- 9. key and status ----------------------------------------------------------------------------------------------------
def expect(code, fn, *a, **kw):
    import groth_sahai_rs_amd as gs

    with pytest.raises(gs.GsError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("cid,cname", CURVES)
def test_key_and_status(cid, cname):
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import _p

    K = sim(cid, cname)
    cs = Case(K, QUAD, 2, 2, 3, 9000)
    arr = cs.arrays()
    eng = gs.Engine(cid, 0)
    try:
        call = lambda: eng.simulate_batch(QUAD, 2, 2, 3, **arr)
        expect(4, eng.set_simulation_key, K.key)  # no CRS
        eng.set_crs(K.hiding)
        assert "gs_set_simulation_key" in expect(3, call)  # no key
        eng.set_simulation_key(K.key)
        good = call()
        same(good, K.eng.simulate_batch(QUAD, 2, 2, 3, **arr), "a second context")
        # a wrong t1 / t2 is refused with the check named, and the earlier key is gone
        for bad, who in (([K.t1 + 1, K.t2], "t1"), ([K.t1, K.t2 + 1], "t2")):
            assert who in expect(3, eng.set_simulation_key, K.frs(bad))
            expect(3, call)
            eng.set_simulation_key(K.key)
            call()
        # gs_set_crs forgets the key, also when the same CRS returns
        eng.set_crs(K.hiding)
        expect(3, call)
        eng.set_simulation_key(K.key)
        # a binding CRS is refused
        eng.set_crs(K.binding)
        msg = expect(3, eng.set_simulation_key, K.key)
        assert "binding" in msg and "t1" in msg, msg
        expect(3, call)
        eng.set_crs(K.hiding)
        eng.set_simulation_key(K.key)
        # PPE is refused, with the reason
        z = lambda nbytes: np.zeros(nbytes, np.uint8)
        msg = expect(3, eng.simulate_batch, 0, 1, 1, 1, z(eng.G1), z(eng.G2), z(32), z(eng.GT), z(64), z(64), z(128))
        assert "PPE" in msg and "identity witness" in msg, msg
        # N = 0 is a no-op
        out = eng.simulate_batch(QUAD, 0, 2, 3, *(z(0),) * 7)
        assert out["pi"].size == 0
        # short buffers are refused before the ABI is crossed
        expect(1, eng.simulate_batch, QUAD, 2, 2, 3, **dict(arr, Tf=arr["Tf"][:-1]))
        # host form: an output that overlaps an input or another output
        buf = np.zeros(good["pi"].size + good["theta"].size, np.uint8)
        lib, N = eng.lib, 2
        args = [_p(arr[k]) for k in ("A", "B", "Gamma", "target", "Rc", "Sc", "Tf")]
        import ctypes

        rc = lib.gs_simulate_batch(eng.ctx, QUAD, ctypes.c_size_t(N), 2, 3, *args, _p(None), _p(None), _p(buf),
                                   _p(buf[good["pi"].size - 1:]))
        assert rc == 3 and b"overlaps" in lib.gs_last_error(eng.ctx)
        rc = lib.gs_simulate_batch(eng.ctx, QUAD, ctypes.c_size_t(N), 2, 3, *args, _p(None), _p(None), _p(arr["Tf"]),
                                   _p(buf))
        assert rc == 3 and b"overlaps" in lib.gs_last_error(eng.ctx)
        # secret hygiene: after a call and gs_sync, clearing the key leaves nothing to simulate with
        call()
        eng.sync()
        eng.set_simulation_key(None)
        expect(3, call)
        eng.set_simulation_key(K.key)
        same(call(), good, "after the key came back")
    finally:
        eng.close()

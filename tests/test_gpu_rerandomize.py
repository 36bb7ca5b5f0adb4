"""gs_rerandomize_batch / gs_rerandomize_statement on the GPU (include/gs_amd.h): fresh commitments and proofs from old
ones without the witness.  The prover is the byte-level oracle: rerandomizing prove(X, Y, R, S, T) with (R', S', T')
must give exactly prove(X, Y, R + R', S + S', T + T' + S'^T Gamma^T R), commitments included; sampled equations are also
checked against the C restatement of the reference (oracle/gs_ref.c), and verdicts must be preserved."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gsutil import HERE, REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))

pytestmark = pytest.mark.gpu

CURVES = [(0, "bls12_381"), (1, "bn254")]
TYPES = [0, 1, 2, 3]
MASK = (1 << 64) - 1


# ---- host-side Fr bookkeeping on Montgomery limbs (vectorised over equations with object arrays) ----
def _ints(t, cols):
    """uint8 buffer of N x cols Montgomery scalars -> (N, cols) object array of ints (still Montgomery)"""
    a = np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint64).reshape(-1, cols, 4).astype(object)
    return a[..., 0] | (a[..., 1] << 64) | (a[..., 2] << 128) | (a[..., 3] << 192)


def _limbs(v):
    return np.stack([((v >> (64 * i)) & MASK).astype(np.uint64) for i in range(4)], axis=-1).reshape(-1).view(np.uint8)


def combined(eng, ty, N, m, n, R, S, T, R1, S1, T1, G, V=None):
    """R + R', S + S' and T'' = T + T' + S'^T Gamma^T R as Montgomery bytes (V = N: per equation; 1: shared R, S)."""
    import torch

    from groth_sahai_rs_amd.workload import CURVES as CV

    r = CV[eng.curve]["r"]
    sh = eng.shape(ty)
    kx, ky = sh["kx"], sh["ky"]
    V = N if V is None else V
    R0, R1i = _ints(R, m * kx).reshape(V, m, kx), _ints(R1, m * kx).reshape(V, m, kx)
    S0, S1i = _ints(S, n * ky).reshape(V, n, ky), _ints(S1, n * ky).reshape(V, n, ky)
    T0, T1i = _ints(T, ky * kx).reshape(N, ky, kx), _ints(T1, ky * kx).reshape(N, ky, kx)
    Gi = _ints(G, m * n).reshape(N, m, n)
    rinv2 = pow(1 << 256, -2, r)  # mont(a) mont(b) mont(c) / 2^512 = mont(abc)
    cross = np.zeros((N, ky, kx), dtype=object)
    for l in range(ky):
        for k in range(kx):
            acc = np.zeros(N, dtype=object)
            for i in range(m):
                for j in range(n):
                    acc = acc + S1i[:, j, l] * Gi[:, i, j] % r * R0[:, i, k]
            cross[:, l, k] = acc % r * rinv2 % r
    dev = lambda v: torch.from_numpy(_limbs(v % r).copy()).to("cuda:0")
    return dev(R0 + R1i), dev(S0 + S1i), dev(T0 + T1i + cross)


_DRAWS = [0]


def rand_like(wl, t):
    """fresh uniform scalars, as many as `t` holds (a new stream on every call)"""
    import torch

    from groth_sahai_rs_amd.workload import CURVES as CV

    r = CV[wl.eng.curve]["r"]
    cnt = t.numel() // 32
    _DRAWS[0] += 1
    g = np.random.default_rng(_DRAWS[0])
    v = np.array([int.from_bytes(g.bytes(32), "little") % r for _ in range(cnt)], dtype=object)
    return torch.from_numpy(_limbs(v).copy()).to("cuda:0")


def outs(eng, ty, N, m, n, V=None):
    import torch

    sh = eng.shape(ty)
    V = N if V is None else V
    e = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda:0")
    return [e(V * m * eng.COM1), e(V * n * eng.COM2), e(N * sh["kx"] * eng.COM2), e(N * sh["ky"] * eng.COM1)]


def rerand(wl, R1, S1, T1, src=None, o=None):
    src = src or (wl.xcoms, wl.ycoms, wl.pi, wl.theta)
    o = o or outs(wl.eng, wl.ty, wl.N, wl.m, wl.n)
    wl.eng.rerandomize_batch_dev(wl.ty, wl.N, wl.m, wl.n, wl.A, wl.B, wl.Gamma, *src, R1, S1, T1, *o)
    wl.eng.sync()
    return o


def prove_with(wl, R, S, T):
    o = outs(wl.eng, wl.ty, wl.N, wl.m, wl.n)
    wl.eng.prove_batch_dev(wl.ty, wl.N, wl.m, wl.n, wl.X, wl.Y, wl.A, wl.B, wl.Gamma, R, S, T, *o)
    wl.eng.sync()
    return o


def same(a, b):
    return all((x.cpu().numpy() == y.cpu().numpy()).all() for x, y in zip(a, b))


_ENG = {}


def engine(cid):
    import groth_sahai_rs_amd as gs

    if cid not in _ENG:
        _ENG[cid] = gs.Engine(cid, 0)
    return _ENG[cid]


def workload(cid, ty, N, m, n, seed=4242, corrupt_every=0):
    from groth_sahai_rs_amd.workload import Workload

    wl = Workload(engine(cid), ty=ty, N=N, m=m, n=n, seed=seed + ty, corrupt_every=corrupt_every)
    wl.prove()
    wl.eng.sync()
    return wl


def fresh(wl):
    return rand_like(wl, wl.R), rand_like(wl, wl.S), rand_like(wl, wl.T)


def check_identity(wl, sample=()):
    """rerandomize(prove(R, S, T), R', S', T') == prove(R + R', S + S', T''), and sampled equations == the C oracle"""
    import gs_ref_py as ref

    R1, S1, T1 = fresh(wl)
    got = rerand(wl, R1, S1, T1)
    R2, S2, T2 = combined(wl.eng, wl.ty, wl.N, wl.m, wl.n, wl.R, wl.S, wl.T, R1, S1, T1, wl.Gamma)
    want = prove_with(wl, R2, S2, T2)
    for name, g, w in zip(("xcoms", "ycoms", "pi", "theta"), got, want):
        bad = np.nonzero((g.cpu().numpy() != w.cpu().numpy()))[0]
        assert bad.size == 0, (name, wl.ty, wl.m, wl.n, bad[:4])
    eng, m, n, sh = wl.eng, wl.m, wl.n, wl.sh
    kx, ky, sx, sy = sh["kx"], sh["ky"], sh["sx"], sh["sy"]
    host = lambda t: t.cpu().numpy()
    X, Y, A, B, G, R2h, S2h, T2h = map(host, (wl.X, wl.Y, wl.A, wl.B, wl.Gamma, R2, S2, T2))
    cut = lambda a, e, sz: a[e * sz:(e + 1) * sz]
    cname = "bls12_381" if eng.curve == 0 else "bn254"
    for e in sample:
        o = ref.commit_and_prove(cname, wl.ty, m, n, cut(X, e, m * sx), cut(Y, e, n * sy), cut(A, e, n * sx),
                                 cut(B, e, m * sy), cut(G, e, m * n * 32), cut(R2h, e, m * kx * 32),
                                 cut(S2h, e, n * ky * 32), cut(T2h, e, ky * kx * 32), wl.crs)
        for name, g, per in (("xcoms", got[0], m * eng.COM1), ("ycoms", got[1], n * eng.COM2),
                             ("pi", got[2], kx * eng.COM2), ("theta", got[3], ky * eng.COM1)):
            assert (o[name] == cut(host(g), e, per)).all(), ("oracle", name, e)
    return got, (R1, S1, T1), (R2, S2, T2)


# 1. fresh-proof identity, all four types, both curves
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (7, 5), (2, 9)])
def test_fresh_proof_identity(cid, cname, ty, shape):
    wl = workload(cid, ty, 64, *shape)
    check_identity(wl, sample=(0, 37, 63))


# 2. verdict preserved; 3. zero randomness is the identity; 4. composition
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_verdicts_zero_and_composition(cid, cname, ty):
    import torch

    wl = workload(cid, ty, 64, 3, 2)
    eng, N = wl.eng, wl.N
    # honest: all verify, RLC passes
    got, r1, comb = check_identity(wl)
    ok = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    eng.verify_batch_dev(wl.ty, N, wl.m, wl.n, wl.A, wl.B, wl.Gamma, wl.target, *got, ok)
    eng.sync()
    assert ok.cpu().numpy().all()
    keep = (wl.xcoms, wl.ycoms, wl.pi, wl.theta)
    wl.xcoms, wl.ycoms, wl.pi, wl.theta = got
    assert eng.gt_finalize(wl.verify_rlc().cpu().numpy()) == 1
    wl.xcoms, wl.ycoms, wl.pi, wl.theta = keep
    # zero randomness returns the inputs byte for byte
    z = [torch.zeros_like(t) for t in (wl.R, wl.S, wl.T)]
    assert same(rerand(wl, *z), keep)
    # composition: two in a row == one prove with the accumulated randomness (the T update carries the cross term)
    R3, S3, T3 = fresh(wl)
    twice = rerand(wl, R3, S3, T3, src=got)
    R4, S4, T4 = combined(eng, wl.ty, N, wl.m, wl.n, *comb, R3, S3, T3, wl.Gamma)
    assert same(twice, prove_with(wl, R4, S4, T4))
    # corrupt every 8th proof with a valid but wrong element (pi of the previous equation)
    stride = wl.sh["kx"] * eng.COM2
    pi_bad = wl.pi.clone()
    bad = list(range(7, N, 8))
    for e in bad:
        pi_bad[e * stride:(e + 1) * stride] = wl.pi[(e - 1) * stride:e * stride]
    o = rerand(wl, *fresh(wl), src=(wl.xcoms, wl.ycoms, pi_bad, wl.theta))
    eng.verify_batch_dev(wl.ty, N, wl.m, wl.n, wl.A, wl.B, wl.Gamma, wl.target, *o, ok)
    eng.sync()
    want = np.ones(N, dtype=np.uint8)
    want[bad] = 0
    assert (ok.cpu().numpy() == want).all()
    wl.xcoms, wl.ycoms, wl.pi, wl.theta = o
    assert eng.gt_finalize(wl.verify_rlc().cpu().numpy()) == 0


# 5. Statement form, and a mixed-type Statement from four single-type calls over the same variable groups
@pytest.mark.parametrize("cid,cname", CURVES)
def test_statement(cid, cname):
    import torch

    from stmtutil import StatementInputs

    eng = engine(cid)
    si = StatementInputs(eng, mg=3, ng=2, ms=2, ns=3, seed=777)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    fresh_rand = {g: si.fr(si.scalars(cnt)) for g, cnt in (("xg", 6), ("yg", 4), ("xs", 2), ("ys", 3))}
    new_coms = {}
    for ty, E in ((0, 16), (1, 4), (2, 4), (3, 4)):
        p = si.part(ty, E)
        gx, gy = si.groups(ty)
        m, n = p["m"], p["n"]
        X, Y, A, B, G, R, S, T = map(dev, (p["X"], p["Y"], p["A"], p["B"], p["Gamma"], p["R"], p["S"], p["T"]))
        old = outs(eng, ty, E, m, n, V=1)
        eng.lib.gs_prove_statement_dev(eng.ctx, ty, ctypes.c_size_t(E), m, n, *[ctypes.c_void_p(t.data_ptr()) for t in
                                       (X, Y, A, B, G, R, S, T, *old)])
        eng.sync()
        # ONE R' for the x group and ONE S' for the y group: the same fresh values for every type that uses the group
        R1, S1 = dev(fresh_rand[gx]), dev(fresh_rand[gy])
        sh = eng.shape(ty)
        T1 = dev(si.fr(si.scalars(E * sh["ky"] * sh["kx"])))
        new = outs(eng, ty, E, m, n, V=1)
        eng.rerandomize_statement_dev(ty, E, m, n, A, B, G, *old, R1, S1, T1, *new)
        eng.sync()
        # against gs_prove_statement(X, Y, R + R', S + S', T''_e)
        R2, S2, T2 = combined(eng, ty, E, m, n, R, S, T, R1, S1, T1, G, V=1)
        want = outs(eng, ty, E, m, n, V=1)
        eng.lib.gs_prove_statement_dev(eng.ctx, ty, ctypes.c_size_t(E), m, n, *[ctypes.c_void_p(t.data_ptr()) for t in
                                       (X, Y, A, B, G, R2, S2, T2, *want)])
        eng.sync()
        assert same(new, want), ty
        # the host form gives the same bytes, and the statement verifies
        h = eng.rerandomize_statement(ty, E, m, n, p["A"], p["B"], p["Gamma"], *[t.cpu().numpy() for t in old],
                                      fresh_rand[gx], fresh_rand[gy], T1.cpu().numpy())
        for k, t in zip(("xcoms", "ycoms", "pi", "theta"), new):
            assert (h[k] == t.cpu().numpy()).all(), (ty, k)
        ok = eng.verify_statement(ty, E, m, n, p["A"], p["B"], p["Gamma"], p["target"], h["xcoms"], h["ycoms"], h["pi"],
                                  h["theta"])
        assert ok.all(), ty
        # the x group's new commitments are the same whichever type's call made them
        # a group's new commitments are the same whichever type's call made them: the four calls together are the
        # rerandomization of one mixed-type Statement over the groups xg, yg, xs, ys
        assert (new_coms.setdefault(gx, h["xcoms"]) == h["xcoms"]).all()
        assert (new_coms.setdefault(gy, h["ycoms"]) == h["ycoms"]).all()


# 6. edge values: identity points in X, A, B; zero rows of R' / S'; a commitment component equal to O
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
def test_edge_values(cid, cname, ty):
    wl = workload(cid, ty, 64, 3, 3)
    eng, sh = wl.eng, wl.sh
    sx, sy, kx, ky = sh["sx"], sh["sy"], sh["kx"], sh["ky"]
    for e in range(0, wl.N, 3):  # identities / zero scalars in X (variable 0), A (constant 1), B (constant 2)
        wl.X[e * 3 * sx:(e * 3 + 1) * sx] = 0
        wl.A[(e * 3 + 1) * sx:(e * 3 + 2) * sx] = 0
        wl.B[(e * 3 + 2) * sy:(e * 3 + 3) * sy] = 0
        wl.R[e * 3 * kx * 32:(e * 3 + 1) * kx * 32] = 0  # with X_0 = O: commitment 0 is (O, O)
    wl.prove()
    eng.sync()
    assert not wl.xcoms[:eng.COM1].any()
    R1, S1, T1 = fresh(wl)
    for e in range(0, wl.N, 2):  # zero rows of R' / S'
        R1[(e * 3 + 1) * kx * 32:(e * 3 + 2) * kx * 32] = 0
        S1[e * 3 * ky * 32:(e * 3 + 1) * ky * 32] = 0
    got = rerand(wl, R1, S1, T1)
    R2, S2, T2 = combined(eng, ty, wl.N, 3, 3, wl.R, wl.S, wl.T, R1, S1, T1, wl.Gamma)
    assert same(got, prove_with(wl, R2, S2, T2))


# 7. large arity: the wide preparation path and the tree folds
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty,m,n", [(0, 40, 33), (1, 33, 32), (2, 33, 32), (3, 33, 32)])
def test_large_arity(cid, cname, ty, m, n):
    wl = workload(cid, ty, 2, m, n)
    check_identity(wl, sample=(1,))


# 8. entry points agree: host and _dev; endo = 0 and endo = 1
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", [0, 3])
def test_entry_points_agree(cid, cname, ty):
    wl = workload(cid, ty, 64, 4, 4)
    eng = wl.eng
    R1, S1, T1 = fresh(wl)
    dev = rerand(wl, R1, S1, T1)
    host = lambda t: t.cpu().numpy()
    h = eng.rerandomize_batch(ty, wl.N, 4, 4, *map(host, (wl.A, wl.B, wl.Gamma, wl.xcoms, wl.ycoms, wl.pi, wl.theta,
                                                          R1, S1, T1)))
    for k, t in zip(("xcoms", "ycoms", "pi", "theta"), dev):
        assert (h[k] == host(t)).all(), k
    eng.set_option("endo", 0)
    try:
        plain = rerand(wl, R1, S1, T1)
    finally:
        eng.set_option("endo", 1)
    assert same(plain, dev)


# 9. full size: 2^16 PPE 4x4, the whole batch against prove with the combined randomness, all verify
def test_full_size_ppe():
    import torch

    wl = workload(0, 0, 1 << 16, 4, 4, seed=2024)
    got, _, _ = check_identity(wl, sample=(0, 12345, 65535))
    ok = torch.empty(wl.N, dtype=torch.uint8, device="cuda:0")
    wl.eng.verify_batch_dev(0, wl.N, 4, 4, wl.A, wl.B, wl.Gamma, wl.target, *got, ok)
    wl.eng.sync()
    assert int(ok.sum()) == wl.N


# 10. mirror and C++ layers
class _Rng:
    def __init__(self, vals):
        self.q, self.i = list(vals), 0

    def fr(self):
        self.i += 1
        return self.q[self.i - 1]


@pytest.mark.parametrize("cid,cname", CURVES)
def test_mirror_rerandomize(cid, cname):
    import groth_sahai_rs_amd.mirror as M

    c = curve(cname)
    g = c.golden["crs"]
    crs = M.CRS([c.com1(g["u"][0]), c.com1(g["u"][1])], [c.com2(g["v"][0]), c.com2(g["v"][1])], c.g1(g["g1"]),
                c.g2(g["g2"]), c.f12(g["gt"]), cid)
    case = c.golden["cases"][4]  # PPE dense 2x2
    equ = M.PPE([c.g1(v) for v in case["a"]], [c.g2(v) for v in case["b"]],
                [[c.fr_hex(s) for s in row] for row in case["gamma"]], c.f12(case["target"]))
    X, Y = [c.g1(v) for v in case["xvars"]], [c.g2(v) for v in case["yvars"]]
    draws = [c.fr(v) for v in range(1000, 1100)]
    proof = equ.commit_and_prove(X, Y, crs, _Rng(draws))
    assert equ.verify(proof, crs)
    rng = _Rng([c.fr(3 ** k + 11) for k in range(1, 40)])
    q = M.rerandomize(equ, proof, crs, rng)
    assert rng.i == 2 * 2 + 2 * 2 + 2 * 2  # R', S', T'
    assert equ.verify(q, crs)
    assert not all((a == b).all() for a, b in zip(q.xcoms.coms, proof.xcoms.coms))
    flat = [v for M_ in (q.xcoms.rand, q.ycoms.rand, q.equ_proofs[0].rand) for row in M_ for v in row]
    again = equ.commit_and_prove(X, Y, crs, _Rng(flat))
    assert q.xcoms == again.xcoms and q.ycoms == again.ycoms
    assert all((a == b).all() for a, b in zip(q.equ_proofs[0].pi, again.equ_proofs[0].pi))
    assert all((a == b).all() for a, b in zip(q.equ_proofs[0].theta, again.equ_proofs[0].theta))
    crs.engine.close()


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_cpp_rerandomize(name, tmp_path):
    from test_gpu_cpp_host import BUILD, LIBDIR, write_case

    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_rerandomize")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(HERE, "cpp", "test_rerandomize.cpp"), "-o", exe, "-L" + LIBDIR, "-lgs_amd",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    c = curve(name)
    for case in c.golden["cases"][4:8]:  # dense 2x2, all four types
        p = str(tmp_path / (case["name"] + ".bin"))
        write_case(c, case, p)
        r = subprocess.run([exe, p], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (case["name"], r.stdout, r.stderr)


# 11. errors
def test_errors():
    wl = workload(0, 0, 4, 2, 2)
    eng, lib = wl.eng, wl.eng.lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o = outs(eng, 0, 4, 2, 2)
    ins = [p(t) for t in (wl.A, wl.B, wl.Gamma, wl.xcoms, wl.ycoms, wl.pi, wl.theta, wl.R, wl.S, wl.T)]
    call = lambda fn, ty, N, m, n, outs_: fn(eng.ctx, ty, ctypes.c_size_t(N), m, n, *ins, *outs_)
    for fn in (lib.gs_rerandomize_batch_dev, lib.gs_rerandomize_statement_dev):
        assert call(fn, 7, 4, 2, 2, [p(t) for t in o]) == 3  # GS_ERR_ARG
        assert call(fn, 0, 4, 0, 2, [p(t) for t in o]) == 1  # GS_ERR_SHAPE
        assert call(fn, 0, 4, 2, 0, [p(t) for t in o]) == 1
        assert call(fn, 0, 0, 2, 2, [p(t) for t in o]) == 0  # N = 0: no-op
    # host form: an output overlapping an input
    host = [t.cpu().numpy() for t in (wl.A, wl.B, wl.Gamma, wl.xcoms, wl.ycoms, wl.pi, wl.theta, wl.R, wl.S, wl.T)]
    hin = [ctypes.c_void_p(a.ctypes.data) for a in host]
    hout = [np.zeros(t.numel(), dtype=np.uint8) for t in o]
    houts = [ctypes.c_void_p(a.ctypes.data) for a in hout]
    rc = lib.gs_rerandomize_batch(eng.ctx, 0, ctypes.c_size_t(4), 2, 2, *hin, hin[5], *houts[1:])
    assert rc == 3  # xcoms_out = pi
    assert lib.gs_rerandomize_batch(eng.ctx, 0, ctypes.c_size_t(4), 2, 2, *hin, *houts) == 0
    assert lib.gs_rerandomize_batch(eng.ctx, 7, ctypes.c_size_t(4), 2, 2, *hin, *houts) == 3
    assert lib.gs_rerandomize_batch(eng.ctx, 0, ctypes.c_size_t(0), 2, 2, *hin, *houts) == 0

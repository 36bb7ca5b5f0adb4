"""The device generator and the drawn entries on the GPU (include/gs_amd.h, "randomness drawn on the device").
gs_rand_fr / gs_rand_rho against the Python model of tests/randvec.py (itself held against OpenSSL and RFC 8439 by
tests/test_rand_cpu.py); the drawn forms of prove and rerandomize against their siblings fed with the model's draws,
byte for byte."""
import ctypes

import numpy as np
import pytest

import randvec as rv
from gsutil import curve

pytestmark = pytest.mark.gpu

CURVES = [(0, "bls12_381"), (1, "bn254")]
TYPES = [0, 1, 2, 3]
M, N_ = 2, 3  # m x n of every drawn test: not square, so a swapped layout shows
TWO32 = 1 << 32

_ENG = {}


def engine(cid):
    import groth_sahai_rs_amd as gs

    if cid not in _ENG:
        _ENG[cid] = gs.Engine(cid, 0)
    return _ENG[cid]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def empty(nbytes, fill=None):
    import torch

    if fill is None:
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda:0")


def host(t):
    return t.cpu().numpy()


_MODEL = {}


def model_fr(key, r, domain, stream, first, count):
    k = (key, r, domain, stream, first, count)
    if k not in _MODEL:
        _MODEL[k] = rv.rand_fr(key, r, domain, stream, first, count).reshape(-1).view(np.uint8)
    return _MODEL[k]


def fr_dev(eng, domain, stream, first, count):
    out = empty(count * 32)
    eng.rand_fr_dev(domain, stream, first, count, out)
    eng.sync()
    return host(out)


# ---- gs_rand_fr[_dev] against the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_rand_fr_model(cid, cname):
    eng, r = engine(cid), curve(cname).r
    eng.rand_set_key(rv.KEY_TEST)
    dom = rv.USER + 7
    for count in (1, 63, 64, 65, 257):
        want = model_fr(rv.KEY_TEST, r, dom, 0, 0, count)
        assert (eng.rand_fr(dom, 0, 0, count) == want).all(), ("host", count)
        assert (fr_dev(eng, dom, 0, 0, count) == want).all(), ("dev", count)
    # the last legal counter, the largest stream, a library domain
    for domain, stream, first, count in ((dom, 0, TWO32 - 65, 65), (dom, rv.STREAM_MAX, 0, 65),
                                         (rv.PROVE_S, rv.STREAM_MAX, TWO32 - 65, 65), (rv.RERAND_T, 3, 0, 9)):
        want = model_fr(rv.KEY_TEST, r, domain, stream, first, count)
        assert (eng.rand_fr(domain, stream, first, count) == want).all(), (domain, stream, first)
        assert (fr_dev(eng, domain, stream, first, count) == want).all(), (domain, stream, first)
    # a slice of a draw is the draw of the slice
    whole = fr_dev(eng, dom, 5, 0, 257)
    assert (np.concatenate([fr_dev(eng, dom, 5, 0, 100), fr_dev(eng, dom, 5, 100, 157)]) == whole).all()
    assert (whole == model_fr(rv.KEY_TEST, r, dom, 5, 0, 257)).all()
    # streams and domains separate
    assert (fr_dev(eng, dom, 6, 0, 4) != whole[:128]).any() and (fr_dev(eng, dom + 1, 5, 0, 4) != whole[:128]).any()
    # other keys: all ones, and the RFC 8439 section 2.3.2 block
    eng.rand_set_key(rv.KEY_ONES)
    assert (eng.rand_fr(dom, 1, 0, 65) == model_fr(rv.KEY_ONES, r, dom, 1, 0, 65)).all()
    eng.rand_set_key(rv.KEY_RFC)
    got = eng.rand_fr(rv.RFC_DOMAIN, rv.RFC_STREAM, rv.RFC_FIRST, 1)
    assert curve(cname).fr_dec(got.view(np.uint64)) == int.from_bytes(bytes.fromhex(rv.RFC_BLOCK_HEX), "little") % r
    eng.rand_set_key(None)


# ---- gs_rand_rho[_dev] against the model ---------------------------------------------------------------------------
def test_rand_rho_model():
    eng = engine(0)
    eng.rand_set_key(rv.KEY_TEST)
    cases = [(0, 0, c) for c in (1, 7, 8, 9, 513)] + [(2, 5, c) for c in (1, 7, 8, 9, 513)] + \
            [(rv.STREAM_MAX, 8 * (TWO32 - 1), 8), (1, 8 * (TWO32 - 1) + 3, 5), (1, 3, 2)]
    for stream, first, count in cases:
        want = rv.rand_rho(rv.KEY_TEST, stream, first, count)
        got = eng.rand_rho(stream, first, count)
        assert (got == want).all() and (got != 0).all(), ("host", stream, first, count)
        out = empty(count * 8 + 16, 0xAB)  # (16 guard bytes behind the partial last block)
        eng.rand_rho_dev(stream, first, count, out[:count * 8])
        eng.sync()
        o = host(out)
        assert (o[:count * 8].view(np.uint64) == want).all(), ("dev", stream, first, count)
        assert (o[count * 8:] == 0xAB).all(), "wrote past the end"
    eng.rand_set_key(None)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    from groth_sahai_rs_amd.capi import GsError

    eng, lib = engine(0), engine(0).lib
    eng.rand_set_key(None)
    out = empty(65 * 32, 0xAB)
    hout = np.full(65 * 32, 0xAB, dtype=np.uint8)
    p, hp = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(hout.ctypes.data)
    # no key
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, 0, 4, p) == 3
    assert lib.gs_rand_fr(eng.ctx, rv.USER, 0, 0, 4, hp) == 3
    assert lib.gs_rand_rho_dev(eng.ctx, 0, 0, 4, p) == 3
    assert lib.gs_rand_rho(eng.ctx, 0, 0, 4, hp) == 3
    with pytest.raises(GsError) as e:
        eng.rand_fr(rv.USER, 0, 0, 4)
    assert e.value.code == 3
    eng.rand_set_key(rv.KEY_TEST)
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, 0, 4, p) == 0
    eng.sync()
    assert (host(out)[:128] == model_fr(rv.KEY_TEST, curve("bls12_381").r, rv.USER, 0, 0, 4)).all()
    # after the key is forgotten
    eng.rand_set_key(None)
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, 0, 4, p) == 3
    assert lib.gs_rand_rho(eng.ctx, 0, 0, 4, hp) == 3
    eng.rand_set_key(rv.KEY_TEST)
    # the counter never wraps: first + count = 2^32 + 1, and nothing is written
    out.fill_(0xAB)
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, TWO32 - 64, 65, p) == 1
    assert lib.gs_rand_fr(eng.ctx, rv.USER, 0, TWO32 - 64, 65, hp) == 1
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, TWO32 + 1, 0, p) == 1
    assert lib.gs_rand_rho_dev(eng.ctx, 0, 8 * TWO32 - 7, 8, p) == 1
    assert lib.gs_rand_rho(eng.ctx, 0, 8 * TWO32 - 7, 8, hp) == 1
    assert lib.gs_rand_rho_dev(eng.ctx, 0, (1 << 64) - 1, 8, p) == 1  # first + count itself would wrap
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, TWO32 - 65, 65, p) == 0  # (the largest legal draw does run)
    eng.sync()
    out.fill_(0xAB)
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, TWO32 - 64, 65, p) == 1
    eng.sync()
    assert (host(out) == 0xAB).all() and (hout == 0xAB).all()
    # count = 0 is a no-op (null pointers included); a null output otherwise is refused
    for fn, args in ((lib.gs_rand_fr_dev, (rv.USER, 0, 0)), (lib.gs_rand_fr, (rv.USER, 0, 0)),
                     (lib.gs_rand_rho_dev, (0, 0)), (lib.gs_rand_rho, (0, 0))):
        assert fn(eng.ctx, *args, 0, None) == 0
        assert fn(eng.ctx, *args, 4, None) == 3
    assert lib.gs_rand_fr_dev(eng.ctx, rv.USER, 0, TWO32, 0, p) == 0
    eng.sync()
    assert (host(out) == 0xAB).all()
    # the key must be 32 bytes (binding), and gs_set_crs leaves it alone (checked in test_drawn_prove: the key is
    # installed before the workload installs its CRS)
    with pytest.raises(GsError):
        eng.rand_set_key(b"short")
    eng.rand_set_key(None)


# ---- drawn prove ---------------------------------------------------------------------------------------------------
def workload(cid, ty, N, seed=977):
    from groth_sahai_rs_amd.workload import Workload

    wl = Workload(engine(cid), ty=ty, N=N, m=M, n=N_, seed=seed + ty, corrupt_every=0)
    wl.eng.sync()
    return wl


def outs(eng, ty, N, V=None):
    sh = eng.shape(ty)
    V = N if V is None else V
    return [empty(V * M * eng.COM1), empty(V * N_ * eng.COM2), empty(N * sh["kx"] * eng.COM2),
            empty(N * sh["ky"] * eng.COM1)]


def same(a, b):
    return all((host(x) == host(y)).all() for x, y in zip(a, b))


def verify_all(wl, o):
    ok = empty(wl.N)
    wl.eng.verify_batch_dev(wl.ty, wl.N, M, N_, wl.A, wl.B, wl.Gamma, wl.target, *o, ok)
    wl.eng.sync()
    return host(ok)


@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("N", [1, 65])
def test_drawn_prove(cid, cname, ty, N):
    import groth_sahai_rs_amd as gs

    eng, r = engine(cid), curve(cname).r
    eng.rand_set_key(rv.KEY_TEST)  # before the workload's gs_set_crs: the key is not tied to the CRS
    wl = workload(cid, ty, N)
    ins = (wl.X, wl.Y, wl.A, wl.B, wl.Gamma)
    stream = 11 + ty
    mR, mS, mT = (a.view(np.uint8) for a in rv.drawn_rst(rv.KEY_TEST, r, ty, N, M, N_, stream))
    # the definition: three gs_rand_fr_dev calls, then gs_prove_batch_dev
    rst = [empty(a.size) for a in (mR, mS, mT)]
    for t, d in zip(rst, (rv.PROVE_R, rv.PROVE_S, rv.PROVE_T)):
        eng.rand_fr_dev(d, stream, 0, t.numel() // 32, t)
    want = outs(eng, ty, N)
    eng.prove_batch_dev(ty, N, M, N_, *ins, *rst, *want)
    got, back = outs(eng, ty, N), [empty(a.size) for a in (mR, mS, mT)]
    eng.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream, *back, *got)
    eng.sync()
    assert same(got, want)
    for name, t, t2, mdl in zip("RST", back, rst, (mR, mS, mT)):
        assert (host(t) == mdl).all() and (host(t2) == mdl).all(), name
    # the same bytes with R_out = S_out = T_out = NULL, and with only one of them asked for
    got2 = outs(eng, ty, N)
    eng.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream, None, None, None, *got2)
    got3, s_only = outs(eng, ty, N), empty(mS.size)
    eng.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream, None, s_only, None, *got3)
    eng.sync()
    assert same(got2, want) and same(got3, want) and (host(s_only) == mS).all()
    # the host form
    h = eng.prove_batch_drawn(ty, N, M, N_, *map(host, ins), stream)
    for k, t in zip(("xcoms", "ycoms", "pi", "theta", "R", "S", "T"), want + rst):
        assert (h[k] == host(t)).all(), ("host", k)
    h2 = eng.prove_batch_drawn(ty, N, M, N_, *map(host, ins), stream, want_rand=False)
    assert h2["R"] is None and all((h2[k] == h[k]).all() for k in ("xcoms", "ycoms", "pi", "theta"))
    # it verifies; another stream gives other proofs
    assert verify_all(wl, got).all()
    other = outs(eng, ty, N)
    eng.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream + 100, None, None, None, *other)
    eng.sync()
    assert all((host(a) != host(b)).any() for a, b in zip(other, want))
    assert verify_all(wl, other).all()
    # the same stream in a fresh context, after unrelated calls, gives the same bytes
    e2 = gs.Engine(cid, 0)
    try:
        e2.set_crs(wl.crs)
        e2.rand_set_key(rv.KEY_TEST)
        e2.rand_fr(rv.USER, 1, 0, 33)
        e2.rand_rho(4, 3, 10)
        scratch_out = outs(e2, ty, N)
        e2.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream + 1, None, None, None, *scratch_out)
        again = outs(e2, ty, N)
        e2.prove_batch_drawn_dev(ty, N, M, N_, *ins, stream, None, None, None, *again)
        e2.sync()
        assert same(again, want)
    finally:
        e2.close()
    eng.rand_set_key(None)


def test_drawn_refusals():
    eng, lib = engine(0), engine(0).lib
    eng.rand_set_key(None)
    wl = workload(0, 0, 4)
    ins = (wl.X, wl.Y, wl.A, wl.B, wl.Gamma)
    o = outs(eng, 0, 4)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    call = lambda ty, N, m, n: lib.gs_prove_batch_drawn_dev(eng.ctx, ty, N, m, n, *map(p, ins), 0, None, None, None,
                                                            *map(p, o))
    assert call(0, 4, M, N_) == 3  # no key
    eng.rand_set_key(rv.KEY_TEST)
    assert call(0, 4, M, N_) == 0
    assert call(7, 4, M, N_) == 3 and call(0, 4, 0, N_) == 1 and call(0, 0, M, N_) == 0
    eng.sync()
    # host form: an output overlapping an input or another output
    hin = [host(t) for t in ins]
    hp = [ctypes.c_void_p(a.ctypes.data) for a in hin]
    ho = [np.zeros(t.numel(), dtype=np.uint8) for t in o]
    hop = [ctypes.c_void_p(a.ctypes.data) for a in ho]
    rbuf = np.zeros(4 * M * 2 * 32, dtype=np.uint8)
    rp = ctypes.c_void_p(rbuf.ctypes.data)
    f = lib.gs_prove_batch_drawn
    assert f(eng.ctx, 0, 4, M, N_, *hp, 0, rp, None, None, *hop) == 0
    assert f(eng.ctx, 0, 4, M, N_, *hp, 0, hop[2], None, None, *hop) == 3  # R_out = pi
    assert f(eng.ctx, 0, 4, M, N_, *hp, 0, hp[4], None, None, *hop) == 3  # R_out = Gamma
    assert f(eng.ctx, 0, 4, M, N_, *hp, 0, rp, None, rp, *hop) == 3  # R_out = T_out
    eng.rand_set_key(None)
    assert f(eng.ctx, 0, 4, M, N_, *hp, 0, rp, None, None, *hop) == 3


# ---- drawn statement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_drawn_statement(cid, cname):
    from stmtutil import StatementInputs

    eng, r = engine(cid), curve(cname).r
    eng.rand_set_key(rv.KEY_TEST)
    si = StatementInputs(eng, mg=M, ng=N_, ms=M, ns=N_, seed=779)
    E = 3
    for ty in TYPES:
        p = si.part(ty, E)
        assert (p["m"], p["n"]) == (M, N_)
        ins = [dev(p[k]) for k in ("X", "Y", "A", "B", "Gamma")]
        stream = 40 + ty
        mR, mS, mT = (dev(a) for a in rv.drawn_rst(rv.KEY_TEST, r, ty, E, M, N_, stream, shared=True))
        sh = eng.shape(ty)
        assert mR.numel() == M * sh["kx"] * 32 and mS.numel() == N_ * sh["ky"] * 32  # R, S: ONE copy
        want = outs(eng, ty, E, V=1)
        eng.lib.gs_prove_statement_dev(eng.ctx, ty, ctypes.c_size_t(E), M, N_,
                                       *[ctypes.c_void_p(t.data_ptr()) for t in (*ins, mR, mS, mT, *want)])
        got, back = outs(eng, ty, E, V=1), [empty(t.numel()) for t in (mR, mS, mT)]
        eng.prove_statement_drawn_dev(ty, E, M, N_, *ins, stream, *back, *got)
        got2 = outs(eng, ty, E, V=1)
        eng.prove_statement_drawn_dev(ty, E, M, N_, *ins, stream, None, None, None, *got2)
        eng.sync()
        assert same(got, want) and same(got2, want), ty
        assert same(back, (mR, mS, mT)), ty
        h = eng.prove_statement_drawn(ty, E, M, N_, *[p[k] for k in ("X", "Y", "A", "B", "Gamma")], stream)
        for k, t in zip(("xcoms", "ycoms", "pi", "theta", "R", "S", "T"), want + [mR, mS, mT]):
            assert (h[k] == host(t)).all(), (ty, k)
        assert eng.verify_statement(ty, E, M, N_, p["A"], p["B"], p["Gamma"], p["target"], h["xcoms"], h["ycoms"],
                                    h["pi"], h["theta"]).all(), ty
        # rerandomize the statement: against gs_rerandomize_statement_dev on the model's RERAND draws
        rR, rS, rT = (dev(a) for a in rv.drawn_rst(rv.KEY_TEST, r, ty, E, M, N_, stream, shared=True, rerand=True))
        a3 = ins[2:]
        rwant = outs(eng, ty, E, V=1)
        eng.rerandomize_statement_dev(ty, E, M, N_, *a3, *want, rR, rS, rT, *rwant)
        rgot, rback = outs(eng, ty, E, V=1), [empty(t.numel()) for t in (rR, rS, rT)]
        eng.rerandomize_statement_drawn_dev(ty, E, M, N_, *a3, *want, stream, *rback, *rgot)
        eng.sync()
        assert same(rgot, rwant) and same(rback, (rR, rS, rT)), ty
        hr = eng.rerandomize_statement_drawn(ty, E, M, N_, p["A"], p["B"], p["Gamma"], *[host(t) for t in want], stream,
                                             want_rand=False)
        for k, t in zip(("xcoms", "ycoms", "pi", "theta"), rwant):
            assert (hr[k] == host(t)).all(), (ty, k)
        assert eng.verify_statement(ty, E, M, N_, p["A"], p["B"], p["Gamma"], p["target"], hr["xcoms"], hr["ycoms"],
                                    hr["pi"], hr["theta"]).all(), ty
    eng.rand_set_key(None)


# ---- drawn rerandomize ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("N", [1, 65])
def test_drawn_rerandomize(cid, cname, ty, N):
    eng, r = engine(cid), curve(cname).r
    eng.rand_set_key(rv.KEY_ONES)
    wl = workload(cid, ty, N)
    wl.prove()
    eng.sync()
    consts = (wl.A, wl.B, wl.Gamma)
    stream = rv.STREAM_MAX - ty
    mdl = [dev(a) for a in rv.drawn_rst(rv.KEY_ONES, r, ty, N, M, N_, stream, rerand=True)]
    valid = (wl.xcoms, wl.ycoms, wl.pi, wl.theta)
    # forged: a well-formed but wrong first pi element (the first y-commitment of the same equation) in every third proof
    pi_bad = wl.pi.clone()
    ps, ys = wl.sh["kx"] * eng.COM2, N_ * eng.COM2
    bad = list(range(0, N, 3))
    for e in bad:
        pi_bad[e * ps:e * ps + eng.COM2] = wl.ycoms[e * ys:e * ys + eng.COM2]
    forged = (wl.xcoms, wl.ycoms, pi_bad, wl.theta)
    verdict = np.ones(N, dtype=np.uint8)
    verdict[bad] = 0
    assert (verify_all(wl, forged) == verdict).all()
    for src, expect in ((valid, np.ones(N, dtype=np.uint8)), (forged, verdict)):
        want = outs(eng, ty, N)
        eng.rerandomize_batch_dev(ty, N, M, N_, *consts, *src, *mdl, *want)
        got, back = outs(eng, ty, N), [empty(t.numel()) for t in mdl]
        eng.rerandomize_batch_drawn_dev(ty, N, M, N_, *consts, *src, stream, *back, *got)
        got2 = outs(eng, ty, N)
        eng.rerandomize_batch_drawn_dev(ty, N, M, N_, *consts, *src, stream, None, None, None, *got2)
        eng.sync()
        assert same(got, want) and same(got2, want) and same(back, mdl)
        assert not same(got[:1], src[:1])  # (the commitments did move)
        assert (verify_all(wl, got) == expect).all()
    h = eng.rerandomize_batch_drawn(ty, N, M, N_, *map(host, consts + valid), stream)
    hw = eng.rerandomize_batch(ty, N, M, N_, *map(host, consts + valid), *map(host, mdl))
    for k in ("xcoms", "ycoms", "pi", "theta"):
        assert (h[k] == hw[k]).all(), k
    for k, t in zip("RST", mdl):
        assert (h[k] == host(t)).all(), k
    eng.rand_set_key(None)


# ---- the mirror layer ----------------------------------------------------------------------------------------------
class _Replay:
    def __init__(self, mats):
        self.q = [v for m_ in mats for row in m_ for v in row]
        self.i = 0

    def fr(self):
        self.i += 1
        return self.q[self.i - 1]


@pytest.mark.parametrize("cid,cname", CURVES)
def test_mirror_device_rng(cid, cname):
    import groth_sahai_rs_amd.mirror as Mi

    c = curve(cname)
    g = c.golden["crs"]
    crs = Mi.CRS([c.com1(g["u"][0]), c.com1(g["u"][1])], [c.com2(g["v"][0]), c.com2(g["v"][1])], c.g1(g["g1"]),
                 c.g2(g["g2"]), c.f12(g["gt"]), cid)
    try:
        case = c.golden["cases"][4]  # PPE dense 2x2
        equ = Mi.PPE([c.g1(v) for v in case["a"]], [c.g2(v) for v in case["b"]],
                     [[c.fr_hex(s) for s in row] for row in case["gamma"]], c.f12(case["target"]))
        X, Y = [c.g1(v) for v in case["xvars"]], [c.g2(v) for v in case["yvars"]]
        rng = Mi.DeviceRng(crs.engine, rv.KEY_TEST)
        proof = equ.commit_and_prove(X, Y, crs, rng)
        assert rng.stream == 1 and equ.verify(proof, crs)
        mR, mS, mT = rv.drawn_rst(rv.KEY_TEST, c.r, 0, 1, 2, 2, 0)
        flat = lambda mats: np.concatenate([v for m_ in mats for row in m_ for v in row])
        assert (flat([proof.xcoms.rand]) == mR).all() and (flat([proof.ycoms.rand]) == mS).all()
        assert (flat([proof.equ_proofs[0].rand]) == mT).all()
        # the carried randomness is the proof's: the ordinary path on it gives the same bytes
        again = equ.commit_and_prove(X, Y, crs, _Replay([proof.xcoms.rand, proof.ycoms.rand, proof.equ_proofs[0].rand]))
        assert again.xcoms == proof.xcoms and again.ycoms == proof.ycoms
        assert all((a == b).all() for a, b in zip(again.equ_proofs[0].pi, proof.equ_proofs[0].pi))
        assert all((a == b).all() for a, b in zip(again.equ_proofs[0].theta, proof.equ_proofs[0].theta))
        q = Mi.rerandomize(equ, proof, crs, rng)
        assert rng.stream == 2 and equ.verify(q, crs)
        assert not all((a == b).all() for a, b in zip(q.xcoms.coms, proof.xcoms.coms))
        # q carries R + R', S + S', T'': the ordinary prover on them reproduces q
        again = equ.commit_and_prove(X, Y, crs, _Replay([q.xcoms.rand, q.ycoms.rand, q.equ_proofs[0].rand]))
        assert again.xcoms == q.xcoms and again.ycoms == q.ycoms
        assert all((a == b).all() for a, b in zip(again.equ_proofs[0].pi, q.equ_proofs[0].pi))
        # R' itself is the model's RERAND draw of stream 1
        rR = rv.drawn_rst(rv.KEY_TEST, c.r, 0, 1, 2, 2, 1, rerand=True)[0].reshape(-1, 4)
        for i, v in enumerate(v for row in q.xcoms.rand for v in row):
            want = (c.fr_dec(mR.reshape(-1, 4)[i]) + c.fr_dec(rR[i])) % c.r
            assert c.fr_dec(v) == want, i
        # a Statement of two equations, and another rng changes nothing
        st = Mi.Statement([equ, equ])
        sp = st.commit_and_prove(X, Y, crs, rng)
        assert rng.stream == 3 and st.verify(sp, crs)
        sR, sS, sT = rv.drawn_rst(rv.KEY_TEST, c.r, 0, 2, 2, 2, 2, shared=True)
        assert (flat([sp.xcoms.rand]) == sR).all() and (flat([sp.ycoms.rand]) == sS).all()
        assert (flat([pf.rand for pf in sp.equ_proofs]) == sT).all()
    finally:
        crs.engine.close()

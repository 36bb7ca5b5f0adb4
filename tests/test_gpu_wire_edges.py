"""The engine's trust boundary on the device, on adversarial encodings: gs_wire_decode_* / gs_wire_encode_* and
gs_validate_points against the big-integer oracle on the tables of tests/wirevec.py -- low-order and mixed-order points
of every small cofactor prime, every branch of fp2_sqrt, every flag combination, every coordinate next to p, Fr next to
r, GT elements outside the r-torsion -- each table in ONE call, ordered so that accepted and rejected elements alternate
inside every wave.  test_wire.py runs the same point tables through the host compile of the headers; this file is the
gfx950 build with its out-of-line multiplier and point subroutines.  The expectations are the oracle's alone."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import wirevec as V
from gsutil import curve

pytestmark = pytest.mark.gpu

SLICES = (1, 63, 64, 65)


@pytest.fixture(scope="module", params=V.CURVES)
def env(request):
    import groth_sahai_rs_amd as gs

    c = curve(request.param)
    eng = gs.Engine(c.curve_id, 0)
    yield c, eng
    eng.close()


def u8(data):
    return np.frombuffer(b"".join(data), dtype=np.uint8).reshape(len(data), -1)


def report(table, ok, want, why):
    return [(k.name, "device %d" % g, "oracle: %s" % (y or "accepted")) for k, g, w, y in zip(table, ok, want, why) if g != w]


def check_wave_shapes(decode, buf, full):
    """per-element results do not depend on how many elements share the call, nor on their neighbours"""
    vals, ok = full
    n = len(ok)
    assert n > 128 and n % 64 not in (0, 1)
    for m in SLICES:
        v, o = decode(buf[:m])
        assert len(o) == m and (o == ok[:m]).all() and (v == vals[:m]).all(), m
    v, o = decode(np.ascontiguousarray(buf[::-1]))
    assert (o[::-1] == ok).all() and (v[::-1] == vals).all(), "reversed"


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("compressed", [True, False])
def test_point_decoder_against_the_oracle(env, group, compressed):
    c, eng = env
    kind = "g%d" % group
    table = V.wave_order(V.point_cases(c.name, group, compressed), V.pad_cases(c.name, group, compressed))
    V.setc(c.name)
    buf = u8([k.data for k in table])
    results = {}
    for validate in (True, False):
        want = [int(k.ok_v if validate else k.ok_nv) for k in table]
        why = [k.why_v if validate else k.why_nv for k in table]
        vals, ok = eng.wire_decode(kind, buf, compressed, validate)
        results[validate] = (vals, ok)
        bad = report(table, ok.tolist(), want, why)
        assert not bad, (c.name, kind, compressed, validate, bad)
        expect = np.stack([V.point_limbs(c.name, k.value, group) if w else np.zeros(vals.shape[1] // 8, dtype=np.uint64)
                           for k, w in zip(table, want)]).view(np.uint8)
        wrong = [k.name for k, a, b in zip(table, vals, expect) if not (a == b).all()]
        assert not wrong, (c.name, kind, compressed, validate, "decoded limbs (rejected: the identity)", wrong)
        # accepted elements go back to the input bytes in the same form and to the oracle's bytes in the other one
        idx = [i for i, w in enumerate(want) if w]
        acc = np.ascontiguousarray(vals[idx])
        same = eng.wire_encode(kind, acc, compressed)
        other = eng.wire_encode(kind, acc, not compressed)
        for j, i in enumerate(idx):
            assert same[j].tobytes() == table[i].data, (table[i].name, "re-encoded")
            assert other[j].tobytes() == V.W.enc_point(table[i].value, group, not compressed), (table[i].name, "other form")
    check_wave_shapes(lambda b: eng.wire_decode(kind, b, compressed, True), buf, results[True])
    check_wave_shapes(lambda b: eng.wire_decode(kind, b, compressed, False), buf, results[False])
    # the plain-ladder option is about scalar multiplication; the verdicts do not move with it
    eng.set_option("endo", 0)
    try:
        vals, ok = eng.wire_decode(kind, buf, compressed, True)
    finally:
        eng.set_option("endo", 1)
    assert (ok == results[True][1]).all() and (vals == results[True][0]).all()


@pytest.mark.parametrize("group", [1, 2])
def test_validate_points_against_the_oracle(env, group):
    c, eng = env
    V.setc(c.name)
    VP = namedtuple("VP", "name limbs ok_v")
    seen, table = set(), []
    for compressed in (True, False):
        for k in V.point_cases(c.name, group, compressed):
            if k.value != V.REJECT and k.value not in seen:  # everything the oracle decodes without validation
                seen.add(k.value)
                table.append(VP(k.name, V.point_limbs(c.name, k.value, group), k.ok_v))
    # coordinates that are no canonical limb strings: the WORDS equal p, p + 1, all ones, one coordinate at a time
    honest = V.point_limbs(c.name, V.honest_point(c.name, group, 13), group)
    for j in range(honest.size // c.nq):
        for nm, v in (("p", c.p), ("p+1", c.p + 1), ("all-ones", c.Rq - 1)):
            w = honest.copy()
            w[j * c.nq:(j + 1) * c.nq] = [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(c.nq)]
            table.append(VP("words/coord%d=%s" % (j, nm), w, False))
    table.append(VP("words/zero", np.zeros_like(honest), True))  # (0, 0): the identity
    pads = [VP(k.name, V.point_limbs(c.name, k.value, group), k.ok_v) for k in V.pad_cases(c.name, group, True)]
    table = V.wave_order(table, pads)
    pts, want, names = [k.limbs for k in table], [int(k.ok_v) for k in table], [k.name for k in table]
    P = np.stack(pts)
    ok = eng.validate_points(group, P)
    bad = [(nm, "device %d" % g) for nm, g, w in zip(names, ok.tolist(), want) if g != w]
    assert not bad, (c.name, group, bad)
    n = len(want)
    assert n > 128
    for m in SLICES:
        assert (eng.validate_points(group, P[:m]) == ok[:m]).all(), m
    assert (eng.validate_points(group, np.ascontiguousarray(P[::-1]))[::-1] == ok).all()
    eng.set_option("endo", 0)
    try:
        assert (eng.validate_points(group, P) == ok).all()
    finally:
        eng.set_option("endo", 1)


def test_fr_decoder_against_the_oracle(env):
    c, eng = env
    table = V.wave_order(V.fr_cases(c.name), [k for k in V.fr_cases(c.name) if k.ok], accepted=lambda k: k.ok)
    buf = u8([k.data for k in table])
    vals, ok = eng.wire_decode("fr", buf)
    bad = report(table, ok.tolist(), [int(k.ok) for k in table], [k.why for k in table])
    assert not bad, (c.name, bad)
    expect = np.stack([c.fr(k.value) if k.ok else np.zeros(c.nr, dtype=np.uint64) for k in table]).view(np.uint8)
    assert (vals == expect).all(), [k.name for k, a, b in zip(table, vals, expect) if not (a == b).all()]
    idx = [i for i, k in enumerate(table) if k.ok]
    back = eng.wire_encode("fr", np.ascontiguousarray(vals[idx]))
    assert all(back[j].tobytes() == table[i].data for j, i in enumerate(idx))
    check_wave_shapes(lambda b: eng.wire_decode("fr", b), buf, (vals, ok))


def test_gt_decoder_against_the_oracle(env):
    c, eng = env
    cases = V.gt_cases(c.name)
    table = V.wave_order(cases, [k for k in cases if k.ok_v])
    V.setc(c.name)
    buf = u8([k.data for k in table])
    for validate in (True, False):
        want = [int(k.ok_v if validate else k.ok_nv) for k in table]
        vals, ok = eng.wire_decode("gt", buf, validate=validate)
        bad = report(table, ok.tolist(), want, [k.why_v if validate else k.why_nv for k in table])
        assert not bad, (c.name, validate, bad)
        expect = np.stack([V.gt_limbs(c.name, k.value) if w else np.zeros(12 * c.nq, dtype=np.uint64)
                           for k, w in zip(table, want)]).view(np.uint8)
        wrong = [k.name for k, a, b in zip(table, vals, expect) if not (a == b).all()]
        assert not wrong, (c.name, validate, "decoded coefficients (rejected: all twelve zero)", wrong)
        idx = [i for i, w in enumerate(want) if w]
        back = eng.wire_encode("gt", np.ascontiguousarray(vals[idx]))
        assert all(back[j].tobytes() == table[i].data for j, i in enumerate(idx))
        check_wave_shapes(lambda b: eng.wire_decode("gt", b, validate=validate), buf, (vals, ok))


def test_encoders_on_values_no_decoder_yields(env):
    """the sort comparison on its boundary (points that are on no curve), and fq_to_canonical on limb-boundary values"""
    c, eng = env
    V.setc(c.name)
    for group in (1, 2):
        cases = V.enc_point_cases(c.name, group)
        P = np.stack([V.point_limbs(c.name, pt, group) for _, pt in cases])
        for compressed in (True, False):
            got = eng.wire_encode("g%d" % group, P, compressed)
            for (name, pt), g in zip(cases, got):
                assert g.tobytes() == V.W.enc_point(pt, group, compressed), (c.name, group, name, compressed)
    vals = V.enc_fq_values(c.name)
    got = eng.wire_encode("gt", np.stack([c.fq(v) for v in vals]).reshape(len(vals) // 12, -1))
    for i in range(len(vals) // 12):
        assert got[i].tobytes() == V.W.enc_gt(V.O.f12_unflat(vals[12 * i:12 * i + 12])), (c.name, i)


def test_empty_batches_touch_nothing(env):
    c, eng = env
    lib, sz = eng.lib, ctypes.c_size_t(0)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    src = np.full(4096, 0x5A, dtype=np.uint8)
    out = np.full(4096, 0xC3, dtype=np.uint8)
    ok = np.full(64, 0x77, dtype=np.uint8)
    for fn in (lib.gs_wire_decode_g1, lib.gs_wire_decode_g2):
        for compressed in (0, 1):
            assert fn(eng.ctx, sz, compressed, 1, vp(src), vp(out), vp(ok)) == 0
    assert lib.gs_wire_decode_fr(eng.ctx, sz, vp(src), vp(out), vp(ok)) == 0
    assert lib.gs_wire_decode_gt(eng.ctx, sz, 1, vp(src), vp(out), vp(ok)) == 0
    for fn in (lib.gs_wire_encode_g1, lib.gs_wire_encode_g2):
        assert fn(eng.ctx, sz, 1, vp(src), vp(out)) == 0
    assert lib.gs_wire_encode_fr(eng.ctx, sz, vp(src), vp(out)) == 0
    assert lib.gs_wire_encode_gt(eng.ctx, sz, vp(src), vp(out)) == 0
    for group in (1, 2):
        assert lib.gs_validate_points(eng.ctx, group, sz, vp(src), vp(ok)) == 0
    assert (src == 0x5A).all() and (out == 0xC3).all() and (ok == 0x77).all()

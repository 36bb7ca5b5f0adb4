"""Real-form Miller lines (csrc/gs_pairing.cuh `Line`, `line_real`, `line_unit`; csrc/gs_tower.cuh f12_mul_by_014r / _034r;
the multiplier body fp2dot3r of csrc/gen_mul28_asm.py) on the CPU.  No GPU needed.

(a) The emitted instruction streams `sub_body_fp2dot(L, 3, real_last=True)` for L = 14 and 10, interpreted by `Machine`
    (tests/test_pointops_gen.py) as tests/test_mul28_gen.py does for the other bodies and compared with big integers:

        a00 a01 b00 b01 | a10 a11 b10 b11 | a20 a21 r   at v0, vL, .. v10L       ->  c0 v11L..,  c1 v12L..

    on the three-pair dot product's own operand sets of tests/arithvec.py (its b21 dropped: a real r IS b2 = (r, 0), the
    expected limbs are those of the general body with b21 = 0), and on operands at THIS body's contract limit
        2 (A_a0 A_b0 + A_a1 A_b1) + A_a2 A_r <= 8
    (a column of an accumulator takes 2 L products per full pair, L for the real one and L reduction terms), with the sign
    patterns that make every term of a column add up; for those the largest column sum reached must EQUAL what the bounds
    allow.  One negative control: one operand one step over the contract trips the interpreter's width assertion.

(b) A twin source of its own, tests/twin/host_lines.cpp, built with -DGS_FQ28_CHECK (every limb contract asserted) twice:
    as it is, and with -DGS_LINES_GENERAL.  On both curves: the real sparse products equal the general ones (real
    coefficient 0, 1, p - 1 and random) and count 6 x 12 L^2 multiply-adds; line_real(l) is l conj(ly) coefficient by
    coefficient; a line with ly = 0 comes back unchanged; the table form is l / ly with the coefficient 1; and a
    multi-Miller value over 3 pairs, finally exponentiated, is the same in both builds for each of the three loop forms,
    with and without line tables, with an identity argument in one pair."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import arithvec as av
from gsutil import HERE, REPO, curve, ptr
from test_mul28_gen import _run
from test_pointops_gen import mulgen

CURVES = [("bls12_381", 14), ("bn254", 10)]
S = 1 << 28
I31 = (1 << 31) - 1


# ---------------------------------------------------------------------------------------------------------------------
# (a) the emitted body
# ---------------------------------------------------------------------------------------------------------------------
def _layout(L):
    return mulgen.sub_body_fp2dot(L, 3, True), [q * L for q in range(11)], [11 * L, 12 * L], range(13 * L, 15 * L + 4)


def _terms(ops):
    a00, a01, b00, b01, a10, a11, b10, b11, a20, a21, r = ops
    neg = lambda v: [-x for x in v]
    return [[(a00, b00), (neg(a01), b01), (a10, b10), (neg(a11), b11), (a20, r)],
            [(a00, b01), (a01, b00), (a10, b11), (a11, b10), (a21, r)]]


def _exact(c, ops):
    return av.exact(c, "fp2dot3", list(ops) + [[0] * c.L])


def _in_contract(c, bd):
    """the documented contract on labelled limb bounds: bd = 11 x (bound on |limb i|, i < L - 1; bound on |top limb|)"""
    B = [b for b, _ in bd]
    if any(t >= (1 << 26) for _, t in bd) or any(b >= (1 << 31) for b in B):
        return False
    room = (1 << 63) - c.L * (1 << 56)
    full = sum(2 * c.L * max(B[4 * t], B[4 * t + 1]) * max(B[4 * t + 2], B[4 * t + 3]) for t in range(2))
    return full + c.L * max(B[8], B[9]) * B[10] < room


def _column_bound(c, bd, which):
    L = c.L
    bv = [[b] * (L - 1) + [t] for b, t in bd]
    conv = lambda x, y, k: sum(x[i] * y[k - i] for i in range(max(0, k - L + 1), min(k, L - 1) + 1))
    return max(sum(conv(bv[4 * t], bv[4 * t + 2 + which], k) + conv(bv[4 * t + 1], bv[4 * t + 3 - which], k) for t in range(2))
               + conv(bv[8 + which], bv[10], k) for k in range(2 * L - 1))


def _limit_cases(c):
    """(name, ops, bounds, accumulator whose analytical column maximum the case reaches)"""
    Z = (0, 0)
    splits = {  # (B_a, B_b) of the two full pairs, (B_a2, B_r): 2 (A A + A A) + A A = 8
        "0+0+8x1": [Z, Z, (I31, S)], "0+0+1x8": [Z, Z, (S, I31)], "0+0+4x2": [Z, Z, (1 << 30, 1 << 29)],
        "2.4+0+0": [(1 << 30, S), Z, Z], "0+2.4+0": [Z, (1 << 29, 1 << 29), Z],
        "2.2+2.1+2": [(1 << 29, S), (S, S), (1 << 29, S)], "2.1+2.1+4": [(S, S), (S, S), (S, 1 << 30)],
        "2.1+2.2+1x2": [(S, S), (S, 1 << 29), (S, 1 << 29)], "2.1+2.1+1": [(S, S), (S, S), (S, S)],
    }
    out = []
    for tier, T in ((1, av.TOP1), (2, av.TOP2)):
        for nm, sp in splits.items():
            bd = []
            for Ba, Bb in sp[:2]:
                bd += [(Ba, T if Ba else 0), (Ba, T if Ba else 0), (Bb, T if Bb else 0), (Bb, T if Bb else 0)]
            Ba, Br = sp[2]
            bd += [(Ba, T if Ba else 0), (Ba, T if Ba else 0), (Br, T if Br else 0)]
            assert _in_contract(c, bd), nm
            # c0 = a00 b00 - a01 b01 + ... + a20 r: a*1 negative, the rest positive;  c1: everything positive
            for pn, sg, att in (("c0+", (1, -1, 1, 1), 0), ("c0-", (-1, 1, 1, 1), 0), ("c1+", (1, 1, 1, 1), 1), ("c1-", (-1, -1, 1, 1), 1)):
                signs = [sg[q % 4] for q in range(8)] + [sg[0], sg[1] if att == 1 else sg[0], 1]
                ops = [[s * b] * (c.L - 1) + [s * t] for s, (b, t) in zip(signs, bd)]
                out.append(("t%d.%s.%s" % (tier, nm, pn), ops, bd, att))
    return out


def _from_dot3(cname):
    n_rand = 0
    for case in av.multiplier_cases(cname):
        if case.body != "fp2dot3":
            continue
        if case.kind == "random":
            n_rand += 1
            if n_rand > 40:
                continue
        yield case.name, case.ops[:11]


@pytest.mark.parametrize("cname,L", CURVES)
def test_emitted_dot3r_on_the_dot_products_operand_sets(cname, L):
    c = av.ctx(cname)
    lay = _layout(L)
    n = 0
    for name, ops in _from_dot3(cname):
        got = _run(c, "fp2dot3r", ops, lay)
        assert got == _exact(c, ops), name
        assert all(0 <= x < (1 << 28) for r in got for x in r[:-1]), name
        n += 1
    assert n >= 40 + 8


@pytest.mark.parametrize("cname,L", CURVES)
def test_emitted_dot3r_at_its_own_contract_limit(cname, L):
    c = av.ctx(cname)
    lay = _layout(L)
    reached = [0, 0]
    for name, ops, bd, att in _limit_cases(c):
        st = [av.Stat(), av.Stat()]
        want = [av.model_acc(c, t, st[i]) for i, t in enumerate(_terms(ops))]
        assert want == _exact(c, ops), name
        assert st[att].prod == _column_bound(c, bd, att), name  # extreme, not merely large
        assert _run(c, "fp2dot3r", ops, lay) == want, name
        reached = [max(r, s.acc) for r, s in zip(reached, st)]
    # the documented bound is tight on BLS12-381: the accumulators come within a fifth of the 64-bit range
    assert all(r < (1 << 63) for r in reached)
    if L == 14:
        assert min(reached) > 0.8 * (1 << 63)


@pytest.mark.parametrize("cname,L", CURVES)
def test_emitted_dot3r_one_step_over_the_contract(cname, L):
    """negative control: the limit case 2.1 + 2.1 + 4 with the lower limbs of the real operand doubled until the
    big-integer model itself leaves int64 -- the interpreter must object as well"""
    c = av.ctx(cname)
    name, ops, bd, att = next(x for x in _limit_cases(c) if x[0] == "t1.2.1+2.1+4.c1+")
    ops = [list(o) for o in ops]
    q = 8  # a20: bound 2^28, room to double
    for _ in range(3):
        ops[q] = [2 * x for x in ops[q][:-1]] + [ops[q][-1]]
        ops[9] = list(ops[q])
        assert av.s32ok(ops[q])
        try:
            [av.model_acc(c, t) for t in _terms(ops)]
        except AssertionError:
            break
    else:
        raise AssertionError("no over-contract case")
    with pytest.raises(AssertionError, match="overflow|wrapped"):
        _run(c, "fp2dot3r", ops, _layout(L))


def test_dot3r_is_shorter_by_two_limb_products():
    for L in (14, 10):
        mads = lambda prog: sum(1 for x in prog if x.startswith("v_mad_"))
        assert mads(mulgen.sub_body_fp2dot(L, 3)) == 14 * L * L
        assert mads(mulgen.sub_body_fp2dot(L, 3, True)) == 12 * L * L


# ---------------------------------------------------------------------------------------------------------------------
# (b) the headers on the host
# ---------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "twin", "host_lines.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _build(tag, flags):
    so = os.path.join(HERE, "twin", "libhost_lines_%s.so" % tag)
    csrc = os.path.join(REPO, "groth_sahai_rs_amd", "csrc")
    srcs = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".cuh", ".h"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        if not os.path.exists(CLANG):
            pytest.skip("no host clang++ for the CPU twin")
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wno-psabi", "-DGS_FQ28_CHECK", "-shared", "-fPIC", "-pthread"]
                              + flags + [SRC, "-o", so])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def real():
    return _build("real", [])


@pytest.fixture(scope="module")
def general():
    return _build("general", ["-DGS_LINES_GENERAL"])


def _fq(c, v):
    return c.fq(v % c.p)


def _f2(c, a):
    return np.concatenate([_fq(c, a[0]), _fq(c, a[1])])


def _f2mul(p, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


@pytest.mark.parametrize("cname,L", CURVES)
def test_line_sizes(real, general, cname, L):
    assert getattr(real, "lines_dwords_" + cname)() == 5 * L
    assert getattr(general, "lines_dwords_" + cname)() == 6 * L


@pytest.mark.parametrize("cname,L", CURVES)
def test_real_sparse_products_equal_the_general_ones(real, cname, L):
    c = curve(cname)
    rnd = random.Random(7 + L)
    f = getattr(real, "lines_sparse_" + cname)
    f.restype = ctypes.c_long
    rv = lambda: rnd.randrange(c.p)
    reals = [0, 1, c.p - 1] + [rv() for _ in range(5)]
    for which in (0, 1):  # f12_mul_by_014r, f12_mul_by_034r: both compile and must hold on either tower
        for r in reals:
            x = np.concatenate([_fq(c, rv()) for _ in range(12)])
            a, b = _f2(c, (rv(), rv())), _f2(c, (rv(), rv()))
            o1, o2 = np.zeros(12 * c.nq, dtype=np.uint64), np.ones(12 * c.nq, dtype=np.uint64)
            mads = f(which, ptr(x), ptr(a), ptr(b), ptr(_fq(c, r)), ptr(o1), ptr(o2))
            assert (o1 == o2).all(), (which, hex(r))
            assert mads == 6 * 12 * L * L
        # f = 1, and a line that is a real number
        one = np.concatenate([_fq(c, 1)] + [_fq(c, 0)] * 11)
        z2 = _f2(c, (0, 0))
        o1, o2 = np.zeros(12 * c.nq, dtype=np.uint64), np.ones(12 * c.nq, dtype=np.uint64)
        f(which, ptr(one), ptr(z2), ptr(z2), ptr(_fq(c, 5)), ptr(o1), ptr(o2))
        assert (o1 == o2).all()
        vals = [int(v, 16) for v in c.f12_dec(o1)]
        assert sorted(vals) == [0] * 11 + [5]


@pytest.mark.parametrize("cname,L", CURVES)
def test_real_form_is_the_line_times_conj_ly(real, cname, L):
    c = curve(cname)
    p = c.p
    rnd = random.Random(11 + L)
    f = getattr(real, "lines_realform_" + cname)
    rv2 = lambda: (rnd.randrange(p), rnd.randrange(p))
    lys = [rv2() for _ in range(6)] + [(1, 0), (0, 1), (p - 1, 0), (0, p - 1), (3, 0), (0, 0)]
    for ly in lys:
        l0, lx = rv2(), rv2()
        inp = np.concatenate([_f2(c, l0), _f2(c, lx), _f2(c, ly)])
        for what in (0, 1):
            out = np.zeros(5 * c.nq, dtype=np.uint64)
            f(what, ptr(inp), ptr(out))
            got = [c.fq_dec(out[i * c.nq:(i + 1) * c.nq]) for i in range(5)]
            if ly == (0, 0):  # degenerate: unchanged, ly' = 0 -- already a real form of itself
                assert got == [l0[0], l0[1], lx[0], lx[1], 0], what
                continue
            if what == 0:     # line_real: l conj(ly), ly' = N(ly)
                k = (ly[0], (-ly[1]) % p)
                n = (ly[0] * ly[0] + ly[1] * ly[1]) % p
            else:             # line_unit (tables): l / ly, ly' = 1
                ni = pow((ly[0] * ly[0] + ly[1] * ly[1]) % p, -1, p)
                k = (ly[0] * ni % p, (-ly[1]) * ni % p)
                n = 1
            assert n != 0
            assert got == list(_f2mul(p, l0, k)) + list(_f2mul(p, lx, k)) + [n], (what, ly)


@pytest.mark.parametrize("cname,L", CURVES)
def test_multi_miller_values_agree_with_the_general_build(real, general, cname, L):
    """3 pairs, the three loop forms (single accumulator, twin, lane pair), no / some / all pairs reading line tables, an
    identity argument in one pair (G1 in one run, G2 in another): after the final exponentiation the real-form build
    gives exactly what the GS_LINES_GENERAL build of the same source gives."""
    c = curve(cname)
    ps = c.golden["pairing_sum"]
    g = c.golden
    # the fixture's pairs hold identities of their own; take three full ones and place the identity explicitly
    g1s = [g["g1_smul"][i]["out"] for i in (1, 2, 3)]
    g2s = [g["g2_smul"][i]["out"] for i in (2, 1, 3)]
    assert all(x is not None for x in g1s + g2s) and len(ps["x"]) >= 3
    fr, fg = getattr(real, "lines_pairing_" + cname), getattr(general, "lines_pairing_" + cname)
    n = 3
    for ident in ("none", "g1", "g2"):
        P = np.concatenate([c.g1(None if (ident == "g1" and i == 1) else g1s[i]) for i in range(n)])
        Q = np.concatenate([c.g2(None if (ident == "g2" and i == 0) else g2s[i]) for i in range(n)])
        ref = None
        for mode in (0, 1, 2):
            for mask in (0, 0b100, 0b110, 0b111):
                a, b = np.zeros(2 * 12 * c.nq, dtype=np.uint64), np.ones(2 * 12 * c.nq, dtype=np.uint64)
                fr(n, ptr(P), ptr(Q), mask, ptr(a), mode)
                fg(n, ptr(P), ptr(Q), mask, ptr(b), mode)
                k = 12 * c.nq * (2 if mode else 1)
                assert (a[:k] == b[:k]).all(), (ident, mode, mask)
                if mode:
                    assert (a[12 * c.nq:k] == a[:12 * c.nq]).all()
                ref = a[:12 * c.nq].copy() if ref is None else ref
                assert (a[:12 * c.nq] == ref).all(), (ident, mode, mask)
    # and the fixture's own four-cell product through the real build (cell (1, 1)), identities and all
    Pf = np.concatenate([c.g1(x[1]) for x in ps["x"]])
    Qf = np.concatenate([c.g2(y[1]) for y in ps["y"]])
    for mode in (0, 1, 2):
        out = np.zeros(2 * 12 * c.nq, dtype=np.uint64)
        fr(len(ps["x"]), ptr(Pf), ptr(Qf), 0b010, ptr(out), mode)
        assert c.f12_dec(out[:12 * c.nq]) == ps["out"][3], mode

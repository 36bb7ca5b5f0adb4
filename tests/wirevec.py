"""Adversarial encodings for the engine's trust boundary -- the wire decoders / encoders of csrc/gs_wire.cuh, the range
checks of k_wire_fr / k_wire_fq, f12_in_torsion and gs_validate_points -- and what the big-integer oracle says about each.
tests/test_wire.py runs the point tables on the CPU twin, tests/test_gpu_wire_edges.py runs everything on the device.
Pure Python, deterministic (one seed), no engine import: every expectation is the verdict, the ValueError reason or the
decoded value of oracle/gs_wire_oracle.py (`dec_point`, `dec_fr`, `dec_gt`, `enc_*`), subgroup membership being the
oracle's plain double-and-add `ec_mul(r, P)`.

One builder per (curve, kind):

  point_cases(cname, group, compressed)   named byte strings, each with the oracle's verdict with and without validation
  fr_cases(cname) / gt_cases(cname)        the same for scalars and GT elements
  enc_point_cases(cname, group)            (x, y) pairs for the ENCODER only: they need not be on the curve
  enc_fq_values(cname)                     canonical Fq values for gs_wire_encode_gt (fq_to_canonical's three selections)

What the point tables hold (DESIGN.md has the prose): subgroup points; for every prime q < 2^20 of the cofactor a point
T_q of exact order q, -T_q and the mixed-order S +- T_q; the large-order cofactor part [r]P; x = 0; one x for every
branch of fp2_sqrt, labelled by a Python model of the branch (`sqrt_branch`); every combination of the flag bits; every
coordinate at p-1, p, p+1, p +- 2^32, p +- 2^(32(N-1)) and the largest value the non-flag bits hold; off-curve and
on-curve neighbours of an honest point.  `selfcheck(cname)` proves from the oracle alone that these classes are really
in the table."""
import functools
import os
import random
import sys
from collections import Counter, namedtuple

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))
import gs_oracle as O  # noqa: E402
import gs_wire_oracle as W  # noqa: E402

SEED = 20241017
CURVES = ["bls12_381", "bn254"]
REJECT = "reject"  # `value` of a case the oracle rejects even without validation

# name, bytes, verdict with / without validation, the oracle's reason (None when accepted), the value decoded without
# validation (REJECT when there is none), a free label (the fp2_sqrt branch, the cofactor prime)
Case = namedtuple("Case", "name data ok_v ok_nv why_v why_nv value label")
FrCase = namedtuple("FrCase", "name data ok why value")

# cofactor primes that must yield a point (checked by hand with the oracle; the others divide the cofactor squared and
# the builder strips their q-part, so they normally yield one too -- `cofactor_points` records what happened)
MUST_YIELD = {("bls12_381", 1): [3], ("bls12_381", 2): [2713, 11953, 262069], ("bn254", 1): [], ("bn254", 2): [10069]}
SQRT_BRANCHES = ("real", "imaginary", "delta1", "delta2", "no-norm")


def setc(cname):
    return O.set_curve(O._bls12_381() if cname == "bls12_381" else O._bn254())


def fld(group):
    return O.FP if group == 1 else O.FP2


def nbytes(cname):
    return curve(cname).nq * 8


# ---- the curves' orders and cofactors ---------------------------------------------------------------------------------
def curve_order(cname, group):
    """#E(Fp) (group 1) / #E'(Fp2) (group 2), from the families' polynomials; `cofactor_points` re-checks [n]P = O"""
    oc = setc(cname)
    x = oc.x
    if cname == "bls12_381":
        if group == 1:
            h, rem = divmod((x - 1) ** 2, 3)
            assert rem == 0 and h * oc.r == oc.p + 1 - (x + 1)  # trace t = x + 1
        else:
            h, rem = divmod(x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13, 9)
            assert rem == 0
    else:
        h = 1 if group == 1 else 2 * oc.p - oc.r
        assert oc.r == oc.p + 1 - (6 * x * x + 1)  # trace t = 6 x^2 + 1
    return h * oc.r, h


@functools.lru_cache(maxsize=None)
def cofactor_primes(cname, group):
    """[(q, e)]: the primes q < 2^20 of the cofactor with their multiplicity in it"""
    _, h = curve_order(cname, group)
    out, q = [], 2
    while q < (1 << 20):
        if h % q == 0:
            e = 0
            while h % q == 0:
                h //= q
                e += 1
            out.append((q, e))
        q += 1 if q == 2 else 2
    return out


def sqrt_branch(cname, x):
    """which way csrc/gs_wire.cuh fp2_sqrt goes for the Fp2 coordinate x of the twist (a Python model of the branch)"""
    oc = setc(cname)
    p = oc.p
    a0, a1 = O.f2_add(O.f2_mul(O.f2_sqr(x), x), oc.b2)
    is_sq = lambda v: v % p == 0 or pow(v % p, (p - 1) // 2, p) == 1
    if a1 == 0:
        return "real" if is_sq(a0) else "imaginary"
    n2 = (a0 * a0 + a1 * a1) % p
    if not is_sq(n2):
        return "no-norm"
    n = pow(n2, (p + 1) // 4, p)  # the root fq_sqrt returns
    return "delta1" if is_sq((a0 + n) * pow(2, -1, p)) else "delta2"


def curve_point(cname, group, x):
    """the curve / twist point above x with the root the oracle's square root returns, or None"""
    oc = setc(cname)
    if group == 1:
        y = W._sqrt_fq((x ** 3 + oc.b) % oc.p)
    else:
        y = W._sqrt_f2(O.f2_add(O.f2_mul(O.f2_sqr(x), x), oc.b2))
    return None if y is None else (x, y)


def start_points(cname, group, count, first=1):
    """curve points found by counting x (G2: x = (k, 1)) up from `first`"""
    out, k = [], first
    while len(out) < count:
        pt = curve_point(cname, group, k if group == 1 else (k, 1))
        if pt is not None:
            out.append(pt)
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def cofactor_points(cname, group):
    """{q: T_q} with T_q of exact order q, for the primes q < 2^20 of the cofactor that yielded one within 8 start
    points: Q = [n / q^e]P with q^e the full power of q in the curve order n, then Q <- [q]Q while that is not O."""
    oc = setc(cname)
    F = fld(group)
    n, _ = curve_order(cname, group)
    primes = cofactor_primes(cname, group)
    if not primes:
        return {}
    starts = start_points(cname, group, 8)
    for pt in starts[:2]:
        assert O.ec_mul(F, n, pt) is None, "curve order"
    out = {}
    for q, _ in primes:
        m = n
        while m % q == 0:
            m //= q
        for pt in starts:
            t = O.ec_mul(F, m, pt)
            if t is None:
                continue
            while True:
                nxt = O.ec_mul(F, q, t)
                if nxt is None:
                    break
                t = nxt
            assert O.ec_mul(F, q, t) is None and t is not None
            out[q] = t
            break
    assert oc.name == cname
    return out


# ---- byte strings -----------------------------------------------------------------------------------------------------
def flag_mask(cname):
    return 0xE0 if cname == "bls12_381" else 0xC0


def flag_pos(cname, data):
    return 0 if cname == "bls12_381" else len(data) - 1


def with_flags(cname, data, flags):
    """the byte string with its flag bits replaced"""
    b = bytearray(data)
    i = flag_pos(cname, b)
    b[i] = (b[i] & ~flag_mask(cname) & 0xFF) | flags
    return bytes(b)


def all_flags(cname):
    return list(range(0, 0x100, 0x20)) if cname == "bls12_381" else [0x00, 0x40, 0x80, 0xC0]


def raw(cname, group, coords, flags):
    """coords: raw integers in the oracle's order (x.c0[, x.c1][, y.c0[, y.c1]]), any value that fits the bytes -- they
    need not be below p; flags: the flag bits as they sit in their byte, OR-ed on top"""
    n = nbytes(cname)
    if cname == "bls12_381":  # big-endian, c1 before c0, flags in the first byte
        order = coords if group == 1 else [v for i in range(0, len(coords), 2) for v in (coords[i + 1], coords[i])]
        b = bytearray(b"".join(v.to_bytes(n, "big") for v in order))
        b[0] |= flags
    else:
        b = bytearray(b"".join(v.to_bytes(n, "little") for v in coords))
        b[-1] |= flags
    return bytes(b)


def coords_of(pt, group, compressed):
    x, y = pt
    xs = [x] if group == 1 else list(x)
    ys = [y] if group == 1 else list(y)
    return xs if compressed else xs + ys


def honest_flags(cname, pt, compressed):
    if cname == "bls12_381":
        return (0x80 | (0x20 if W._largest(pt[1]) else 0)) if compressed else 0
    return 0x80 if W._largest(pt[1]) else 0


def payload_bits(cname, group, compressed, j):
    """bits of coordinate j (oracle order) that are not flag bits"""
    n = 8 * nbytes(cname)
    ncoord = (1 if group == 1 else 2) * (1 if compressed else 2)
    if cname == "bls12_381":
        carrier = 0 if group == 1 else 1  # the first coordinate written: x (G1), x.c1 (G2)
        return n - 3 if j == carrier else n
    return n - 2 if j == ncoord - 1 else n  # the last coordinate written


def judge(cname, group, compressed, name, data, label=None):
    res = []
    for validate in (True, False):
        try:
            res.append((True, None, W.dec_point(data, group, compressed, validate)))
        except ValueError as e:
            res.append((False, str(e), REJECT))
    (ok_v, why_v, val_v), (ok_nv, why_nv, val_nv) = res
    assert not ok_v or (ok_nv and val_v == val_nv)
    return Case(name, data, ok_v, ok_nv, why_v, why_nv, val_nv, label)


def subgroup_points(cname, group):
    """[(name, point)]: the generator, [2]G, [r-1]G and fixed-seed random multiples"""
    oc = setc(cname)
    gen = oc.g1 if group == 1 else oc.g2
    rnd = random.Random(SEED + group)
    ks = [("G", 1), ("2G", 2), ("(r-1)G", oc.r - 1)] + [("rand%d.G" % i, rnd.randrange(3, oc.r - 1)) for i in range(4)]
    return [(nm, O.ec_mul(fld(group), k, gen)) for nm, k in ks]


def honest_point(cname, group, k):
    oc = setc(cname)
    return O.ec_mul(fld(group), k, oc.g1 if group == 1 else oc.g2)


def beta(cname):
    """a primitive cube root of unity of Fp"""
    p = curve(cname).p
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    return pow(g, (p - 1) // 3, p)


def sqrt_branch_xs(cname):
    """[(label, x)]: at least two twist x-coordinates per branch of fp2_sqrt, searched upward"""
    oc = setc(cname)
    p = oc.p
    out, have = [], Counter()
    # x^3 + b' real: 3 x0^2 x1 - x1^3 + Im(b') = 0
    x1 = 2
    while have["real"] < 2 or have["imaginary"] < 2:
        t = (x1 ** 3 - oc.b2[1]) * pow(3 * x1, -1, p) % p
        x0 = W._sqrt_fq(t)
        if x0 is not None:
            for x in ((x0, x1), (p - x0, x1)):
                lab = sqrt_branch(cname, x)
                assert lab in ("real", "imaginary")
                if have[lab] < 2:
                    have[lab] += 1
                    out.append((lab, x))
        x1 += 1
    k = 1
    while min(have[b] for b in ("delta1", "delta2", "no-norm")) < 2:
        lab = sqrt_branch(cname, (k, 1))
        assert lab in ("delta1", "delta2", "no-norm")
        if have[lab] < 3:
            have[lab] += 1
            out.append((lab, (k, 1)))
        k += 1
    return out


def range_values(cname, bits):
    """[(name, v)]: values next to p, and the largest value `bits` bits hold"""
    c = curve(cname)
    p, top = c.p, 32 * (2 * c.nq - 1)
    vals = [("p-1", p - 1), ("p", p), ("p+1", p + 1), ("p-2^32", p - (1 << 32)), ("p+2^32", p + (1 << 32)),
            ("p-2^%d" % top, p - (1 << top)), ("p+2^%d" % top, p + (1 << top)), ("max", (1 << bits) - 1)]
    assert all(0 <= v < (1 << bits) for _, v in vals)
    return vals


@functools.lru_cache(maxsize=None)
def point_cases(cname, group, compressed):
    oc = setc(cname)
    F, p = fld(group), oc.p
    zc = cname == "bls12_381"
    cases, seen = [], set()

    def add(name, data, label=None):
        if data in seen:  # the order-3 points (0, +-2) of BLS12-381 G1 are T_3, -T_3 and the x = 0 cases
            return
        seen.add(data)
        cases.append(judge(cname, group, compressed, name, data, label))

    def add_pt(name, pt, label=None):
        add(name, W.enc_point(pt, group, compressed), label)

    def add_raw(name, coords, flags, label=None):
        add(name, raw(cname, group, coords, flags), label)

    # subgroup points and the identity
    sub = subgroup_points(cname, group)
    for nm, pt in sub:
        add_pt("sub/" + nm, pt)
    add_pt("identity", None)
    S = sub[3][1]
    # cofactor points: T_q, -T_q, S +- T_q, and the large-order part [r]P
    tq = cofactor_points(cname, group)
    for q, t in sorted(tq.items()):
        add_pt("cof/T%d" % q, t, q)
        add_pt("cof/-T%d" % q, O.ec_neg(F, t), q)
        add_pt("cof/S+T%d" % q, O.ec_add(F, S, t), q)
        add_pt("cof/S-T%d" % q, O.ec_add(F, S, O.ec_neg(F, t)), q)
    for i, pt in enumerate(start_points(cname, group, 2, first=100)):
        if cname == "bn254" and group == 1:
            add_pt("curve/P%d" % i, pt)  # cofactor 1: every curve point is in the group
        else:
            add_pt("cof/P%d" % i, pt, "h.r")
            add_pt("cof/[r]P%d" % i, O.ec_mul(F, oc.r, pt), "h")
    # x = 0: the order-3 point of BLS12-381 G1, a coordinate with no point above it elsewhere
    nx = 1 if group == 1 else 2
    if compressed:
        for fl in ([0x80, 0xA0] if zc else [0x00, 0x80]):
            add_raw("x=0/flags%02x" % fl, [0] * nx, fl)
    else:
        for nm, y in (("2", 2), ("-2", p - 2), ("0", 0), ("1", 1)):
            add_raw("x=0/y=" + nm, [0] * nx + ([y] if group == 1 else [y, 0]), 0)
    # every branch of fp2_sqrt (compressed G2), both sort flags
    if group == 2 and compressed:
        for i, (lab, x) in enumerate(sqrt_branch_xs(cname)):
            for fl in ([0x80, 0xA0] if zc else [0x00, 0x80]):
                add_raw("sqrt/%s/%d/flags%02x" % (lab, i, fl), list(x), fl, lab)
    # flags: every combination on an honest encoding and on the identity
    A = honest_point(cname, group, 5)
    for nm, data in (("honest", W.enc_point(A, group, compressed)), ("identity", W.enc_point(None, group, compressed))):
        for fl in all_flags(cname):
            add("flags/%s/%02x" % (nm, fl), with_flags(cname, data, fl))
    ident = W.enc_point(None, group, compressed)
    for nm, pos in (("first", 0), ("middle", len(ident) // 2), ("last", len(ident) - 1)):
        b = bytearray(ident)
        b[pos] |= 0x01
        add("identity/bit-in-%s-byte" % nm, bytes(b))
    # the sort flag flipped: -P in compressed form, not a failure; next to an explicit y it contradicts it
    B = honest_point(cname, group, 7)
    add("sort-flipped", with_flags(cname, W.enc_point(B, group, compressed),
                                   honest_flags(cname, B, compressed) ^ (0x20 if zc else 0x80)))
    # canonical range: one coordinate at a time on an honest point
    Cp = honest_point(cname, group, 9)
    base = coords_of(Cp, group, compressed)
    names = (["x"] if group == 1 else ["x.c0", "x.c1"]) + ([] if compressed else (["y"] if group == 1 else ["y.c0", "y.c1"]))
    for j, cn in enumerate(names):
        for nm, v in range_values(cname, payload_bits(cname, group, compressed, j)):
            co = list(base)
            co[j] = v
            add_raw("range/%s=%s" % (cn, nm), co, honest_flags(cname, Cp, compressed))
    # neighbours of an honest point
    D = honest_point(cname, group, 11)
    bx = (D[0] * beta(cname) % p) if group == 1 else O.f2_scale(D[0], beta(cname))
    add_pt("beta.x", (bx, D[1]))  # phi(D): on the curve and in the subgroup
    if not compressed:
        yp = (D[1] + 1) % p if group == 1 else ((D[1][0] + 1) % p, D[1][1])
        add_pt("off/y+1", (D[0], yp))
        add_pt("off/swapped", (D[1], D[0]))
        add_pt("neg-y", O.ec_neg(F, D))
        if group == 2:
            add_pt("off/y.c1+1", (D[0], (D[1][0], (D[1][1] + 1) % p)))
            add_pt("off/x-conjugate", (O.f2_conj(D[0]), D[1]))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def pad_cases(cname, group, compressed, count=8):
    """honest subgroup points that are in no table"""
    return tuple(judge(cname, group, compressed, "pad/%dG" % k, W.enc_point(honest_point(cname, group, k), group, compressed))
                 for k in range(1000, 1000 + count))


def wave_order(cases, pads, accepted=lambda k: k.ok_v):
    """The cases in the order the device gets them: accepted and rejected ones alternate, so that in every wave of 64 half
    the lanes leave early while the others go through the out-of-line subroutines.  The shorter class goes round again
    (those names get a suffix) until every case is placed and there are more than 128 elements; `pads` (accepted) then make
    n % 64 neither 0 nor 1."""
    acc = [k for k in cases if accepted(k)]
    rej = [k for k in cases if not accepted(k)]
    assert acc and rej and pads
    pairs = max(len(acc), len(rej), 65)
    again = lambda lst: [k if i < len(lst) else k._replace(name="%s/again%d" % (k.name, i // len(lst)))
                         for i, k in ((i, lst[i % len(lst)]) for i in range(pairs))]
    out = [k for pair in zip(again(acc), again(rej)) for k in pair]
    i = 0
    while len(out) % 64 in (0, 1):
        out.append(pads[i % len(pads)]._replace(name="%s/%d" % (pads[i % len(pads)].name, i)))
        i += 1
    return out


# ---- Fr ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fr_cases(cname):
    oc = setc(cname)
    r = oc.r
    rnd = random.Random(SEED + 7)
    vals = [("0", 0), ("1", 1), ("r-1", r - 1), ("r", r), ("r+1", r + 1), ("r-2^32", r - (1 << 32)), ("r+2^32", r + (1 << 32)),
            ("r-2^224", r - (1 << 224)), ("r+2^224", r + (1 << 224)), ("2^256-1", (1 << 256) - 1)]
    vals += [("rand%d" % i, rnd.randrange(r)) for i in range(32)]
    out = []
    for nm, v in vals:
        data = v.to_bytes(32, "little")
        try:
            out.append(FrCase(nm, data, True, None, W.dec_fr(data)))
        except ValueError as e:
            out.append(FrCase(nm, data, False, str(e), REJECT))
    return tuple(out)


# ---- GT ---------------------------------------------------------------------------------------------------------------
def raw_gt(cname, coeffs):
    return b"".join(v.to_bytes(nbytes(cname), "little") for v in coeffs)


@functools.lru_cache(maxsize=None)
def gt_cases(cname):
    oc = setc(cname)
    p = oc.p
    gt = O.f12_unflat([int(s, 16) for s in curve(cname).golden["crs"]["gt"]])
    rnd = random.Random(SEED + 12)
    neg = lambda f: O.FP12.neg(f)
    f = O.f12_unflat(list(range(2, 14)))
    g = O.f12_mul(O.f12_conj(f), O.f12_inv(f))  # f^(p^6 - 1)
    g = O.f12_pow(g, p * p + 1)  # cyclotomic
    h = O.f12_pow(g, oc.r)
    assert h != O.F12_1, "g^r = 1"
    assert O.f12_pow(h, (p ** 4 - p * p + 1) // oc.r) == O.F12_1 and O.f12_pow(g, p ** 4 - p * p + 1) == O.F12_1
    elems = [("one", O.F12_1), ("gt", gt), ("gt^2", O.f12_sqr(gt)), ("gt^(r-1)", O.f12_pow(gt, oc.r - 1))]
    elems += [("gt^rand%d" % i, O.f12_pow(gt, rnd.randrange(3, oc.r - 1))) for i in range(3)]
    elems += [("-1", neg(O.F12_1)), ("-gt", neg(gt)), ("fp-2", O.f12_from_fp(2)), ("cube-root-of-unity", O.f12_from_fp(beta(cname))),
              ("cyclotomic-not-torsion", h), ("junk", f)]
    raws = [(nm, O.f12_flat(e)) for nm, e in elems]
    honest = O.f12_flat(gt)
    for j in range(12):
        co = list(honest)
        co[j] = p
        raws.append(("coeff%d=p" % j, co))
    for j in (0, 5, 11):
        co = list(honest)
        co[j] = p - 1
        raws.append(("coeff%d=p-1" % j, co))
    co = list(honest)
    co[3] = p + 1
    raws.append(("coeff3=p+1", co))
    raws.append(("all-ones", [(1 << (8 * nbytes(cname))) - 1] * 12))
    out = []
    for nm, co in raws:
        data = raw_gt(cname, co)
        res = []
        for validate in (True, False):
            try:
                res.append((True, None, W.dec_gt(data, validate)))
            except ValueError as e:
                res.append((False, str(e), REJECT))
        out.append(Case(nm, data, res[0][0], res[1][0], res[0][1], res[1][1], res[1][2], None))
    return tuple(out)


# ---- encoder-only inputs ----------------------------------------------------------------------------------------------
def enc_point_cases(cname, group):
    """[(name, (x, y))] that put the encoder's sort comparison on its boundary; no curve point has y = (p-1)/2 on either
    G1, so these are not curve points, which neither wire_encode_point nor the oracle's enc_point looks at"""
    p = curve(cname).p
    edge = [("1", 1), ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2), ("p-1", p - 1)]
    if group == 1:
        return [("y=" + nm, (1, v)) for nm, v in edge]
    out = [("y=(%s,0)" % nm, ((1, 0), (v, 0))) for nm, v in edge]
    out += [("y=(0,%s)" % nm, ((1, 0), (0, v))) for nm, v in edge]
    out.append(("y=(p-1,(p-1)/2)", ((1, 0), (p - 1, (p - 1) // 2))))
    out.append(("y=((p-1)/2,(p+1)/2)", ((1, 0), ((p - 1) // 2, (p + 1) // 2))))
    return out


def enc_fq_values(cname):
    """canonical Fq values (a multiple of 12 of them) for gs_wire_encode_gt: 0, 1, p-1, (p+-1)/2, 2^(28k) +- 1 at every
    limb boundary, the values whose BOUNDARY word string is one of those, and 64 fixed-seed random ones"""
    c = curve(cname)
    p = c.p
    L = (p.bit_length() + 27) // 28
    special = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2]
    for k in range(1, L):
        special += [v for v in ((1 << (28 * k)) - 1, (1 << (28 * k)) + 1) if v < p]
    rinv = pow(c.Rq, -1, p)
    vals = special + [w * rinv % p for w in special]  # boundary words = w
    rnd = random.Random(SEED + 28)
    vals += [rnd.randrange(p) for _ in range(64)]
    vals += [0] * (-len(vals) % 12)
    return vals


# ---- boundary limbs of oracle values ----------------------------------------------------------------------------------
def point_limbs(cname, pt, group):
    """uint64 boundary limbs (tests/gsutil.py) of an oracle point; the identity is all zero"""
    import numpy as np

    c = curve(cname)
    if pt is None:
        return np.zeros((2 if group == 1 else 4) * c.nq, dtype=np.uint64)
    return np.concatenate([c.fq(v) for v in coords_of(pt, group, False)])


def gt_limbs(cname, f):
    import numpy as np

    c = curve(cname)
    return np.concatenate([c.fq(v) for v in O.f12_flat(f)])


def expected_reasons(cname, group, compressed):
    """every reason dec_point can give for a byte string of the right length"""
    rs = ["non-canonical coordinate", "identity with non-zero coordinates"]
    rs.append("x is not on the curve" if compressed else "not on the curve")
    if cname == "bls12_381":
        rs.append("compression flag")
        # on an uncompressed string the sort flag is refused before the infinity flag is looked at
        rs.append("sort flag on the identity" if compressed else "sort flag on an uncompressed point")
    else:
        rs.append("flags")
        if not compressed:
            rs.append("sort flag does not match y")
    if not (cname == "bn254" and group == 1):
        rs.append("not in the prime-order subgroup")
    return rs


def selfcheck(cname):
    """The table is what it claims, from the oracle alone.  Returns {(group): [cofactor primes that yielded a point]}."""
    yielded = {}
    for group in (1, 2):
        tq = cofactor_points(cname, group)
        yielded[group] = sorted(tq)
        assert all(q in tq for q in MUST_YIELD[(cname, group)]), (cname, group, sorted(tq))
        assert all(q in [pq for pq, _ in cofactor_primes(cname, group)] for q in tq)
        if cname == "bn254" and group == 1:
            assert not tq and not cofactor_primes(cname, group)
        for compressed in (True, False):
            cases = point_cases(cname, group, compressed)
            assert len(cases) < 400 and len({k.name for k in cases}) == len(cases) == len({k.data for k in cases})
            why = Counter(k.why_v for k in cases if not k.ok_v)
            want = expected_reasons(cname, group, compressed)
            assert set(why) == set(want), (cname, group, compressed, why)
            assert all(why[r] >= 2 for r in want), (cname, group, compressed, why)
            # without validation the only difference is the subgroup test
            for k in cases:
                assert (k.ok_nv and not k.ok_v) == (k.why_v == "not in the prime-order subgroup"), k.name
                assert k.ok_nv or k.why_nv == k.why_v, k.name
            if cname == "bn254" and group == 1:
                assert all(k.ok_v == k.ok_nv for k in cases)  # every curve point is accepted
            vals = [k.value for k in cases if k.ok_nv]
            assert len(set(vals)) == len(vals), (cname, group, compressed)
            # the cofactor classes: T_q has order q, the mixed points order q r; all rejected, all decodable
            labels = Counter(k.label for k in cases)
            for q, t in tq.items():
                assert labels[q] == 4, (cname, group, q)
            for k in cases:
                if k.name.startswith("cof/"):
                    assert k.ok_nv and not k.ok_v, k.name
                if k.name.startswith("cof/S"):
                    q = k.label
                    assert O.ec_mul(fld(group), q, k.value) is not None and O.ec_mul(fld(group), O.R, k.value) is not None
                    assert O.ec_mul(fld(group), q * O.R, k.value) is None
                if k.name.startswith(("sub/", "beta.x", "neg-y")) or (k.name == "sort-flipped" and compressed):
                    assert k.ok_v, k.name
                if k.name.startswith("off/"):
                    assert not k.ok_nv, k.name
            if group == 2 and compressed:
                br = Counter(k.label for k in cases if k.name.startswith("sqrt/"))
                assert all(br[b] >= 2 for b in SQRT_BRANCHES), br
                for k in cases:
                    if k.name.startswith("sqrt/"):
                        assert k.ok_nv == (k.label != "no-norm"), k.name
                        if k.label == "real":
                            assert k.value[1][1] == 0 and k.value[1][0] != 0
                        if k.label == "imaginary":
                            assert k.value[1][0] == 0 and k.value[1][1] != 0
    if cname == "bls12_381":  # the order-3 point is one bit away from the identity's encoding
        c3 = [k for k in point_cases(cname, 1, True) if k.ok_nv and k.value is not None and k.value[0] == 0]
        assert len(c3) == 2 and all(k.ok_nv and not k.ok_v and k.value[0] == 0 for k in c3)
        assert {k.value[1] for k in c3} == {2, O.P - 2}
    fr = fr_cases(cname)
    assert Counter(k.why for k in fr)["non-canonical Fr"] >= 2 and sum(k.ok for k in fr) >= 32
    gt = gt_cases(cname)
    why = Counter(k.why_v for k in gt if not k.ok_v)
    assert why["non-canonical Fq"] >= 2 and why["GT element not in the r-torsion"] >= 2
    byname = {k.name: k for k in gt}
    for nm in ("-1", "-gt", "fp-2", "cube-root-of-unity", "cyclotomic-not-torsion", "junk"):
        assert byname[nm].ok_nv and not byname[nm].ok_v, nm
    for nm in ("one", "gt", "gt^2", "gt^(r-1)"):
        assert byname[nm].ok_v, nm
    vals = [k.value for k in gt if k.ok_nv]
    assert len(set(vals)) == len(vals)
    assert len(enc_fq_values(cname)) % 12 == 0
    return yielded

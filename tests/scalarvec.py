"""Named scalars for everything that turns an Fr scalar into digit streams -- limb_divmod_const (Barrett division by
lambda and by |x|), endo_lattice (Babai rounding, BN254), recode_w4 / recode_w4_limbs / recode_w_limbs (signed windows),
shared_digits, the unsigned 16-bit windows of k_fix and the bit loop of k_gt_pow (csrc/gs_curve.cuh, csrc/gs_kernels.cuh).
tests/test_scalar_decomp.py runs the table on the CPU twin, tests/test_gpu_scalar_edges.py on the device.

Pure Python, deterministic (one seed), no engine import.  A small big-integer MODEL of each decomposition lives here; it
is used to CLASSIFY a scalar (which Barrett correction count it takes, which sign pattern, which digits it produces) and
to compare the twin's digit streams with, never to say what a group operation must return: those expectations come from
oracle/gs_oracle.py and oracle/gs_ref.c.  The constants are read from csrc/gs_params_<curve>.h.

  table(cname)              [Case(name, k, classes)], every k canonical (< r), unique by value
  scalars(cname, cls)       the k of one class (or of all)
  decompose(cname, g, k)    Decomp(mags, signs, exact, label): the sub-scalars of group g as the device forms them
  stream_digits(...)        signed width-W digits of every stream, plain_digits(k) those of recode_w4
  selfcheck(cname)          the classes are really in the table; returns the reached correction counts / sign patterns

Classes: universal, window16, exponent, and per curve bls_g1 / bls_g2 / bls_w8 / bn_g1 / bn_g2 (DESIGN.md 4.1 has the
prose)."""
import functools
import os
import random
import re
from collections import namedtuple

from gsutil import REPO, curve

SEED = 20241018
CURVES = ["bls12_381", "bn254"]
SEARCH = 1 << 17  # candidates of every seeded model search
Case = namedtuple("Case", "name k classes")
Decomp = namedtuple("Decomp", "mags signs exact label")


# ---- constants of the generated headers ---------------------------------------------------------------------------------
def _param(cname, name):
    """an integer array of csrc/gs_params_<curve>.h, nested as declared"""
    with open(os.path.join(REPO, "groth_sahai_rs_amd", "csrc", "gs_params_%s.h" % cname)) as f:
        m = re.search(r"\b%s((?:\[\d+\])+) = (\{.*?\});" % name, f.read())
    dims = [int(d) for d in re.findall(r"\[(\d+)\]", m.group(1))]
    flat = [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(2))]

    def nest(v, ds):
        if len(ds) == 1:
            assert len(v) == ds[0]
            return v
        step = len(v) // ds[0]
        return [nest(v[i * step:(i + 1) * step], ds[1:]) for i in range(ds[0])]

    return nest(flat, dims)


def _int(limbs):
    return sum(int(x) << (32 * i) for i, x in enumerate(limbs))


class Model:
    """The decompositions of csrc/gs_curve.cuh on big integers."""

    def __init__(self, cname):
        c = curve(cname)
        self.name, self.r, self.p, self.bn = cname, c.r, c.p, cname == "bn254"
        self.nbits = self.r.bit_length()
        self.NS = {1: 2, 2: 4}
        if self.bn:
            self.NL = {1: 5, 2: 3}
            self.lat = {}
            for g, tag in ((1, "GLV1"), (2, "GLS2")):
                G = [_int(v) for v in _param(cname, tag + "_G")]
                GS = _param(cname, tag + "_GS")
                Bm, BS = _param(cname, tag + "_B"), _param(cname, tag + "_BS")
                B = [[(-1 if BS[i][j] else 1) * _int(Bm[i][j]) for j in range(len(G))] for i in range(len(G))]
                self.lat[g] = (G, GS, B, len(_param(cname, tag + "_G")[0]))
            B1 = self.lat[1][2]
            # the G1 eigenvalue is not a constant of the header: every basis row has b0 + b1 lambda = 0 (mod r)
            self.eig = {1: -B1[0][0] * pow(B1[0][1], -1, self.r) % self.r, 2: self.p % self.r}
            self.subbits = {1: int(self._scalar("GLV1_SUBBITS")), 2: int(self._scalar("GLS2_SUBBITS"))}
        else:
            self.NL = {1: 4, 2: 2}
            self.lam = _int(_param(cname, "LAMBDA"))
            self.xabs = _int(_param(cname, "XABS_LIMBS"))
            self.eig = {1: self.lam, 2: self.r - self.xabs}  # psi acts as x = -|x|

    def _scalar(self, name):
        with open(os.path.join(REPO, "groth_sahai_rs_amd", "csrc", "gs_params_%s.h" % self.name)) as f:
            return re.search(r"\b%s = (\d+);" % name, f.read()).group(1)

    @staticmethod
    def barrett(n, D, NN, ND):
        """limb_divmod_const<NN, ND>: (quotient, remainder, corrections).  corrections = 3 stands for a remainder that is
        still >= D after the two corrections the routine makes (a wrong result)."""
        mu = (1 << (32 * NN)) // D
        qh = (n * mu) >> (32 * NN)
        assert qh < 1 << (32 * (NN - ND + 2))
        rem = (n - qh * D) % (1 << (32 * (ND + 1)))
        corr = 0
        for _ in range(2):
            if rem >= D:
                rem, qh, corr = rem - D, qh + 1, corr + 1
        if rem >= D:
            corr = 3
        return qh, rem, corr

    def decompose(self, group, k):
        """mags: what the device hands to the recoder (NL limbs each); signs: 1 = the stream enters negated; exact: the
        signed sub-scalars as integers; label: the Barrett correction counts (BLS12-381) or the sign pattern (BN254)"""
        if self.bn:
            G, GS, B, gw = self.lat[group]
            n = len(G)
            c = [((k * G[i]) >> 256) % (1 << (32 * gw)) * (-1 if GS[i] else 1) for i in range(n)]
            exact = [(k if j == 0 else 0) - sum(c[i] * B[i][j] for i in range(n)) for j in range(n)]
            acc = [v % (1 << 320) for v in exact]  # 10 words, two's complement
            signs = [a >> 319 for a in acc]
            mags = [((1 << 320) - a if s else a) % (1 << (32 * self.NL[group])) for a, s in zip(acc, signs)]
            return Decomp(mags, signs, exact, tuple(signs))
        if group == 1:
            q, k1, corr = self.barrett(k, self.lam, 8, 4)
            return Decomp([k1, q % (1 << 128)], [0, 0], [k1, q], (corr,))
        n, d, corrs = k, [], []
        for _ in range(3):
            n, rem, corr = self.barrett(n, self.xabs, 8, 2)
            d.append(rem)
            corrs.append(corr)
        d.append(n % (1 << 64))
        return Decomp(d, [0, 1, 0, 1], d[:3] + [n], tuple(corrs))

    def recombine(self, group, mags, signs):
        """sum +-mag_j eig^j mod r: k, if the decomposition is right"""
        return sum((-m if s else m) * pow(self.eig[group], j, self.r) for j, (m, s) in enumerate(zip(mags, signs))) % self.r


@functools.lru_cache(maxsize=None)
def model(cname):
    return Model(cname)


def decompose(cname, group, k):
    return model(cname).decompose(group, k)


def nd_of(NL, W):
    return (32 * NL + W - 1) // W + 1


def recode(mag, NL, W):
    """recode_w_limbs<NL, W> (and recode_w4_limbs<NL> at W = 4): signed digits in [-2^(W-1), 2^(W-1)), the last one spare"""
    out, carry = [], 0
    for i in range(nd_of(NL, W)):
        bit = i * W
        v = ((mag >> bit) & ((1 << W) - 1) if bit < 32 * NL else 0) + carry
        if v >= 1 << (W - 1):
            out.append(v - (1 << W))
            carry = 1
        else:
            out.append(v)
            carry = 0
    return out


def plain_digits(k, nbits):
    """recode_w4 on the whole 256-bit scalar: (nbits + 3) / 4 + 1 digits"""
    out, carry = [], 0
    for i in range((nbits + 3) // 4 + 1):
        v = ((k >> (4 * i)) & 15 if 4 * i < 256 else 0) + carry
        if v >= 8:
            out.append(v - 16)
            carry = 1
        else:
            out.append(v)
            carry = 0
    return out


def stream_digits(cname, group, k, W):
    m = model(cname)
    return [recode(mag, m.NL[group], W) for mag in m.decompose(group, k).mags]


def spare_threshold(ND, W):
    """the smallest magnitude whose last (spare) digit is 1: one more than the largest value ND - 1 digits below
    2^(W-1) can hold"""
    return sum(((1 << (W - 1)) - 1) << (W * i) for i in range(ND - 1)) + 1


# ---- the table --------------------------------------------------------------------------------------------------------
def _cut(v, r, step):
    """a pattern `truncated below r`: top windows dropped until it is canonical"""
    while v >= r:
        v >>= step
    return v


def _rep(pattern, total):
    """`pattern` (a bit string) repeated from bit 0 upwards over `total` bits"""
    s = pattern * (total // len(pattern) + 1)
    return int(s[len(s) - total:], 2)


@functools.lru_cache(maxsize=None)
def _search(cname, group):
    """The seeded search of SEARCH random scalars: {label: [first scalars that took it]}, and for BN254 the scalars with
    the longest sub-scalar of every stream."""
    m = model(cname)
    rnd = random.Random(SEED + 17 * group + (1000 if m.bn else 0))
    by_label, longest = {}, [[] for _ in range(m.NS[group])]
    for _ in range(SEARCH):
        k = rnd.randrange(m.r)
        d = m.decompose(group, k)
        by_label.setdefault(d.label, [])
        if len(by_label[d.label]) < 4:
            by_label[d.label].append(k)
        if m.bn:
            for j, v in enumerate(d.exact):
                longest[j].append((abs(v), k))
                if len(longest[j]) > 64:
                    longest[j] = sorted(longest[j], reverse=True)[:4]
    longest = [sorted(lst, reverse=True)[:4] for lst in longest]
    return by_label, longest


def reached(cname, group):
    """BLS12-381: per division stage the set of correction counts the search reached; BN254: the set of sign patterns"""
    labels = _search(cname, group)[0]
    if model(cname).bn:
        return sorted(labels)
    stages = len(next(iter(labels)))
    return [sorted({lab[s] for lab in labels}) for s in range(stages)]


def _universal(m):
    r, nb = m.r, m.nbits
    out = [("zero", 0), ("one", 1), ("two", 2), ("r-1", r - 1), ("r-2", r - 2), ("(r-1)/2", (r - 1) // 2),
           ("(r+1)/2", (r + 1) // 2)]
    for i in range(1, nb + 1):
        if any(i % s == 0 for s in (4, 5, 8, 16, 32)):
            if 1 << i < r:
                out.append(("2^%d" % i, 1 << i))
            if (1 << i) - 1 < r:
                out.append(("2^%d-1" % i, (1 << i) - 1))
    for pat in ("8", "7", "F", "08", "F0", "0F"):
        bits = "".join(format(int(ch, 16), "04b") for ch in pat)
        out.append(("nibbles_%s" % pat, _cut(_rep(bits, 256), r, 4)))
    for pat in ("10000", "01111", "11111"):
        out.append(("quints_%s" % pat, _cut(_rep(pat, 255), r, 5)))
    # the plain path (recode_w4 on the whole scalar): its spare digit is 1 from 0x788..8 upwards, which is above r on
    # both curves (selfcheck proves it), so no canonical scalar sets it.  What can be had: a carry that runs through
    # every nibble into the top one, below and at the top nibble of r.
    top = (r >> 252) & 15
    out.append(("plain_carry_chain_below_top", ((top - 1) << 252) | int("8" * 63, 16)))
    out.append(("plain_carry_chain_cut", _cut((top << 252) | int("8" * 63, 16), r, 4)))
    out.append(("plain_top_nibble_neg8_chain", int("7" + "8" * 62, 16)))
    return out


def _window16(m):
    r = m.r
    out = []
    for w in range(16):
        for d in (1, 0x00FF, 0x0100, 0xFF00, 0xFFFF):
            if d << (16 * w) < r:
                out.append(("win16_%d_%04x" % (w, d), d << (16 * w)))
    for pat in ("ff00", "0100", "8000"):
        out.append(("win16_lowbytes_zero_%s" % pat, _cut(int(pat * 16, 16), r, 16)))
    for pat in ("00ff", "0001", "0080"):
        out.append(("win16_highbytes_zero_%s" % pat, _cut(int(pat * 16, 16), r, 16)))
    return out


def _exponent(m):
    nb = m.nbits
    out = []
    for n in range(5):
        unit = "1" + "0" * n
        s = (unit * (nb // len(unit) + 1))[:nb - 2] + "1"  # nb - 1 bits: below 2^(nb-1) <= r
        out.append(("exp_run_1_0^%d_1" % n, int(s, 2)))
    out.append(("exp_top_bit", 1 << (nb - 1)))
    out.append(("exp_bottom_bit", 1))
    return out


def _bls_g1(m):
    lam, r = m.lam, m.r
    pats = lambda hi: [("8s", _cut(int("8" * 32, 16), hi + 1, 4)), ("7s", _cut(int("7" * 32, 16), hi + 1, 4)),
                       ("Fs", _cut(int("F" * 32, 16), hi + 1, 4))]
    qs = [("0", 0), ("1", 1), ("2", 2), ("max", lam)] + pats(lam)
    ss = [("0", 0), ("1", 1), ("2", 2), ("max", lam - 1)] + pats(lam - 1)
    out = []
    for qn, q in qs:
        for sn, s in ss:
            out.append(("g1_q%s_s%s" % (qn, sn), q * lam + s))
    out.append(("g1_q(max+1)_s0", (lam + 1) * lam))  # = r - 1
    for sn, s in ss[1:]:
        out.append(("g1_k1=k2=%s" % sn, s * lam + s))
    by_label, _ = _search(m.name, 1)
    for (corr,), ks in sorted(by_label.items()):
        for i, k in enumerate(ks):
            out.append(("g1_corr%d_#%d" % (corr, i), k))
    rnd = random.Random(SEED + 1)
    for i in range(4):
        q = rnd.randrange(3, lam)
        out.append(("g1_multiple_#%d" % i, q * lam))
        out.append(("g1_multiple_pred_#%d" % i, q * lam - 1))
    assert all(k < r for _, k in out)
    return out


def _bls_g2(m):
    x, r = m.xabs, m.r
    d3max = (r - 1) // x ** 3
    V = [0, 1, x - 1, 0x7777777777777777, 0x8888888888888888]
    assert all(v < x for v in V)

    def compose(d):
        d = list(d)
        d[3] = min(d[3], d3max)
        k = sum(v * x ** j for j, v in enumerate(d))
        if k >= r:  # only with the top digit at its limit
            d[3] -= 1
            k = sum(v * x ** j for j, v in enumerate(d))
        return k

    out = []
    for v in V:
        out.append(("g2_all_digits_%x" % v, compose([v] * 4)))
    for j in range(4):
        for v in V[1:]:
            out.append(("g2_only_d%d=%x" % (j, v), compose([v if i == j else 0 for i in range(4)])))
    for s in range(5):  # every value at every position
        out.append(("g2_cycle_%d" % s, compose([V[(j + s) % 5] for j in range(4)])))
        out.append(("g2_cycle_rev_%d" % s, compose([V[(s - j) % 5] for j in range(4)])))
    by_label, _ = _search(m.name, 2)
    for stage in range(3):
        for corr in sorted({lab[stage] for lab in by_label}):
            ks = [k for lab, lst in sorted(by_label.items()) if lab[stage] == corr for k in lst][:4]
            for i, k in enumerate(ks):
                out.append(("g2_stage%d_corr%d_#%d" % (stage, corr, i), k))
    rnd = random.Random(SEED + 2)
    for i in range(4):  # exact multiples of |x|, |x|^2, |x|^3 and their predecessors: a correction in every stage
        q = rnd.randrange(3, d3max)
        for e in (1, 2, 3):
            k = (q * x ** 3 + rnd.randrange(x ** 3)) // x ** e * x ** e
            out.append(("g2_multiple_x^%d_#%d" % (e, i), k))
            out.append(("g2_multiple_x^%d_pred_#%d" % (e, i), k - 1))
    assert all(0 <= k < r for _, k in out)
    return out


def _bls_w8(m):
    """8-bit windows (k_var_tab8): the largest digit, +127, in the two upper base-|x| streams of G2, which no other class
    puts there twice -- a lone 0x7f in window 0 and in window 1 of d2 and of d3"""
    x = m.xabs
    out = [("g2_w8_d%d=%x" % (j, v), v * x ** j) for j in (2, 3) for v in (0x7F, 0x7F00)]
    assert all(k < m.r for _, k in out)
    return out


def _bn(m, group):
    r = m.r
    G, GS, B, gw = m.lat[group]
    tag = "bn_g%d" % group
    out = []
    by_label, longest = _search(m.name, group)
    for lab, ks in sorted(by_label.items()):
        for i, k in enumerate(ks[:2]):
            out.append(("%s_signs_%s_#%d" % (tag, "".join("-" if s else "+" for s in lab), i), k))
    for i, g in enumerate(G):
        jmax = ((r - 1) * g) >> 256
        for jn, j in (("first", 1), ("middle", max(jmax // 2, 1)), ("last", jmax)):
            k = -((-j << 256) // g)  # ceil(j 2^256 / G_i): the first k with c_i = j
            assert k < r and (k * g) >> 256 == j and ((k - 1) * g) >> 256 == j - 1
            out.append(("%s_c%d_step_%s" % (tag, i, jn), k))
            out.append(("%s_c%d_step_%s_pred" % (tag, i, jn), k - 1))
    for j, lst in enumerate(longest):
        for i, (_, k) in enumerate(lst):
            out.append(("%s_longest_stream%d_#%d" % (tag, j, i), k))
    small = -((-1 << 256) // max(G)) - 1  # the largest k with every c_i = 0
    for name, k in (("max", small), ("half", small >> 1), ("8s", _cut(int("8" * 64, 16), small + 1, 4))):
        assert all((k * g) >> 256 == 0 for g in G)
        out.append(("%s_all_c_zero_%s" % (tag, name), k))
    return out


@functools.lru_cache(maxsize=None)
def _build(cname):
    m = model(cname)
    parts = [("universal", _universal(m)), ("window16", _window16(m)), ("exponent", _exponent(m))]
    if m.bn:
        parts += [("bn_g1", _bn(m, 1)), ("bn_g2", _bn(m, 2))]
    else:
        parts += [("bls_g1", _bls_g1(m)), ("bls_g2", _bls_g2(m)), ("bls_w8", _bls_w8(m))]
    by_value, order, names = {}, [], {}
    for cls, lst in parts:
        for name, k in lst:
            assert 0 <= k < m.r and names.get(name, k) == k, (name, hex(k))
            names[name] = k
            if k in by_value:
                if cls not in by_value[k][1]:
                    by_value[k][1].append(cls)
            else:
                by_value[k] = (name, [cls])
                order.append(k)
    return [Case(by_value[k][0], k, tuple(by_value[k][1])) for k in order], names


def table(cname):
    """the cases, unique by value: a scalar that several builders produce keeps its first name and joins every class"""
    return _build(cname)[0]


def by_name(cname):
    """{name: k} with every name a builder gave, those of merged duplicates included"""
    return _build(cname)[1]


def scalars(cname, cls=None):
    return [c.k for c in table(cname) if cls is None or cls in c.classes]


def name_of(cname, k):
    for c in table(cname):
        if c.k == k:
            return c.name
    return hex(k)


# ---- what the table must hold -------------------------------------------------------------------------------------------
def stream_bound(cname, group, s):
    """an upper bound of stream s's magnitude: exact on BLS12-381, 2^(SUBBITS + 1) on BN254 (SUBBITS is the measured
    length; the extra bit is the slack the slots are sized with)"""
    m = model(cname)
    if m.bn:
        return 1 << (m.subbits[group] + 1)
    if group == 1:
        return (m.lam - 1, m.lam + 1)[s]
    return m.xabs - 1 if s < 3 else (m.r - 1) // m.xabs ** 3


def selfcheck(cname):
    """Every class is there, every reached correction count / sign pattern has its scalars, and every stream sees the
    most negative digit and a carry past its top window, at the widths 4, 5 and 8; at W = 8 the largest digit as well,
    twice.  Returns the reached sets."""
    m = model(cname)
    tab = table(cname)
    ks = [c.k for c in tab]
    assert len(tab) < 700 and len(set(ks)) == len(ks) and all(0 <= k < m.r for k in ks)
    classes = ["universal", "window16", "exponent"] + (["bn_g1", "bn_g2"] if m.bn else ["bls_g1", "bls_g2", "bls_w8"])
    for cls in classes:
        assert scalars(cname, cls), cls
    out = {}
    for group in (1, 2):
        NL, NS = m.NL[group], m.NS[group]
        decs = [m.decompose(group, k) for k in ks]
        for k, d in zip(ks, decs):
            # the model against plain integer arithmetic: it classifies, so it had better be right
            assert m.recombine(group, d.mags, d.signs) == k, (group, hex(k))
            assert all(abs(v) < 1 << (32 * NL) for v in d.exact), (group, hex(k))
            if not m.bn:
                assert 3 not in d.label, (group, hex(k))
                if group == 1:
                    assert (d.exact[1], d.exact[0]) == divmod(k, m.lam)
                else:
                    assert sum(v * m.xabs ** j for j, v in enumerate(d.exact)) == k and all(v < m.xabs for v in d.exact[:3])
        labels = {d.label for d in decs}
        by_label, longest = _search(cname, group)
        if m.bn:
            assert set(by_label) <= labels
            for lab in by_label:
                assert sum(1 for d in decs if d.label == lab) >= min(2, len(by_label[lab])), lab
            for j, lst in enumerate(longest):
                assert all(k in ks for _, k in lst)
                assert lst[0][0].bit_length() <= m.subbits[group], (group, j, lst[0][0].bit_length())
            G = m.lat[group][0]
            assert any(all((k * g) >> 256 == 0 for g in G) and k > 2 for k in ks)
            for s in range(NS):
                assert any(d.exact[s] == 0 and (k or s == 0) for k, d in zip(ks, decs)), (group, s)
        else:
            for stage, counts in enumerate(reached(cname, group)):
                for cnt in counts:
                    assert sum(1 for d in decs if d.label[stage] == cnt) >= 4, (group, stage, cnt)
            for s in range(NS):
                assert any(d.mags[s] == 0 and k for k, d in zip(ks, decs)), (group, s)
            if group == 1:
                assert any(d.mags[0] == d.mags[1] != 0 for d in decs)
                assert any(k and k % m.lam == 0 for k in ks) and any((k + 1) % m.lam == 0 for k in ks)
            else:
                assert any(len(set(d.mags)) == 1 and d.mags[0] for d in decs)
                for s in range(NS):
                    assert any(d.mags[s] and sum(1 for v in d.mags if v) == 1 for d in decs), s
        out[group] = reached(cname, group)
        # digits: -2^(W-1) in every stream; a carry past the top window of the value in every stream; the spare digit
        # itself wherever the stream's range lets a magnitude reach it
        for W in (4, 5, 8):
            ND = nd_of(NL, W)
            for s in range(NS):
                streams = [recode(d.mags[s], NL, W) for d in decs]
                assert any(-(1 << (W - 1)) in dg for dg in streams), (group, W, s)
                assert any(d.mags[s] and max(i for i, v in enumerate(dg) if v) >= -(-d.mags[s].bit_length() // W)
                           for d, dg in zip(decs, streams)), (group, W, s)
                can = stream_bound(cname, group, s) >= spare_threshold(ND, W)
                assert any(dg[-1] == 1 for dg in streams) == can, (group, W, s, can)
                assert all(dg[-1] in (0, 1) for dg in streams)
                if W == 8:  # (the widths 4 and 5 get their largest digit from the repeated nibbles and quintets)
                    assert sum(1 for dg in streams if 127 in dg) >= 2, (group, s)
    # the plain path: digit -8, the carry chain into the top nibble, and the proof that the spare digit stays 0
    nd = (m.nbits + 3) // 4 + 1
    assert spare_threshold(nd, 4) > m.r - 1
    plain = [plain_digits(k, m.nbits) for k in ks]
    assert any(-8 in dg for dg in plain) and all(dg[-1] == 0 for dg in plain)
    assert any(dg[nd - 2] == ((m.r >> 252) & 15) and (k >> 252) & 15 == ((m.r >> 252) & 15) - 1 for k, dg in zip(ks, plain))
    # 16-bit windows: every window alone at every d that fits, all low / all high bytes zero
    for w in range(16):
        for d in (1, 0x00FF, 0x0100, 0xFF00, 0xFFFF):
            assert (d << (16 * w) in ks) == (d << (16 * w) < m.r), (w, d)
    wins = lambda k: [(k >> (16 * w)) & 0xFFFF for w in range(16)]
    assert any(k and all(v & 0xFF == 0 for v in wins(k)) and sum(1 for v in wins(k) if v) > 8 for k in ks)
    assert any(k and all(v >> 8 == 0 for v in wins(k)) and sum(1 for v in wins(k) if v) > 8 for k in ks)
    # exponent runs: zero runs of 0 .. 4 between ones, and the lone top / bottom bits
    for n in range(5):
        assert any(("1" + "0" * n) * 3 + "1" in bin(k) and "0" * (n + 1) not in bin(k)[2:] for k in ks), n
    assert 1 << (m.nbits - 1) in ks and 1 in ks
    return out

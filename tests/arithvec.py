"""Adversarial operands for the lazy radix-2^28 arithmetic (csrc/gs_fq28.cuh and what is built on it), and the table of
operations that tests/test_mul28_gen.py (generated instruction streams on the CPU), tests/test_twin.py (the headers
compiled for the host with every contract assertion on) and tests/test_gpu_arith.py (the device code itself) run on them.
Pure Python, deterministic (one seed), big integers throughout.

Operands are raw INTERNAL limb vectors (int32 x L, V = sum v[i] 2^(28 i), element = V / 2^(28 L) mod p), so a case fixes
the lazy REPRESENTATION and not only the field element:

  * column extremes (`multiplier_cases`): for every multiplier body -- product, squaring, Fp2 product, Fp2 squaring,
    three-pair Fp2 dot product -- operands at the body's documented limb limit with the sign pattern that makes every
    term of a column add up.  Tier 1 has the top limb at 2^26 - 1 (what the CPU twin's contract check admits), tier 2
    has |V| < 2^(28L-6) (the value contract of the header).  "A = 8" means 2^31 - 1: limbs are int32.
  * value edges, zero tests, vreduce inputs next to half-integer quotients, inversion inputs, boundary inputs that take
    each branch of fq_to_boundary, N-form tower and curve inputs with every limb at the largest value a multiplier or a
    carry round can leave -- see the functions below.
  * seeded random vectors per class, lazily perturbed within contract.

`selfcheck()` (run by test_mul28_gen.py) proves the labels: every vector is inside the contract it is labelled with,
the label is inside the body's contract (asserted again by `op_cases` on every case it hands out), and for each body the largest |sum of product terms of one column| that the
big-integer model reaches over the set EQUALS the largest the labelled bounds allow, computed here from those bounds
column by column.  That equality is what makes the vectors extreme and not merely large.  The Montgomery reduction
terms m_i p_j depend on p and come on top; with them the largest |column accumulator| reached, as a fraction of 2^63:

    body       bls12_381 (L = 14)   bn254 (L = 10)
    mul             0.8598               0.5838
    sqr             0.8598               0.5823
    fp2mul          0.8468               0.5688
    fp2sqr          0.8468               0.5688
    fp2dot3         0.8468               0.5785

(`selfcheck` asserts these figures to the four digits printed.)  The closest documented bound to its limit is the single
product / squaring on BLS12-381 at A_a A_b = 8: 86.0 % of the accumulator.  The "~1.5 % to spare" of the generator's
comment is for limbs at the full bound in EVERY term of the longest column; the top limbs, capped at 2^26 by the value
contract, take two terms out of it, and the longest full-size column is the one below (L - 1 terms).
"""
import math
import os
import random
import re
import sys

from gsutil import REPO, curve

M28 = (1 << 28) - 1
LIMBS = {"bls12_381": 14, "bn254": 10}
TOP1 = (1 << 26) - 1   # tier 1: the top-limb bound of the multiplier contract (fq28_check: |top| < 2^26)
TOP2 = (1 << 22) - 16  # tier 2: with lower limbs up to 2^31 in magnitude this keeps |V| < 2^(28L-6)
NMAX, NMIN = (1 << 28) + 6, -8  # "N" limbs: what one carry round of int32 limbs can leave ((x & M28) + (y >> 28))
SEED = 20240917

REACHED = {  # largest |column accumulator| / 2^63 per body and curve (the table of the docstring)
    "bls12_381": {"mul": "0.8598", "sqr": "0.8598", "fp2mul": "0.8468", "fp2sqr": "0.8468", "fp2dot3": "0.8468"},
    "bn254": {"mul": "0.5838", "sqr": "0.5823", "fp2mul": "0.5688", "fp2sqr": "0.5688", "fp2dot3": "0.5785"},
}


def _param_array(cname, name):
    """an int array of csrc/gs_params_<curve>.h (the constants the device multiplies by at its boundary)"""
    with open(os.path.join(REPO, "groth_sahai_rs_amd", "csrc", "gs_params_%s.h" % cname)) as f:
        m = re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, f.read())
    return [int(x, 0) for x in m.group(1).split(",")]


class Ctx:
    def __init__(self, cname):
        c = curve(cname)
        self.name, self.p, self.L = cname, c.p, LIMBS[cname]
        self.R = 1 << (28 * self.L)
        self.Rinv = pow(self.R, -1, self.p)
        self.pinvR = pow(self.p, -1, self.R)
        self.P28 = [(self.p >> (28 * i)) & M28 for i in range(self.L)]
        self.ninv = (-pow(self.p, -1, 1 << 28)) % (1 << 28)
        self.N = 2 * c.nq  # u32 words of the boundary form
        self.Rb = 1 << (32 * self.N)
        self.K_OUT28 = _param_array(cname, "K_OUT28")
        self.xi = (1, 1) if cname == "bls12_381" else (9, 1)
        self.golden = c.golden

    def val(self, v):
        return sum(int(x) << (28 * i) for i, x in enumerate(v))

    def fe(self, v):
        return self.val(v) * self.Rinv % self.p

    def limbs(self, V):
        """the unique limbs of the integer V: 0..L-2 in [0, 2^28), top signed"""
        return [(V >> (28 * i)) & M28 for i in range(self.L - 1)] + [V >> (28 * (self.L - 1))]

    def enc(self, x):
        return self.limbs(x * self.R % self.p)

    def mont(self, W):
        """the integer a Montgomery reduction of the double-length integer W returns: (W + m p) / R, 0 <= m < R"""
        m = (-W * self.pinvR) % self.R
        return (W + m * self.p) >> (28 * self.L)

    def words(self, x):
        """boundary form of the canonical x: u32 words of x 2^(32N) mod p"""
        w = x * self.Rb % self.p
        return [(w >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]

    def unwords(self, w):
        return sum((int(x) & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(w)) * pow(self.Rb, -1, self.p) % self.p


_CTX = {}


def ctx(cname):
    if cname not in _CTX:
        _CTX[cname] = Ctx(cname)
    return _CTX[cname]


def s32ok(v):
    return all(-(1 << 31) <= x < (1 << 31) for x in v)


def norm(v):
    """one parallel carry round (gs_fq28.cuh norm) on Python integers"""
    L = len(v)
    return [v[0] & M28] + [(v[i] & M28) + (v[i - 1] >> 28) for i in range(1, L - 1)] + [v[L - 1] + (v[L - 2] >> 28)]


def carry(v, rnd, amp, keep=None):
    """the same integer in other limbs: c 2^28 moved from limb i to limb i + 1 for random |c| <= amp"""
    v = list(v)
    for i in range(len(v) - 1):
        c = rnd.randint(-amp, amp)
        if keep is not None and not keep(v[i] + (c << 28)):
            continue
        v[i] += c << 28
        v[i + 1] -= c
    return v


def n_form(c, V, rnd=None, hi=True):
    """the integer V in N limbs pushed to the edge of their range: lower limbs 2^28 + 0..6 (hi) or -8..-1 where the unique
    limb allows it, the carry taken from / given to the next limb"""
    v = c.limbs(V)
    for i in range(c.L - 1):
        if hi and v[i] <= 6:
            v[i] += 1 << 28
            v[i + 1] -= 1
        elif not hi and v[i] >= (1 << 28) - 8:
            v[i] -= 1 << 28
            v[i + 1] += 1
    return v


def n_extreme(c, sign_top, lo=NMAX, top=TOP2):
    """N limbs with EVERY lower limb at the edge of the range and the top limb at the value-contract limit"""
    return [lo] * (c.L - 1) + [sign_top * top]


# ---------------------------------------------------------------------------------------------------------------------
# big-integer model of the multiplier bodies: product scanning, one accumulator per output, with the statistics the
# self-check needs.  `terms` = [(x, y), ...]: the accumulator receives sum_t sum_(i+j=k) x_t[i] y_t[j] in column k.
# ---------------------------------------------------------------------------------------------------------------------
class Stat:
    def __init__(self):
        self.prod = 0  # largest |sum of the product terms of one column|
        self.acc = 0   # largest |accumulator| (products + reduction terms + carry from the column below)


def model_acc(c, terms, st=None):
    L, acc, m, r = c.L, 0, [0] * c.L, [0] * c.L
    for k in range(2 * L - 1):
        col = 0
        for i in range(max(0, k - L + 1), min(k, L - 1) + 1):
            j = k - i
            for x, y in terms:
                col += x[i] * y[j]
                assert -(1 << 63) <= acc + col < (1 << 63), "column accumulator leaves int64"
        acc += col
        for i in range(max(0, k - L + 1), min(k - 1, L - 1) + 1):
            acc += m[i] * c.P28[k - i]
        if k < L:
            m[k] = ((acc & M28) * c.ninv) & M28
            acc += m[k] * c.P28[0]
        else:
            r[k - L] = acc & M28
        assert -(1 << 63) <= acc < (1 << 63), "column accumulator leaves int64"
        if st is not None:
            st.prod, st.acc = max(st.prod, abs(col)), max(st.acc, abs(acc))
        acc >>= 28
    r[L - 1] = acc
    return r


def body_terms(body, ops):
    """the accumulators of a body as lists of terms"""
    neg = lambda v: [-x for x in v]
    if body == "mul":
        return [[(ops[0], ops[1])]]
    if body == "sqr":
        return [[(ops[0], ops[0])]]
    if body == "fp2mul":
        a0, a1, b0, b1 = ops
        return [[(a0, b0), (neg(a1), b1)], [(a0, b1), (a1, b0)]]
    if body == "fp2sqr":
        a0, a1 = ops
        s, d, t = [x + y for x, y in zip(a0, a1)], [x - y for x, y in zip(a0, a1)], [2 * x for x in a1]
        assert s32ok(s) and s32ok(d) and s32ok(t), "operand sums leave int32"
        return [[(s, d)], [(a0, t)]]
    if body == "fp2dot3":
        t0, t1 = [], []
        for t in range(3):
            a0, a1, b0, b1 = ops[4 * t:4 * t + 4]
            t0 += [(a0, b0), (neg(a1), b1)]
            t1 += [(a0, b1), (a1, b0)]
        return [t0, t1]
    raise KeyError(body)


def model(c, body, ops, stats=None):
    """the limb vectors the body returns, by the big-integer model"""
    accs = body_terms(body, ops)
    return [model_acc(c, t, None if stats is None else stats[i]) for i, t in enumerate(accs)]


def exact(c, body, ops):
    """the same from the VALUES alone: the Montgomery reduction of the exact double-length integer"""
    V = [c.val(o) for o in ops]
    if body == "mul":
        W = [V[0] * V[1]]
    elif body == "sqr":
        W = [V[0] * V[0]]
    elif body == "fp2mul":
        W = [V[0] * V[2] - V[1] * V[3], V[0] * V[3] + V[1] * V[2]]
    elif body == "fp2sqr":
        W = [V[0] * V[0] - V[1] * V[1], 2 * V[0] * V[1]]
    else:
        W = [sum(V[4 * t] * V[4 * t + 2] - V[4 * t + 1] * V[4 * t + 3] for t in range(3)),
             sum(V[4 * t] * V[4 * t + 3] + V[4 * t + 1] * V[4 * t + 2] for t in range(3))]
    return [c.limbs(c.mont(w)) for w in W]


NOPS = {"mul": 2, "sqr": 1, "fp2mul": 4, "fp2sqr": 2, "fp2dot3": 12}
BODIES = list(NOPS)


class Case:
    def __init__(self, body, name, ops, kind, tier=1, bounds=None, attains=None):
        self.body, self.name, self.ops, self.kind, self.tier = body, name, ops, kind, tier
        self.bounds = bounds    # per operand: (bound on |limb i|, i < L - 1; bound on |top limb|); None = unlabelled
        self.attains = attains  # index of the accumulator whose analytical column maximum this case reaches


def in_contract(c, body, bounds):
    """the body's documented contract, on the labelled limb bounds"""
    L = c.L
    B = [b for b, _ in bounds]
    if any(t >= (1 << 26) for _, t in bounds) or any(b >= (1 << 31) for b in B):
        return False
    room = (1 << 63) - L * (1 << 56)  # L reduction terms m_i p_j < 2^56 per column
    if body == "mul":
        return L * B[0] * B[1] < room                          # A_a A_b <= 8
    if body == "sqr":
        return L * B[0] * B[0] < room and 2 * B[0] < (1 << 31)
    if body == "fp2mul":
        return 2 * L * max(B[0], B[1]) * max(B[2], B[3]) < room  # A_a A_b <= 4
    if body == "fp2sqr":
        return max(B) <= (1 << 29)                               # A <= 2
    return sum(2 * L * max(B[4 * t], B[4 * t + 1]) * max(B[4 * t + 2], B[4 * t + 3]) for t in range(3)) < room


def column_bound(c, body, bounds, which):
    """the largest |sum of the product terms of one column| of accumulator `which` that the labelled bounds allow"""
    L = c.L
    bv = [[b] * (L - 1) + [t] for b, t in bounds]
    conv = lambda x, y, k: sum(x[i] * y[k - i] for i in range(max(0, k - L + 1), min(k, L - 1) + 1))
    best = 0
    for k in range(2 * L - 1):
        if body == "mul":
            s = conv(bv[0], bv[1], k)
        elif body == "sqr":
            s = conv(bv[0], bv[0], k)
        elif body == "fp2mul":
            s = conv(bv[0], bv[2 + which], k) + conv(bv[1], bv[3 - which], k)
        elif body == "fp2dot3":
            s = sum(conv(bv[4 * t], bv[4 * t + 2 + which], k) + conv(bv[4 * t + 1], bv[4 * t + 3 - which], k) for t in range(3))
        elif which == 1:  # fp2sqr, c1 = a0 (2 a1)
            s = 2 * conv(bv[0], bv[1], k)
        else:
            # fp2sqr, c0 = sum (a0 + a1)_i (a0 - a1)_j: the terms (i, j) and (j, i) add up to 2 (a0_i a0_j - a1_i a1_j),
            # at most 4 b_i b_j for the pair; the diagonal term is a0^2 - a1^2, at most b^2
            b = [max(x, y) for x, y in zip(bv[0], bv[1])]
            s = sum(4 * b[i] * b[k - i] for i in range(max(0, k - L + 1), min(k, L - 1) + 1) if i < k - i)
            if k % 2 == 0 and k // 2 < L:
                s += b[k // 2] ** 2
        best = max(best, s)
    return best


def _ext(c, B, T, sign):
    return [sign * B] * (c.L - 1) + [sign * T]


def _pat(c, B, T, signs):
    return [s * B for s in signs[:-1]] + [signs[-1] * T]


def _extreme_cases(c):
    L = c.L
    out = []
    S = 1 << 28
    RT8 = math.isqrt(8 << 56)  # floor(2^28 sqrt 8) = 759250124
    for tier, T in ((1, TOP1), (2, TOP2)):
        tg = "t%d" % tier
        # product: A_a A_b <= 8 split 8 x 1, 1 x 8, 4 x 2, sqrt 8 squared; all +, all -, one operand negated
        for Ba, Bb in (((1 << 31) - 1, S), (S, (1 << 31) - 1), (1 << 30, 1 << 29), (RT8, RT8)):
            for sa, sb in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
                out.append(Case("mul", "%s.%dx%d.%+d%+d" % (tg, Ba, Bb, sa, sb), [_ext(c, Ba, T, sa), _ext(c, Bb, T, sb)],
                                "extreme", tier, [(Ba, T), (Bb, T)], 0))
        for sa in (1, -1):
            out.append(Case("sqr", "%s.%+d" % (tg, sa), [_ext(c, RT8, T, sa)], "extreme", tier, [(RT8, T)], 0))
        # Fp2 product: a0, b0, b1 at +max with a1 at -max makes every term of c0 add up; equal signs do it for c1
        for Ba, Bb in ((1 << 30, S), (1 << 29, 1 << 29), (S, 1 << 30)):
            bd = [(Ba, T), (Ba, T), (Bb, T), (Bb, T)]
            for nm, sg, att in (("c0+", (1, -1, 1, 1), 0), ("c0-", (-1, 1, 1, 1), 0), ("c1+", (1, 1, 1, 1), 1),
                                ("c1-", (-1, -1, 1, 1), 1), ("c0+b", (1, 1, 1, -1), 0), ("c1-b", (1, -1, 1, -1), 1)):
                ops = [_ext(c, b, T, s) for (b, _), s in zip(bd, sg)]
                out.append(Case("fp2mul", "%s.%dx%d.%s" % (tg, Ba, Bb, nm), ops, "extreme", tier, bd, att))
        # Fp2 squaring at A = 2.  c1 = 2 a0 a1: equal signs.  c0: with a1_i = +a0_i on one set of limbs and -a0_i on the other,
        # (a0 + a1)_i (a0 - a1)_j = 4 B^2 whenever i is in the first set and j in the second.  Alternating sets reach the
        # maximum of every ODD column; the split "below / above the middle of column k" reaches column k, even ones too.
        B = 1 << 29
        bd = [(B, T), (B, T)]
        plus = [1] * L
        for sg in (1, -1):
            out.append(Case("fp2sqr", "%s.equal%+d" % (tg, sg), [_pat(c, B, T, plus), _pat(c, B, T, [sg] * L)], "extreme",
                            tier, bd, 1))
        for nm, sig in (("alt", [1 if i % 2 == 0 else -1 for i in range(L)]), ("tla", [-1 if i % 2 == 0 else 1 for i in range(L)])):
            out.append(Case("fp2sqr", "%s.%s" % (tg, nm), [_pat(c, B, T, plus), _pat(c, B, T, sig)], "extreme", tier, bd, None))
        for k in range(L - 3, L + 1):
            for flip in (1, -1):
                sig = [flip if 2 * i < k else (-flip if 2 * i > k else 0) for i in range(L)]
                out.append(Case("fp2sqr", "%s.col%d%+d" % (tg, k, flip), [_pat(c, B, T, plus), _pat(c, B, T, sig)], "extreme",
                                tier, bd, None))
        # dot product: sum A_a A_b <= 4 split over the three pairs
        Z = (0, 0)
        T43 = (4 * S) // 3
        splits = {"4+0+0": [(1 << 30, S), Z, Z], "0+4+0": [Z, (1 << 29, 1 << 29), Z], "0+0+4": [Z, Z, (S, 1 << 30)],
                  "2+1+1": [(1 << 29, S), (S, S), (S, S)], "1+1+2": [(S, S), (S, S), (S, 1 << 29)],
                  "1+2+1": [(S, S), (1 << 29, S), (S, S)], "1+1+1": [(S, S), (S, S), (S, S)],
                  "4/3 each": [(T43, S), (S, T43), (T43, S)]}
        for nm, sp in splits.items():
            bd = []
            for Ba, Bb in sp:
                bd += [(Ba, T if Ba else 0), (Ba, T if Ba else 0), (Bb, T if Bb else 0), (Bb, T if Bb else 0)]
            for pn, sg, att in (("c0+", (1, -1, 1, 1), 0), ("c0-", (-1, 1, 1, 1), 0), ("c1+", (1, 1, 1, 1), 1), ("c1-", (-1, -1, 1, 1), 1)):
                ops = [_ext(c, b, t, sg[q % 4]) for q, (b, t) in enumerate(bd)]
                out.append(Case("fp2dot3", "%s.%s.%s" % (tg, nm, pn), ops, "extreme", tier, bd, att))
            # the pairs with different signs: the first pair against the other two (no column maximum, full-size limbs)
            ops = [_ext(c, b, t, (1, -1, 1, 1)[q % 4] * (1 if q < 4 else -1)) for q, (b, t) in enumerate(bd)]
            out.append(Case("fp2dot3", "%s.%s.mixed" % (tg, nm), ops, "extreme", tier, bd, None))
    return out


def value_edges(c, lazy=True):
    """(name, limbs): integers at the edges of the value range, in unique and (lazy) in borrowed / carried limbs"""
    rnd = random.Random(SEED + 1)
    p, L = c.p, c.L
    out = [("zero", [0] * L)]
    for k in (1, -1, 2, -3, 7, -8, 31, -32):
        out.append(("%dp" % k, c.limbs(k * p)))
        if lazy:
            out.append(("%dp~" % k, carry(c.limbs(k * p), rnd, 1)))
    for nm, V in (("1", 1), ("-1", -1), ("p-1", p - 1), ("1-p", 1 - p), ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2),
                  ("p+1", p + 1), ("one", c.R % p), ("-one", -(c.R % p)), ("2^(28 L/2)", 1 << (28 * (L // 2))),
                  ("2^(28L-7)", 1 << (28 * L - 7)), ("-2^(28L-7)", -(1 << (28 * L - 7)))):
        out.append((nm, c.limbs(V)))
    if lazy:
        out.append(("p-1~", carry(c.limbs(p - 1), rnd, 1)))
    out.append(("Nmax+", n_extreme(c, 1)))
    out.append(("Nmax-", n_extreme(c, -1)))
    out.append(("Nmin+", n_extreme(c, 1, NMIN)))
    out.append(("Nmin-", n_extreme(c, -1, NMIN)))
    return out


def lazy_random(c, rnd, amp=3, kbits=None):
    """a random field element as a lazily perturbed representative: x R mod p + k p, limbs carried by up to +-amp"""
    kmax = ((1 << (28 * c.L - 7)) // c.p) if kbits is None else (1 << kbits)
    V = rnd.randrange(c.p) + rnd.randint(-kmax, kmax) * c.p
    return carry(c.limbs(V), rnd, amp)


def _edge_cases(c):
    out = []
    ed = value_edges(c)
    one = c.limbs(1)
    # quotient digits of the reduction all 0 (the product is a multiple of 2^(28L)) and all 2^28 - 1 (the product is p)
    h = c.limbs(1 << (28 * (c.L // 2)))
    out.append(Case("mul", "m=0", [h, h], "edge"))
    out.append(Case("mul", "m=-1", [c.limbs(c.p), one], "edge"))
    out.append(Case("sqr", "m=0", [h], "edge"))
    for i, (na, a) in enumerate(ed):
        out.append(Case("sqr", na, [a], "edge"))
        for j, (nb, b) in enumerate(ed):
            out.append(Case("mul", na + " * " + nb, [a, b], "edge"))
        # Fp2: the edge value in each position, the others walking through the list
        e = lambda k: ed[(i + k) % len(ed)][1]
        out.append(Case("fp2sqr", na, [a, e(5)], "edge"))
        out.append(Case("fp2sqr", na + "'", [e(7), a], "edge"))
        out.append(Case("fp2mul", na, [a, e(3), e(11), e(17)], "edge"))
        out.append(Case("fp2mul", na + "'", [e(3), e(11), a, e(17)], "edge"))
    edn = value_edges(c, lazy=False)  # three pairs share the contract: unique / N limbs only
    for i in range(len(edn)):
        out.append(Case("fp2dot3", edn[i][0], [edn[(i + k) % len(edn)][1] for k in (0, 1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29)], "edge"))
    z = [0] * c.L
    out.append(Case("fp2mul", "0 * x", [z, z, ed[5][1], ed[9][1]], "edge"))
    out.append(Case("fp2mul", "(1 + u)(1 - u) with a = b", [one, one, one, [-x for x in one]], "edge"))
    out.append(Case("fp2sqr", "a0 = a1", [ed[9][1], ed[9][1]], "edge"))      # c0 = 0
    out.append(Case("fp2sqr", "a0 = -a1", [ed[9][1], [-x for x in ed[9][1]]], "edge"))
    return out


def _random_cases(c, per_body):
    rnd = random.Random(SEED + 2 + c.L)
    out = []
    S = 1 << 28
    for body in BODIES:
        for it in range(per_body):
            if it % 4 == 3:
                # random FULL-SIZE limbs inside the contract (signs free): no column maximum, but every limb large
                B = {"mul": math.isqrt(8 << 56), "sqr": math.isqrt(8 << 56), "fp2mul": 1 << 29, "fp2sqr": 1 << 29,
                     "fp2dot3": math.isqrt((4 << 56) // 3)}[body]
                # (dot product: three pairs of B x B with 3 B^2 <= 4 2^56)
                ops = [[rnd.randint(-B, B) for _ in range(c.L - 1)] + [rnd.randint(-TOP1, TOP1)] for _ in range(NOPS[body])]
                out.append(Case(body, "rand-full%d" % it, ops, "random", 1, [(B, TOP1)] * NOPS[body]))
            else:
                ops = [lazy_random(c, rnd, 0 if body == "fp2dot3" else 1) for _ in range(NOPS[body])]
                out.append(Case(body, "rand%d" % it, ops, "random", 2))
    return out


_CASES = {}


def multiplier_cases(cname, per_body=2000):
    """every case of the five multiplier bodies: extremes, value edges, `per_body` seeded random ones"""
    key = (cname, per_body)
    if key not in _CASES:
        c = ctx(cname)
        _CASES[key] = _extreme_cases(c) + _edge_cases(c) + _random_cases(c, per_body)
    return _CASES[key]


def over_contract_case(cname, body):
    """negative control: the first extreme case of the body with the lower limbs of ONE operand (the smallest) doubled
    until the big-integer model itself leaves int64 / int32 -- one doubling, except two for the Fp2 product and the dot
    product at L = 10, whose contract A_a A_b <= 4 is the L = 14 one and leaves room there.  Never sent to a device."""
    c = ctx(cname)
    case = next(x for x in _extreme_cases(c) if x.body == body and x.attains is not None)
    ops = [list(o) for o in case.ops]
    q = min((i for i, o in enumerate(ops) if any(o)), key=lambda i: max(abs(x) for x in ops[i]))
    for _ in range(3):
        ops[q] = [2 * x for x in ops[q][:-1]] + [ops[q][-1]]
        assert s32ok(ops[q])
        try:
            model(c, body, ops)
        except AssertionError:
            return Case(body, case.name + ".over", ops, "over")
    raise AssertionError("no over-contract case for " + body)


def assert_case_in_contract(c, case):
    """a case is inside the contract it is labelled with, and the label inside the body's contract (limb bounds only, no
    model: cheap enough for every case that is handed to the twin or to a device)"""
    body = case.body
    assert len(case.ops) == NOPS[body] and all(len(o) == c.L and s32ok(o) for o in case.ops), case.name
    assert all(abs(o[-1]) < (1 << 26) for o in case.ops), case.name
    if case.tier == 2:
        assert all(abs(c.val(o)) < (1 << (28 * c.L - 6)) for o in case.ops), case.name
    if case.bounds is not None:
        assert in_contract(c, body, case.bounds), case.name
        for o, (b, t) in zip(case.ops, case.bounds):
            assert all(abs(x) <= b for x in o[:-1]) and abs(o[-1]) <= t, case.name
    else:  # unlabelled (edges, lazy random values): inside the contract by their own limbs
        assert in_contract(c, body, [(max(abs(x) for x in o[:-1]), abs(o[-1])) for o in case.ops]), case.name


def selfcheck(cname, per_body=200):
    """the claims of the docstring, asserted; returns {body: largest |accumulator| / 2^63}"""
    c = ctx(cname)
    reached = {}
    for body in BODIES:
        stats = [Stat(), Stat()]
        want = [0, 0]
        for case in multiplier_cases(cname, per_body):
            if case.body != body:
                continue
            assert_case_in_contract(c, case)
            st = [Stat(), Stat()]
            got = model(c, body, case.ops, st)
            assert got == exact(c, body, case.ops), case.name
            for w in range(len(got)):
                stats[w].prod, stats[w].acc = max(stats[w].prod, st[w].prod), max(stats[w].acc, st[w].acc)
                if case.bounds is not None:
                    bound = column_bound(c, body, case.bounds, w)
                    assert st[w].prod <= bound, case.name
                    want[w] = max(want[w], bound)
                    if case.attains == w:
                        assert st[w].prod == bound, (case.name, st[w].prod / 2.0**56, bound / 2.0**56)
        for w in range(1 if body in ("mul", "sqr") else 2):
            assert stats[w].prod == want[w], (body, w)  # the set reaches what its labels allow, exactly
        reached[body] = max(s.acc for s in stats) / 2.0**63
        assert "%.4f" % reached[body] == REACHED[cname][body], (body, reached[body])
    # the over-contract controls are outside the contract, by their own bounds
    for body in BODIES:
        oc = over_contract_case(cname, body)
        assert not in_contract(c, body, [(max(abs(x) for x in o[:-1]), abs(o[-1])) for o in oc.ops]), body
    return reached


# =====================================================================================================================
# The operation table (tests/hip/arith_ops.inc holds the same ids and shapes): operands per operation and the
# big-integer check of what came back.  `op_cases(cname, op)` -> [Item]; `op_check(cname, op, item, outs)` asserts.
# =====================================================================================================================
OPS = {  # name: (id, operands, results) in base-field elements of L int32 limbs
    "fq_mul": (0, 2, 1), "fq_sqr": (1, 1, 1), "fq_norm": (2, 1, 1), "fq_norm_full": (3, 1, 1), "fq_vreduce": (4, 1, 1),
    "fq_is_zero": (5, 1, 1), "fq_is_zero_slow": (6, 1, 1), "fq_eq": (7, 2, 1), "fq_inv": (8, 1, 1),
    "fq_from_boundary": (9, 1, 1), "fq_to_boundary": (10, 1, 1), "f2_mul": (11, 4, 2), "f2_mul_l2": (12, 4, 2),
    "f2_sqr": (13, 2, 2), "f2_sqr_l2": (14, 2, 2), "f2_dot3": (15, 12, 2), "f2_mul_xi": (16, 2, 2), "f2_mul_fp": (17, 3, 2),
    "f2_inv": (18, 2, 2), "f6_mul": (19, 12, 6), "f6_mul_by_01": (20, 10, 6), "f12_mul": (21, 24, 12),
    "f12_sqr": (22, 12, 12), "f12_mul_by_014": (23, 18, 12), "f12_mul_by_034": (24, 18, 12), "f12_cyclo_chain": (25, 12, 12),
    "f12_inv": (26, 12, 12), "f12_frob": (27, 12, 36), "f12_eq": (28, 24, 1), "g1_dbl": (29, 3, 3), "g1_madd": (30, 5, 3),
    "g1_add": (31, 6, 3), "g2_dbl": (32, 6, 6), "g2_madd": (33, 10, 6), "g2_add": (34, 12, 6),
    "f12_cyclo_sqr": (35, 12, 12),
}
BASE_FP2_OPS = [k for k in OPS if k.startswith(("fq_", "f2_"))]  # the families the inline-multiplier build runs too
CYCLO_STEPS = 9
_BODY_OF = {"fq_mul": "mul", "fq_sqr": "sqr", "f2_mul": "fp2mul", "f2_mul_l2": "fp2mul", "f2_sqr": "fp2sqr",
            "f2_sqr_l2": "fp2sqr", "f2_dot3": "fp2dot3"}


class Item:
    def __init__(self, ops, tag="", want=None):
        self.ops, self.tag, self.want = ops, tag, want


def _oracle(c):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gs_oracle as O

    O.set_curve(O._bls12_381() if c.name == "bls12_381" else O._bn254())
    return O


def zero_values(c):
    """(V, is a multiple of p): k p, k p +- 1 and k p +- 2^56 (which the two-limb filter cannot tell from k p) for |k|
    swept in powers of two with neighbours up to the limit of is_zero: |top limb| < 2^26 after one carry round"""
    kmax = ((1 << (28 * c.L - 2)) - (1 << (28 * (c.L - 1) + 5))) // c.p
    ks = {0, 1, 2, 3, kmax, kmax - 1}
    j = 2
    while (1 << j) - 1 <= kmax:
        ks |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
        j += 1
    out = []
    for k in sorted(x for x in ks if 0 <= x <= kmax):
        for sg in (1, -1):
            for d in (0, 1, -1, 1 << 56, -(1 << 56)):
                out.append((sg * k * c.p + d, d == 0))
    return out, kmax


def _zero_items(c, small_limbs=False):
    rnd = random.Random(SEED + 3)
    items = []
    vals, _ = zero_values(c)
    for V, z in vals:
        reps = [c.limbs(V), n_form(c, V, hi=True), n_form(c, V, hi=False)]
        if not small_limbs:
            reps += [carry(c.limbs(V), rnd, 6), carry(c.limbs(V), rnd, 1)]
        for r in reps:
            assert s32ok(r) and abs(norm(r)[-1]) < (1 << 26) and c.val(r) == V
            items.append(Item([r], "V=%dp%+d" % (round(V / c.p), V - round(V / c.p) * c.p) if abs(V) > c.p // 2 else "V=%d" % V, z))
    for _ in range(500):  # random non-multiples and random representatives of 0
        V = c.val(lazy_random(c, rnd))
        z = rnd.random() < 0.3
        if z:
            V = rnd.randint(-40, 40) * c.p
        r = carry(c.limbs(V), rnd, 0 if small_limbs else 3)
        items.append(Item([r], "random", V % c.p == 0))
    return items


def _vreduce_items(c):
    rnd = random.Random(SEED + 4)
    p, L = c.p, c.L
    lim = min(p << 20, ((1 << 31) - 16) << (28 * (L - 1)))  # |V| < 2^20 p, and the top limb is an int32
    qmax = lim // p - 1
    Vs = []
    qs = {0, 1, 2, qmax, qmax - 1}
    j = 2
    while (1 << j) + 1 <= qmax:
        qs |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
        j += 1
    for q in sorted(qs):
        for sg in (1, -1):
            for r in (0, 1, -1, (p - 1) // 2, -((p - 1) // 2), (p + 1) // 2, rnd.randrange(p)):
                Vs.append(sg * q * p + r)
    # V / p within one f32 ulp (2^-23 relative, and a quarter / four times that) of a half-integer, on both sides
    for m in (0, 1, 2, 5, 100, 1 << 10, (1 << 14) - 3, (1 << 17) + 1, (1 << 19) + 3, (1 << 20) - 2):
        for sg in (1, -1):
            h = ((2 * m + 1) * p) // 2
            for e in (0, 1, p * (m + 1) >> 25, p * (m + 1) >> 23, p * (m + 1) >> 21):
                Vs += [sg * (h + e), sg * (h - e)]
    for _ in range(2000):
        Vs.append(rnd.randint(-1, 1) * rnd.randrange(1 << rnd.randint(1, lim.bit_length() - 1)) + rnd.randrange(p))
    items = []
    for V in Vs:
        if abs(V) >= lim:
            continue
        for r in (c.limbs(V), n_form(c, V, hi=True), n_form(c, V, hi=False)):
            assert s32ok(r)
            items.append(Item([r], "V/p=%.6f" % (V / p)))
    return items


def inversion_values(c):
    """the value list of tests/test_twin.py::test_inversion_safegcd"""
    import numpy as np

    rng = np.random.default_rng(2024)
    vals = [int.from_bytes(rng.bytes(64), "little") % c.p for _ in range(400)]
    vals += [1, 2, 3, c.p - 1, c.p - 2, (c.p - 1) // 2, (c.p + 1) // 2]
    for k in range(1, c.p.bit_length(), 7):
        vals += [(1 << k) % c.p, ((1 << k) - 1) % c.p, (c.p - (1 << k)) % c.p]
    return vals


def _inv_items(c):
    rnd = random.Random(SEED + 5)
    kmax = ((1 << (28 * c.L - 2)) - (1 << (28 * (c.L - 1) + 5))) // c.p - 1
    items = []
    for n, x in enumerate(inversion_values(c) + [0]):
        V = x * c.R % c.p
        reps = [c.limbs(V), c.limbs(V - c.p), carry(c.limbs(V + rnd.randint(-kmax, kmax) * c.p), rnd, 3)]
        if n % 8 == 0 or n >= 400:
            reps += [c.limbs(V + kmax * c.p), c.limbs(V - kmax * c.p), n_form(c, V + c.p, hi=True), carry(c.limbs(V), rnd, 6)]
        for r in reps:
            assert s32ok(r) and abs(norm(r)[-1]) < (1 << 26)
            items.append(Item([r], hex(x), x))
    return items


def to_boundary_branch(c, v):
    """which branch of fq_to_boundary the internal limbs v take: the product t = norm(v) K_OUT / R is < 0 (`plus`: p is
    added), >= p (`minus`) or already canonical (`t`)"""
    t = c.mont(c.val(v) * c.val(c.K_OUT28))
    assert -c.p // 2 < t < 3 * c.p // 2
    return "plus" if t < 0 else ("minus" if t >= c.p else "t")


def _to_boundary_items(c):
    rnd = random.Random(SEED + 6)
    items = [Item([c.enc(x)], "canonical", x) for x in (0, 1, c.p - 1, 2, (c.p - 1) // 2)]
    items += [Item([v], nm) for nm, v in value_edges(c)]
    count = {"plus": 0, "minus": 0, "t": 0}
    kmax = (1 << (28 * c.L - 6)) // c.p
    tries = 0
    while min(count.values()) < 40 and tries < 200000:
        tries += 1
        V = rnd.randrange(c.p) + rnd.choice((-1, 1)) * rnd.randint(kmax * 3 // 4, kmax - 1) * c.p
        v = carry(c.limbs(V), rnd, 1)
        b = to_boundary_branch(c, v)
        if count[b] < 40 or b != "t" and count[b] < 120:
            count[b] += 1
            items.append(Item([v], b))
    assert min(count.values()) >= 40, count  # all three branches are taken, by the reference's own computation
    return items


def _n_pool(c, rnd, n_random):
    """base-field elements in N form: the four all-limbs-extreme vectors, the value edges, random values in edge limbs"""
    pool = [n_extreme(c, 1), n_extreme(c, -1), n_extreme(c, 1, NMIN), n_extreme(c, -1, NMIN)]
    pool += [v for _, v in value_edges(c, lazy=False)]
    for i in range(n_random):
        V = rnd.randrange(c.p) + rnd.randint(-2, 2) * c.p
        pool.append(n_form(c, V, hi=i % 2 == 0))
    return pool


def _tower_items(c, ncoef, count=160):
    """items of `ncoef` N-form coefficients: every coefficient at one extreme; the extremes alternating; operand against
    operand; the edge pool walking through the positions; random"""
    rnd = random.Random(SEED + 7 + ncoef)
    pool = _n_pool(c, rnd, 64)
    ext = pool[:4]
    items = [Item([e] * ncoef, "all ext%d" % i) for i, e in enumerate(ext)]
    items += [Item([ext[(q + s) % 2] for q in range(ncoef)], "alternating") for s in (0, 1)]
    items += [Item([ext[(q // 2 + s) % 2] for q in range(ncoef)], "alternating Fp2") for s in (0, 1)]
    items += [Item([ext[2 + (q + s) % 2] for q in range(ncoef)], "alternating min") for s in (0, 1)]
    # lower limbs at the top of the N range in one coefficient and at the bottom in its neighbour: N limbs have (almost)
    # no sign, so differences such as a0 + b0 - b1 are largest when the subtracted coefficient is the small one
    items += [Item([ext[0] if (q + s) % 2 == 0 else ext[2] for q in range(ncoef)], "max / min alternating") for s in (0, 1)]
    items += [Item([ext[1] if (q // 2 + s) % 2 == 0 else ext[3] for q in range(ncoef)], "max / min alternating Fp2") for s in (0, 1)]
    items += [Item([rnd.choice(ext) for q in range(ncoef)], "extremes at random") for _ in range(16)]
    items += [Item([ext[0 if q < ncoef // 2 else 1] for q in range(ncoef)], "a+ b-"),
              Item([ext[1 if q < ncoef // 2 else 0] for q in range(ncoef)], "a- b+")]
    for s in range(len(pool)):
        items.append(Item([pool[(s + 5 * q) % len(pool)] for q in range(ncoef)], "edges %d" % s))
    while len(items) < count:
        items.append(Item([rnd.choice(pool) for _ in range(ncoef)], "random"))
    return items


def _cyclo_items(c):
    rnd = random.Random(SEED + 8)
    g = c.golden
    vals = [e["out"] for e in g["pairing"]] + list(g["pairing_sum"]["out"])
    items = []
    for h in vals:
        xs = [int(s, 16) for s in h]
        for rep in range(6):
            ops = []
            for x in xs:
                V = x * c.R % c.p + (0 if rep == 0 else rnd.randint(-2, 2) * c.p)
                ops.append(c.limbs(V) if rep < 2 else n_form(c, V, hi=rep % 2 == 0))
            items.append(Item(ops, "gt"))
    one = [c.enc(1)] + [[0] * c.L] * 11
    items.append(Item(one, "one"))
    return items


def _coord_extreme(c, rnd, lo):
    """a coordinate with EVERY lower limb at the edge of the N range and a value inside (-p/2, 3p/2)"""
    while True:
        v = [lo] * (c.L - 1) + [rnd.randint(-c.P28[-1], 2 * c.P28[-1])]
        if -c.p // 2 < c.val(v) < 3 * c.p // 2:
            return v


def _coord(c, rnd, x, mode):
    V = x * c.R % c.p
    if mode % 3 == 1:
        V += c.p if V < c.p // 2 else -c.p
    return n_form(c, V, hi=mode % 2 == 0)


def _curve_items(c, op):
    """Jacobian operands as N-form coordinates.  The generic cases come first, in whole waves of 64 (the generated point
    additions leave the wave for the C++ edge path when ANY lane has an edge), then the edge cases."""
    rnd = random.Random(SEED + 9 + OPS[op][0])
    g2 = op.startswith("g2")
    kind = op[3:]
    w = 2 if g2 else 1  # base-field elements per coordinate
    p = c.p
    fadd = (lambda a, b: tuple((x + y) % p for x, y in zip(a, b)))
    if g2:
        fmul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)
        finv = lambda a: (lambda n: (a[0] * n % p, -a[1] * n % p))(pow(a[0] * a[0] + a[1] * a[1], -1, p))
        fneg = lambda a: ((-a[0]) % p, (-a[1]) % p)
        rand = lambda: (rnd.randrange(p), rnd.randrange(p))
        ONE = (1, 0)
    else:
        fmul = lambda a, b: (a[0] * b[0] % p,)
        finv = lambda a: (pow(a[0], -1, p),)
        fneg = lambda a: ((-a[0]) % p,)
        rand = lambda: (rnd.randrange(p),)
        ONE = (1,)
    enc = lambda f, mode: [_coord(c, rnd, x, mode) for x in f]
    zero = [[0] * c.L] * w
    ncoord = {"dbl": 3, "madd": 5, "add": 6}[kind]
    items = []
    for i in range(128):  # generic: two whole waves
        if i < 32:
            ops = [_coord_extreme(c, rnd, NMAX if (i + q) % 3 else NMIN) for q in range(ncoord * w)]
        else:
            ops = [v for _ in range(ncoord) for v in enc(rand(), i)]
        items.append(Item(ops, "generic"))
    if kind == "dbl":
        for i in range(8):
            X, Y = rand(), rand()
            items.append(Item(enc(X, i) + enc(Y, i) + zero, "identity"))
            items.append(Item(enc(X, i) + enc(Y, i) + enc(ONE, 1 + 3 * i), "Z = lazy 1"))
        return items
    for i in range(12):
        X, Y, Z = rand(), rand(), rand()
        if i % 4 == 3:
            Z = ONE
        zi = finv(Z)
        zi2 = fmul(zi, zi)
        x, y = fmul(X, zi2), fmul(Y, fmul(zi2, zi))  # the affine point of (X, Y, Z)
        P = enc(X, i) + enc(Y, i + 1) + enc(Z, 1 if Z == ONE else i + 2)
        if kind == "madd":
            items.append(Item(P + enc(x, i) + enc(y, i), "P + P"))
            items.append(Item(P + enc(x, i + 1) + enc(fneg(y), i), "P + (-P)"))
            items.append(Item(P + zero + zero, "P + O"))
            items.append(Item(enc(X, i) + enc(Y, i) + zero + enc(x, i) + enc(y, i), "O + P"))
            items.append(Item(P + enc(rand(), i) + enc(rand(), i), "generic among edges"))
        else:
            Z2 = rand()
            z22 = fmul(Z2, Z2)
            Q = lambda yy: enc(fmul(x, z22), i) + enc(fmul(yy, fmul(z22, Z2)), i) + enc(Z2, i + 1)
            items.append(Item(P + Q(y), "P + P"))
            items.append(Item(P + Q(fneg(y)), "P + (-P)"))
            items.append(Item(P + enc(rand(), i) + enc(rand(), i) + zero, "P + O"))
            items.append(Item(enc(X, i) + enc(Y, i) + zero + Q(y), "O + P"))
            items.append(Item(P + enc(rand(), i) + enc(rand(), i) + enc(ONE, 1), "Z2 = lazy 1"))
    return items


_OPCASES = {}


def op_cases(cname, op):
    key = (cname, op)
    if key in _OPCASES:
        return _OPCASES[key]
    c = ctx(cname)
    rnd = random.Random(SEED + 100 + OPS[op][0])
    S31 = (1 << 31) - 16
    if op in _BODY_OF:
        mine = [x for x in multiplier_cases(cname) if x.body == _BODY_OF[op]]
        for x in mine:  # the set that is actually sent (selfcheck models a shorter random set): every case in contract
            assert_case_in_contract(c, x)
        items = [Item(x.ops, x.kind + " " + x.name) for x in mine]
    elif op in ("fq_norm", "fq_norm_full"):
        top = (1 << 30)
        vs = [[s * S31] * (c.L - 1) + [t * top] for s in (1, -1) for t in (1, -1)]
        vs += [[S31 if i % 2 else -S31 for i in range(c.L - 1)] + [top], [-S31 if i % 2 else S31 for i in range(c.L - 1)] + [-top]]
        vs += [v for _, v in value_edges(c)]
        vs += [[rnd.randint(-S31, S31) for _ in range(c.L - 1)] + [rnd.randint(-top, top)] for _ in range(1500)]
        vs += [lazy_random(c, rnd, 6) for _ in range(500)]
        items = [Item([v]) for v in vs]
    elif op == "fq_vreduce":
        items = _vreduce_items(c)
    elif op in ("fq_is_zero", "fq_is_zero_slow"):
        items = _zero_items(c)
    elif op == "fq_eq":
        items = []
        for z in _zero_items(c, small_limbs=True):
            a = n_form(c, rnd.randrange(c.p), hi=rnd.random() < 0.5)
            items.append(Item([a, [x - y for x, y in zip(a, z.ops[0])]], z.tag, z.want))
            assert s32ok(items[-1].ops[1])
    elif op == "fq_inv":
        items = _inv_items(c)
    elif op == "fq_from_boundary":
        xs = [0, 1, 2, c.p - 1, c.p - 2, (c.p - 1) // 2, pow(c.Rb, -1, c.p), (c.p - 1) * pow(c.Rb, -1, c.p) % c.p]
        xs += [rnd.randrange(c.p) for _ in range(1000)]
        s32 = lambda w: w - (1 << 32) if w >> 31 else w  # the u32 words travel as int32 bit patterns
        items = [Item([[s32(w) for w in c.words(x)] + [0] * (c.L - c.N)], hex(x), x) for x in xs]
    elif op == "fq_to_boundary":
        items = _to_boundary_items(c)
    elif op == "f2_mul_xi":
        pool = _n_pool(c, rnd, 200)
        items = [Item([pool[i], pool[(i * 7 + s) % len(pool)]]) for i in range(len(pool)) for s in (0, 1, 3)]
    elif op == "f2_mul_fp":
        pool = _n_pool(c, rnd, 100) + [lazy_random(c, rnd, 1) for _ in range(200)]
        items = [Item([pool[i], pool[(i * 7 + 1) % len(pool)], pool[(i * 11 + 2) % len(pool)]]) for i in range(len(pool))]
    elif op == "f2_inv":
        pool = _n_pool(c, rnd, 100) + [lazy_random(c, rnd, 1) for _ in range(100)]
        items = [Item([pool[i], pool[(i * 7 + 1) % len(pool)]]) for i in range(len(pool))]
        items += [Item([[0] * c.L, [0] * c.L], "zero"), Item([c.limbs(c.p), c.limbs(-c.p)], "zero as (p, -p)")]
    elif op == "f12_cyclo_chain":
        items = _cyclo_items(c)
    elif op == "f12_eq":
        items = []
        for it in _tower_items(c, 12, 60):
            same = [n_form(c, c.val(v) % c.p + rnd.randint(-1, 1) * c.p, hi=rnd.random() < 0.5) for v in it.ops]
            items.append(Item(it.ops + same, "same element", True))
            q = rnd.randrange(12)
            other = [list(v) for v in same]
            other[q][0] += 1
            items.append(Item(it.ops + other, "one coefficient + 1", False))
    elif op.startswith(("f6_", "f12_")):
        items = _tower_items(c, OPS[op][1])
    else:
        items = _curve_items(c, op)
    for it in items:
        assert len(it.ops) == OPS[op][1] and all(len(o) == c.L and s32ok(o) for o in it.ops), (op, it.tag)
    _OPCASES[key] = items
    return items


def _f2(c, v):
    return (c.fe(v[0]), c.fe(v[1]))


def _f6(c, v):
    return tuple(_f2(c, v[2 * i:2 * i + 2]) for i in range(3))


def _f12(c, v):
    return (_f6(c, v[:6]), _f6(c, v[6:12]))


def _n_range(c, outs, what, lo=-NMAX):
    """the representation an N output has: lower limbs within one carry round's range (negated values included), the
    top limb inside the multiplier contract"""
    for r in outs:
        assert all(lo <= x <= NMAX for x in r[:-1]) and abs(r[-1]) < (1 << 26), what


def cyclo_sqr_formula(c, O, f):
    """Granger-Scott squaring as the polynomial map it is (equal to f^2 on the cyclotomic subgroup only): three Fp4
    squarings (a + b t)^2, t^2 = xi, and z <- 3 t -+ 2 z"""
    def fp4_sqr(a, b):
        return O.f2_add(O.f2_sqr(a), O.f2_mul(c.xi, O.f2_sqr(b))), O.f2_scale(O.f2_mul(a, b), 2)

    lin = lambda t, z, s: O.f2_add(O.f2_scale(t, 3), O.f2_scale(z, 2 * s))
    (a0, a1, a2), (b0, b1, b2) = f
    t0, t1 = fp4_sqr(a0, b1)
    t2, t3 = fp4_sqr(b0, a2)
    t4, t5 = fp4_sqr(a1, b2)
    return ((lin(t0, a0, -1), lin(t2, a1, -1), lin(t4, a2, -1)), (lin(O.f2_mul(c.xi, t5), b0, 1), lin(t1, b1, 1), lin(t3, b2, 1)))


def op_check(cname, op, item, outs):
    """assert that `outs` (result limb vectors) is what `op` must return on item.ops"""
    c = ctx(cname)
    p, L = c.p, c.L
    ops, what = item.ops, (cname, op, item.tag)
    if op in _BODY_OF:
        assert outs == exact(c, _BODY_OF[op], ops), what  # congruent, limbs unique, value in [W/R, W/R + p)
        for r in outs:
            assert all(0 <= x < (1 << 28) for x in r[:-1]), what
        return
    if op == "fq_norm":
        assert outs[0] == norm(ops[0]) and c.val(outs[0]) == c.val(ops[0]), what
        assert all(NMIN <= x <= NMAX for x in outs[0][:-1]), what
    elif op == "fq_norm_full":
        assert outs[0] == c.limbs(c.val(ops[0])), what
    elif op == "fq_vreduce":
        V, W = c.val(ops[0]), c.val(outs[0])
        assert (V - W) % p == 0 and outs[0] == c.limbs(W), what
        assert abs(W) * (1 << 21) < (1 << 20) * p + abs(V) + (1 << (28 * (L - 2) + 22)), what  # the header's bound, times 2^21
        assert abs(W) < p + (1 << (28 * (L - 2) + 1)), what  # ... which over the input range is this
    elif op in ("fq_is_zero", "fq_is_zero_slow", "fq_eq"):
        assert outs[0] == [1 if item.want else 0] + [0] * (L - 1), what
    elif op == "fq_inv":
        x = c.fe(ops[0])
        assert x == item.want and c.fe(outs[0]) == (pow(x, -1, p) if x else 0), what
        assert all(0 <= v < (1 << 28) for v in outs[0][:-1]) and -p // 2 < c.val(outs[0]) < 3 * p // 2, what
    elif op == "fq_from_boundary":
        w = sum((x & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(ops[0][:c.N]))
        assert c.fe(outs[0]) == item.want and outs[0] == c.limbs(c.mont(w * c.val(_param_array(cname, "K_IN28")))), what
    elif op == "fq_to_boundary":
        assert [x & 0xFFFFFFFF for x in outs[0][:c.N]] == c.words(c.fe(ops[0])) and not any(outs[0][c.N:]), what
    elif op == "f2_mul_xi":
        a = _f2(c, ops)
        assert _f2(c, outs) == ((c.xi[0] * a[0] - a[1]) % p, (c.xi[0] * a[1] + a[0]) % p), what
        if c.xi[0] == 1:
            assert outs == [[x - y for x, y in zip(*ops)], [x + y for x, y in zip(*ops)]], what
    elif op == "f2_mul_fp":
        assert outs == [exact(c, "mul", [ops[0], ops[2]])[0], exact(c, "mul", [ops[1], ops[2]])[0]], what
    elif op == "f2_inv":
        a = _f2(c, ops)
        n = (a[0] * a[0] + a[1] * a[1]) % p
        ni = pow(n, -1, p) if n else 0
        assert _f2(c, outs) == (a[0] * ni % p, -a[1] * ni % p), what
        _n_range(c, outs, what)
    elif op.startswith(("f6_", "f12_")):
        O = _oracle(c)
        if op == "f6_mul":
            want = O.f6_mul(_f6(c, ops[:6]), _f6(c, ops[6:]))
            got = _f6(c, outs)
        elif op == "f6_mul_by_01":
            want = O.f6_mul(_f6(c, ops[:6]), (_f2(c, ops[6:8]), _f2(c, ops[8:10]), (0, 0)))
            got = _f6(c, outs)
        elif op == "f12_eq":
            assert outs[0] == [1 if item.want else 0] + [0] * (L - 1), what
            assert (_f12(c, ops[:12]) == _f12(c, ops[12:])) == item.want, what
            return
        elif op == "f12_frob":
            a = _f12(c, ops)
            for j in (1, 2, 3):
                assert _f12(c, outs[12 * (j - 1):12 * j]) == O.frob_fp12(a, j), what + (j,)
            _n_range(c, outs, what)
            return
        else:
            a = _f12(c, ops[:12])
            got = _f12(c, outs)
            z = (0, 0)
            if op == "f12_mul":
                want = O.f12_mul(a, _f12(c, ops[12:]))
            elif op == "f12_sqr":
                want = O.f12_mul(a, a)
            elif op == "f12_mul_by_014":
                l0, l1, l4 = (_f2(c, ops[12 + 2 * i:14 + 2 * i]) for i in range(3))
                want = O.f12_mul(a, ((l0, l1, z), (z, l4, z)))
            elif op == "f12_mul_by_034":
                l0, l3, l4 = (_f2(c, ops[12 + 2 * i:14 + 2 * i]) for i in range(3))
                want = O.f12_mul(a, ((l0, z, z), (l3, l4, z)))
            elif op == "f12_cyclo_sqr":
                want = cyclo_sqr_formula(c, O, a)
            elif op == "f12_cyclo_chain":
                want = a
                for _ in range(CYCLO_STEPS):
                    want = O.f12_mul(want, want)
            else:
                assert op == "f12_inv"
                want = O.f12_inv(a) if a != O.F12_0 else None
                if want is None:
                    return
        assert got == want, what
        _n_range(c, outs, what)
    else:
        O = _oracle(c)
        g2 = op.startswith("g2")
        w = 2 if g2 else 1
        F = O.FP2 if g2 else O.FP
        el = (lambda v: _f2(c, v)) if g2 else (lambda v: c.fe(v[0]))
        zero = (0, 0) if g2 else 0

        def aff(X, Y, Z):
            if all(x == 0 for v in Z for x in v):  # the identity is EXACT zero limbs
                return None
            z = el(Z)
            assert z != zero, what
            zi = F.inv(z)
            zi2 = F.mul(zi, zi)
            return (F.mul(el(X), zi2), F.mul(el(Y), F.mul(zi2, zi)))

        co = [ops[i * w:(i + 1) * w] for i in range(len(ops) // w)]
        P = aff(co[0], co[1], co[2])
        if op.endswith("dbl"):
            want = O.ec_add(F, P, P)
        elif op.endswith("madd"):
            qinf = all(x == 0 for v in co[3] + co[4] for x in v)
            want = O.ec_add(F, P, None if qinf else (el(co[3]), el(co[4])))
        else:
            want = O.ec_add(F, P, aff(co[3], co[4], co[5]))
        ro = [outs[i * w:(i + 1) * w] for i in range(3)]
        zval = el(ro[2])
        if want is None:
            assert zval == zero, what
        else:
            assert zval != zero and aff(*ro) == want, what
        _n_range(c, outs, what, lo=NMIN if "generic" in item.tag else -NMAX)


def pack(cname, op, items):
    import numpy as np

    return np.array([x for it in items for o in it.ops for x in o], dtype=np.int64).astype(np.int32)


def unpack(cname, op, n, out):
    L, nout = LIMBS[cname], OPS[op][2]
    a = out.reshape(n, nout, L).tolist()
    return a


def check_all(cname, op, items, out):
    res = unpack(cname, op, len(items), out)
    for it, o in zip(items, res):
        op_check(cname, op, it, o)


def run_table(lib_path, entry, cname, ops, curve_arg=None):
    """every operation of `ops` over its cases through the C entry `entry` of the shared object: {op: int32 results}.
    curve_arg None: entry(op, n, in, out) (the CPU twin); else entry(curve, op, n, in, out) (the device probe)."""
    import ctypes

    import numpy as np

    lib = ctypes.CDLL(lib_path)
    fn = getattr(lib, entry)
    fn.restype = ctypes.c_int
    res = {}
    for op in ops:
        if curve_arg is not None:  # the table here and the one compiled into the probe agree
            a, b = ctypes.c_int(), ctypes.c_int()
            if lib.probe_shape(OPS[op][0], ctypes.byref(a), ctypes.byref(b)) != 0 or (a.value, b.value) != OPS[op][1:]:
                raise RuntimeError("operation table mismatch: " + op)
        items = op_cases(cname, op)
        sys.stderr.write("raw op %s %s: %d items\n" % (cname, op, len(items)))
        sys.stderr.flush()
        a = pack(cname, op, items)
        out = np.zeros(len(items) * OPS[op][2] * LIMBS[cname], dtype=np.int32)
        args = (OPS[op][0], len(items), a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        rc = fn(*args) if curve_arg is None else fn(curve_arg, *args)
        if rc != 0:
            raise RuntimeError("%s(%s, %s) returned %d" % (entry, cname, op, rc))
        res[op] = out
    return res


if __name__ == "__main__":
    # child process of tests/test_twin.py and tests/test_gpu_arith.py: arithvec.py LIB ENTRY CURVE OUT.npz OP[,OP...] [CURVE_ID]
    # (the first failure ends the process: nothing further is run)
    import numpy as np

    _lib, _entry, _cname, _out, _ops = sys.argv[1:6]
    _cid = int(sys.argv[6]) if len(sys.argv) > 6 else None
    np.savez(_out, **run_table(_lib, _entry, _cname, _ops.split(","), _cid))

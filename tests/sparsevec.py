"""Sparse and degenerate Groth-Sahai statements: one named batch per (curve, type) in which every equation is a TRUE
statement (three named families of false twins apart) and carries one degenerate pattern -- identity variables and
constants, sparse Gamma, commitments without randomness, a dead commitment component, dead commitments, sums that cancel
to the identity from non-identity terms, everything the identity.  Random batches (groth_sahai_rs_amd/workload.py) draw
every element uniformly and never contain one of these, so the kernels behind the large-batch plans never see an
identity; tests/test_gpu_sparse.py puts this batch through every forced kernel shape.

How the batch is built.  The CRS is the binding key of forge.crs_pair over p1 = AL g1, p2 = BE g2 with known trapdoors
a1, a2, t1, t2:  u = [(p1, a1 p1), (t1 p1, t1 a1 p1)],  v likewise.  Every variable, constant, Gamma entry and every
random scalar is kept as an integer mod r (its discrete logarithm to p1 / p2 where it is a group element); the points are
built with the C oracle (gs_ref_py.g_mul), never with the engine.  The target of an equation comes from the logarithms,
  t = sum_j a_j y_j + sum_i x_i b_i + sum_ij x_i gamma_ij y_j,
as gt^t (PPE, gs_ref_py.gt_pow), t p1 / t p2 (MSMEG1 / MSMEG2) or t itself (QuadEqu).

Because every logarithm is known, the logarithm of every commitment component and of every proof element is known too
(model()): iota1(X) = (0, x) for a group element and x (u1 + (O, p1)) = (x t1, x (t1 a1 + 1)) for a scalar,
  c_i = iota1(x_i) + sum_k R_ik u_k,   d_j = iota2(y_j) + sum_k S_jk v_k,
  pi_k = sum_i R_ik iota2(b_i) + sum_j (R^T Gamma)_kj iota2(y_j) + sum_l (R^T Gamma S - T^T)_kl v_l,
  theta_k = sum_j S_jk iota1(a_j) + sum_i (S^T Gamma^T)_ki iota1(x_i) + sum_l T_kl u_l.
selfcheck() compares every one of them with what oracle/gs_ref.c computes, so "the identity appears exactly where the
pattern claims it and nowhere else" is checked on every element of every equation, not on a named few; the named claims
of a pattern (CLAIMS) are checked on top, and a claim a type cannot hold (a scalar commitment without randomness has no
dead component) is RETURNED by name, never dropped silently.

Equation e carries pattern e % P; with P = 36 patterns N is 72 (the next N with N % 64 not in {0, 1} that holds every
pattern twice): two waves per Miller task in the twin form, three in the pair forms, the last one ragged, every wave a
mix of patterns and every pattern at two lane positions."""
import os
import random
import sys

import numpy as np

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))
import forge  # noqa: E402
import gs_ref_py as ref  # noqa: E402
from forge import u8, xg, yg  # noqa: E402

M = N_ = 4
# scalars of the CRS (fixed; any non-zero values do)
AL, BE = 0x5EED0001, 0x5EED0002
TRAP = dict(a1=0x1111111111111111222222222222222233333333, a2=0x4444444444444444555555555555555566666666,
            t1=0x7777777777777777888888888888888899999999, t2=0xAAAAAAAAAAAAAAAABBBBBBBBBBBBBBBBCCCCCCCC)


# ---- logarithm arithmetic ---------------------------------------------------------------------------------------
def _key(a, t, r):
    return [(1, a % r), (t % r, t * a % r)]


def _iota(isg, v, a, t, r):
    return (0, v % r) if isg else (v * t % r, v * (t * a + 1) % r)


def _lin(terms, r):
    """sum of s * (l0, l1) over (s, (l0, l1)) terms"""
    return (sum(s * v[0] for s, v in terms) % r, sum(s * v[1] for s, v in terms) % r)


def _matmul(a, b, r):
    return [[sum(a[i][k] * b[k][j] for k in range(len(b))) % r for j in range(len(b[0]))] for i in range(len(a))]


def _tr(a):
    return [list(x) for x in zip(*a)]


def model(L, ty, r):
    """logarithms (pairs, to p1 / p2) of every commitment and proof element of the equation with logarithms L"""
    a1, a2, t1, t2 = (TRAP[k] for k in ("a1", "a2", "t1", "t2"))
    U, V = _key(a1, t1, r), _key(a2, t2, r)
    kx, ky = (2 if xg(ty) else 1), (2 if yg(ty) else 1)
    m, n = len(L["x"]), len(L["y"])
    ix = [_iota(xg(ty), v, a1, t1, r) for v in L["x"]]
    ia = [_iota(xg(ty), v, a1, t1, r) for v in L["a"]]
    iy = [_iota(yg(ty), v, a2, t2, r) for v in L["y"]]
    ib = [_iota(yg(ty), v, a2, t2, r) for v in L["b"]]
    R, S, T, G = L["R"], L["S"], L["T"], L["G"]
    xc = [_lin([(1, ix[i])] + [(R[i][k], U[k]) for k in range(kx)], r) for i in range(m)]
    yc = [_lin([(1, iy[j])] + [(S[j][k], V[k]) for k in range(ky)], r) for j in range(n)]
    Rt, St = _tr(R), _tr(S)
    psi = _matmul(Rt, G, r)  # kx x n
    om = [[(p - q) % r for p, q in zip(ra, rb)] for ra, rb in zip(_matmul(psi, S, r), _tr(T))]  # kx x ky
    pi = [_lin([(Rt[k][i], ib[i]) for i in range(m)] + [(psi[k][j], iy[j]) for j in range(n)] +
               [(om[k][l], V[l]) for l in range(ky)], r) for k in range(kx)]
    phi = _matmul(St, _tr(G), r)  # ky x m
    th = [_lin([(St[k][j], ia[j]) for j in range(n)] + [(phi[k][i], ix[i]) for i in range(m)] +
               [(T[k][l], U[l]) for l in range(kx)], r) for k in range(ky)]
    gd = [_lin([(G[i][j], yc[j]) for j in range(n)], r) for i in range(m)]  # Gamma d, the verifier's G2 side
    gc = [_lin([(G[i][j], xc[i]) for i in range(m)], r) for j in range(n)]  # Gamma^T c, the same on the G1 side
    # arguments of the target's pairing (lin_t): PPE has none (the target is a GT value in cell (1, 1))
    t = L["t"]
    one1, one2 = _iota(False, 1, a1, t1, r), _iota(False, 1, a2, t2, r)
    lt = {0: None, 1: ((0, t), one2), 2: (one1, (0, t)), 3: (one1, _iota(False, t, a2, t2, r))}[ty]
    return dict(xcoms=xc, ycoms=yc, pi=pi, theta=th, ia=ia, ib=ib, gd=gd, gc=gc, U=U[:kx], V=V[:ky], lt=lt)


def identity_cells(L, ty, r):
    """cells (a, b) -> 2a + b of the ComT comparison in which EVERY pairing on both sides has an identity argument (so
    both sides are products of nothing: f = 1 before and after the final exponentiation)"""
    mo = model(L, ty, r)
    out = []
    for a in (0, 1):
        for b in (0, 1):
            pairs = [(mo["ia"][j][a], mo["ycoms"][j][b]) for j in range(len(L["y"]))]
            pairs += [(mo["xcoms"][i][a], mo["ib"][i][b]) for i in range(len(L["x"]))]
            pairs += [(mo["xcoms"][i][a], mo["gd"][i][b]) for i in range(len(L["x"]))]
            pairs += [(mo["U"][k][a], mo["pi"][k][b]) for k in range(len(mo["U"]))]
            pairs += [(mo["theta"][k][a], mo["V"][k][b]) for k in range(len(mo["V"]))]
            if mo["lt"] is not None:
                pairs.append((mo["lt"][0][a], mo["lt"][1][b]))
            elif (a, b) == (1, 1) and L["t"] % r:
                continue  # a PPE target other than 1
            if all(p == 0 or q == 0 for p, q in pairs):
                out.append(2 * a + b)
    return out


# ---- the patterns -----------------------------------------------------------------------------------------------
# A pattern is (name, mutate, tamper, false): mutate(L, K) edits the dense logarithms L before the target is computed
# (K: r, a1, a2, t1, t2, ty); tamper(L, K) edits them AFTER it (the false twins); false: the statement is false.
def _zero_all(L, K, keys):
    for k in keys:
        v = L[k]
        L[k] = [[0] * len(v[0]) for _ in v] if isinstance(v[0], list) else [0] * len(v)


def _set(key, idx, val=0):
    def f(L, K):
        for i in ([idx] if isinstance(idx, int) else idx(L)):
            L[key][i] = val
    return f


def _both(*fs):
    def f(L, K):
        for g in fs:
            g(L, K)
    return f


def _keep(pred):
    """Gamma keeps its random entry where pred(i, j, m, n) holds and is zero elsewhere"""
    def f(L, K):
        m, n = len(L["x"]), len(L["y"])
        L["G"] = [[L["G"][i][j] if pred(i, j, m, n) else 0 for j in range(n)] for i in range(m)]
    return f


def _gamma_ones(L, K):
    L["G"] = [[1] * len(L["y"]) for _ in L["x"]]


def _rand_zero(*keys):
    return lambda L, K: _zero_all(L, K, keys)


def _row_zero(key, i):
    def f(L, K):
        L[key][i] = [0] * len(L[key][i])
    return f


def _comp_dead(side, i, comp):
    """randomness (group side, comp 1: the variable itself) that makes component `comp` of commitment i the identity"""
    def f(L, K):
        r = K["r"]
        a, t, isg = (K["a1"], K["t1"], xg(K["ty"])) if side == "x" else (K["a2"], K["t2"], yg(K["ty"]))
        var, rnd = ("x", "R") if side == "x" else ("y", "S")
        if isg and comp == 0:
            L[rnd][i] = [0, 0]  # c = (O, X)
        elif isg:  # X = -(R_i . u).1, so c = ((R_i . u).0, O)
            L[var][i] = -a * (L[rnd][i][0] + L[rnd][i][1] * t) % r
        elif comp == 0:  # scalar: c = ((x t + rho) p, (x (t a + 1) + rho a) p)
            L[rnd][i] = [-L[var][i] * t % r]
        else:
            L[rnd][i] = [-L[var][i] * (t * a + 1) * pow(a, -1, r) % r]
    return f


def _dead_com(side, i):
    var, rnd = ("x", "R") if side == "x" else ("y", "S")
    return _both(_set(var, i), _row_zero(rnd, i))


def _cancel(side):
    """x_(2k+1) = -x_2k with negated randomness, Gamma rows 2k and 2k+1 equal: every sum_i gamma_ij c_i is the identity
    from non-identity terms (side "y": the mirror image on Y, S and the columns of Gamma)"""
    def f(L, K):
        r = K["r"]
        var, rnd = ("x", "R") if side == "x" else ("y", "S")
        cnt = len(L[var])
        assert cnt % 2 == 0
        for k in range(0, cnt, 2):
            L[var][k + 1] = -L[var][k] % r
            L[rnd][k + 1] = [-v % r for v in L[rnd][k]]
            if side == "x":
                L["G"][k + 1] = list(L["G"][k])
            else:
                for row in L["G"]:
                    row[k + 1] = row[k]
    return f


def _cancel_pairs(L, K):
    L["a"][1] = L["a"][0]
    L["y"][1] = -L["y"][0] % K["r"]


def _everything(L, K):
    _zero_all(L, K, ("x", "y", "a", "b", "G", "R", "S", "T"))


def _target_plus_one(L, K):
    L["t"] = (L["t"] + 1) % K["r"]


def _gamma00_plus_one(L, K):
    L["G"][0][0] = (L["G"][0][0] + 1) % K["r"]


_all = lambda key: (lambda L: range(len(L[key])))
_mid = lambda cnt: cnt // 2
PATTERNS = [
    ("dense", None, None, False),
    ("x_one_identity", _set("x", 1), None, False),
    ("x_all_identity", _set("x", _all("x")), None, False),
    ("y_one_identity", _set("y", 2), None, False),
    ("y_all_identity", _set("y", _all("y")), None, False),
    ("const_one_identity", _both(_set("a", 0), _set("b", 3)), None, False),
    ("a_all_identity", _set("a", _all("a")), None, False),
    ("b_all_identity", _set("b", _all("b")), None, False),
    ("gamma_zero", _keep(lambda i, j, m, n: False), None, False),
    ("gamma_one_corner", _keep(lambda i, j, m, n: (i, j) == (m - 1, 0)), None, False),
    ("gamma_one_middle", _keep(lambda i, j, m, n: (i, j) == (1, 2)), None, False),
    ("gamma_diagonal", _keep(lambda i, j, m, n: i == j), None, False),
    ("gamma_zero_row", _keep(lambda i, j, m, n: i != 2), None, False),
    ("gamma_zero_col", _keep(lambda i, j, m, n: j != 1), None, False),
    ("gamma_ones", _gamma_ones, None, False),
    ("R_zero", _rand_zero("R"), None, False),
    ("S_zero", _rand_zero("S"), None, False),
    ("T_zero", _rand_zero("T"), None, False),
    ("RST_zero", _rand_zero("R", "S", "T"), None, False),
    ("R_row_zero", _row_zero("R", 1), None, False),
    ("x_comp1_dead", _comp_dead("x", 1, 1), None, False),
    ("y_comp1_dead", _comp_dead("y", 2, 1), None, False),
    ("x_comp0_dead_then_comp1_dead", _both(_comp_dead("x", 0, 0), _comp_dead("x", 1, 1)), None, False),
    ("x_dead_commitment_first", _dead_com("x", 0), None, False),
    ("x_dead_commitment_middle", _dead_com("x", 2), None, False),
    ("x_dead_commitment_last", _dead_com("x", 3), None, False),
    ("y_dead_commitment_first", _dead_com("y", 0), None, False),
    ("y_dead_commitment_middle", _dead_com("y", 1), None, False),
    ("y_dead_commitment_last", _dead_com("y", 3), None, False),
    ("cancel_x", _cancel("x"), None, False),
    ("cancel_y", _cancel("y"), None, False),
    ("cancel_pairings", _cancel_pairs, None, False),
    ("everything_identity", _everything, None, False),
    ("false_everything_identity", _everything, _target_plus_one, True),
    ("false_RST_zero", _rand_zero("R", "S", "T"), _target_plus_one, True),
    ("false_cancel_x", _cancel("x"), _gamma00_plus_one, True),
]
P = len(PATTERNS)
N = 72  # P = 36 > 33: the next N with N % 64 not in {0, 1} that holds every pattern at least twice
assert N >= 2 * P and N % 64 not in (0, 1)
FALSE_TWINS = tuple(nm for nm, _, _, f in PATTERNS if f)

# The named claims of a pattern, on top of the element-wise comparison with model():
#   ("slot", array, indices, component, needs): that component of those elements is the identity; needs = "xg" / "yg":
#       only where that side holds group elements -- otherwise the claim CANNOT HOLD for the type and is reported;
#   ("cells", {type: cells or None}): those ComT cells are all-identity products (None: cannot hold for the type);
#   ("gsum", side): every Gamma-weighted sum of the commitments of that side is the identity, from non-identity terms.
_ALL4 = (0, 1, 2, 3)
CLAIMS = {
    "R_zero": [("slot", "xcoms", _ALL4, 0, "xg")],
    "S_zero": [("slot", "ycoms", _ALL4, 0, "yg")],
    "RST_zero": [("slot", "xcoms", _ALL4, 0, "xg"), ("slot", "ycoms", _ALL4, 0, "yg"), ("slot", "pi", None, 0, None),
                 ("slot", "pi", None, 1, None), ("slot", "theta", None, 0, None), ("slot", "theta", None, 1, None),
                 ("cells", {0: (0, 1, 2), 1: (0, 1), 2: (0, 2), 3: None})],
    "R_row_zero": [("slot", "xcoms", (1,), 0, "xg")],
    "x_comp1_dead": [("slot", "xcoms", (1,), 1, None)],
    "y_comp1_dead": [("slot", "ycoms", (2,), 1, None)],
    "x_comp0_dead_then_comp1_dead": [("slot", "xcoms", (0,), 0, None), ("slot", "xcoms", (1,), 1, None)],
    "x_dead_commitment_first": [("slot", "xcoms", (0,), 0, None), ("slot", "xcoms", (0,), 1, None)],
    "x_dead_commitment_middle": [("slot", "xcoms", (2,), 0, None), ("slot", "xcoms", (2,), 1, None)],
    "x_dead_commitment_last": [("slot", "xcoms", (3,), 0, None), ("slot", "xcoms", (3,), 1, None)],
    "y_dead_commitment_first": [("slot", "ycoms", (0,), 0, None), ("slot", "ycoms", (0,), 1, None)],
    "y_dead_commitment_middle": [("slot", "ycoms", (1,), 0, None), ("slot", "ycoms", (1,), 1, None)],
    "y_dead_commitment_last": [("slot", "ycoms", (3,), 0, None), ("slot", "ycoms", (3,), 1, None)],
    "cancel_x": [("gsum", "x")],
    "cancel_y": [("gsum", "y")],
    "everything_identity": [("cells", {0: _ALL4, 1: _ALL4, 2: _ALL4, 3: _ALL4})],
}
CLAIMS["false_RST_zero"] = [c for c in CLAIMS["RST_zero"] if c[0] == "slot"]
# what selfcheck() returns, per type: the claims a type cannot hold
CANNOT = {
    0: [],
    1: ["S_zero:ycoms.0", "RST_zero:ycoms.0", "false_RST_zero:ycoms.0"],
    2: ["R_zero:xcoms.0", "RST_zero:xcoms.0", "R_row_zero:xcoms.0", "false_RST_zero:xcoms.0"],
    3: ["R_zero:xcoms.0", "S_zero:ycoms.0", "RST_zero:xcoms.0", "RST_zero:ycoms.0", "RST_zero:cells", "R_row_zero:xcoms.0",
        "false_RST_zero:xcoms.0", "false_RST_zero:ycoms.0"],
}


# ---- equations and batches --------------------------------------------------------------------------------------
_CRS = {}


def crs(cname):
    """(bytes of the binding CRS, forge.Ctx over it)"""
    if cname not in _CRS:
        c = curve(cname)
        fr = lambda v: u8(c.fr(v % c.r))
        g1 = u8(c.g1(c.golden["g1_smul"][0]["out"]))  # k = 1: the standard generators
        g2 = u8(c.g2(c.golden["g2_smul"][0]["out"]))
        p1, p2 = ref.g_mul(cname, 1, g1, fr(AL)), ref.g_mul(cname, 2, g2, fr(BE))
        binding, _ = forge.crs_pair(cname, p1, p2, TRAP["a1"], TRAP["a2"], TRAP["t1"], TRAP["t2"])
        _CRS[cname] = (binding, forge.Ctx(cname, binding))
    return _CRS[cname]


def dense_logs(rng, ty, m, n, r):
    kx, ky = (2 if xg(ty) else 1), (2 if yg(ty) else 1)
    vec = lambda k: [rng.randrange(1, r) for _ in range(k)]
    mat = lambda a, b: [vec(b) for _ in range(a)]
    return dict(x=vec(m), y=vec(n), a=vec(n), b=vec(m), G=mat(m, n), R=mat(m, kx), S=mat(n, ky), T=mat(ky, kx))


def target_log(L, r):
    m, n = len(L["x"]), len(L["y"])
    s = sum(L["a"][j] * L["y"][j] for j in range(n)) + sum(L["x"][i] * L["b"][i] for i in range(m))
    s += sum(L["x"][i] * L["G"][i][j] % r * L["y"][j] for i in range(m) for j in range(n))
    return s % r


def make_equation(cname, ty, m, n, pattern, rng):
    """One equation of `pattern` (an entry of PATTERNS): its logarithms and its arrays in boundary layout."""
    name, mutate, tamper, false = pattern
    _, cx = crs(cname)
    r = cx.r
    K = dict(TRAP, r=r, ty=ty)
    L = dense_logs(rng, ty, m, n, r)
    if mutate:
        mutate(L, K)
    L["t"] = target_log(L, r)
    if tamper:
        tamper(L, K)
    pts = lambda group, isg, vals: np.concatenate([cx.mul(group, cx.gen(group), v) if isg else cx.fr(v) for v in vals])
    t = L["t"]
    target = {0: lambda: ref.gt_pow(cname, cx.gt, cx.fr(t)), 1: lambda: cx.mul(1, cx.g1, t), 2: lambda: cx.mul(2, cx.g2, t),
              3: lambda: cx.fr(t)}[ty]()
    return dict(name=name, false=false, L=L, X=pts(1, xg(ty), L["x"]), A=pts(1, xg(ty), L["a"]), Y=pts(2, yg(ty), L["y"]),
                B=pts(2, yg(ty), L["b"]), G=cx.fr_mat(L["G"]), R=cx.fr_mat(L["R"]), S=cx.fr_mat(L["S"]), T=cx.fr_mat(L["T"]),
                target=u8(target))


IN_KEYS = ("X", "Y", "A", "B", "G", "R", "S", "T", "target")
OUT_KEYS = ("xcoms", "ycoms", "pi", "theta")
_BATCH, _EXPECTED = {}, {}


def build_batch(cname, ty, m, n, patterns, count, seed):
    """`count` equations, equation e of pattern e % len(patterns), each with the oracle's commitments, proof and verdict.
    The oracle work runs over gpubatch.pool()."""
    from gpubatch import pool

    binding, _ = crs(cname)
    rng = random.Random(seed)
    seeds = [rng.getrandbits(64) for _ in range(count)]

    def one(e):
        eq = make_equation(cname, ty, m, n, patterns[e % len(patterns)], random.Random(seeds[e]))
        out = ref.commit_and_prove(cname, ty, m, n, eq["X"], eq["Y"], eq["A"], eq["B"], eq["G"], eq["R"], eq["S"], eq["T"],
                                   binding)
        eq.update(out)
        eq["verdict"] = ref.verify(cname, ty, m, n, eq["A"], eq["B"], eq["G"], eq["target"], out["xcoms"], out["ycoms"],
                                   out["pi"], out["theta"], binding)
        return eq

    crs(cname)  # (built once, before the threads ask for it)
    eqs = list(pool().map(one, range(count)))
    return dict(cname=cname, ty=ty, m=m, n=n, N=count, crs=binding, eqs=eqs, names=[q["name"] for q in eqs],
                false=[e for e, q in enumerate(eqs) if q["false"]])


def expected(cname, ty):
    """The named batch of (curve, type) with the oracle's commitments, pi, theta and verdicts; computed once."""
    key = (cname, ty)
    if key not in _EXPECTED:
        _EXPECTED[key] = build_batch(cname, ty, M, N_, PATTERNS, N, 0x5BA55E + 16 * ty + (0 if cname == "bls12_381" else 8))
    return _EXPECTED[key]


def pack(batch, key, idx=None):
    """array `key` of the equations idx (default: all) of a batch, concatenated"""
    eqs = batch["eqs"] if idx is None else [batch["eqs"][e] for e in idx]
    if key == "verdict":
        return np.array([q["verdict"] for q in eqs], dtype=np.uint8)
    return np.concatenate([q[key] for q in eqs])


# ---- the proof of presence --------------------------------------------------------------------------------------
def check_equation(cname, ty, eq, crs_bytes, cannot):
    """One equation against the oracle: verdict, every commitment / proof element against model(), the named claims."""
    _, cx = crs(cname)
    r, name, L = cx.r, eq["name"], eq["L"]
    m, n = len(L["x"]), len(L["y"])
    assert eq["verdict"] == (0 if eq["false"] else 1), (cname, ty, name, "oracle verdict", eq["verdict"])
    mo = model(L, ty, r)
    for key, group in (("xcoms", 1), ("ycoms", 2), ("pi", 2), ("theta", 1)):
        sz = cx.size(group)
        for s, lg in enumerate(v for pair in mo[key] for v in pair):
            got = eq[key][s * sz:(s + 1) * sz]
            assert bool(got.any()) == (lg != 0), (cname, ty, name, key, s // 2, s % 2, "identity where none is claimed"
                                                   if lg else "no identity where one is claimed")
            assert (got == cx.mul(group, cx.gen(group), lg)).all(), (cname, ty, name, key, s // 2, s % 2)
    one = np.zeros(cx.GT, np.uint8)
    one[:cx.FQ] = u8(cx.c.fq(1))
    for claim in CLAIMS.get(name, ()):
        if claim[0] == "slot":
            _, key, idx, comp, needs = claim
            if (needs == "xg" and not xg(ty)) or (needs == "yg" and not yg(ty)):
                cannot.add("%s:%s.%d" % (name, key, comp))
                continue
            for i in (range(len(mo[key])) if idx is None else idx):
                if comp < 2 and i < len(mo[key]):
                    assert mo[key][i][comp] == 0, (cname, ty, name, key, i, comp)
        elif claim[0] == "cells":
            cells = claim[1][ty]
            if cells is None:
                cannot.add("%s:cells" % name)
                continue
            assert tuple(identity_cells(L, ty, r)) == tuple(cells), (cname, ty, name, identity_cells(L, ty, r))
            ok, lhs, rhs, _ = ref.verify_cells(cname, ty, m, n, eq["A"], eq["B"], eq["G"], eq["target"], eq["xcoms"],
                                               eq["ycoms"], eq["pi"], eq["theta"], crs_bytes)
            for c in cells:
                assert (lhs[c] == one).all() and (rhs[c] == one).all(), (cname, ty, name, "cell", c)
        else:  # the Gamma-weighted sums, recomputed with the oracle's left_mul
            G = L["G"]
            if claim[1] == "x":
                sums = ref.left_mul(cname, 1, n, m, cx.fr_mat(_tr(G)), eq["xcoms"])
                terms, key = eq["xcoms"].reshape(2 * m, -1), "gc"
            else:
                sums = ref.left_mul(cname, 2, m, n, cx.fr_mat(G), eq["ycoms"])
                terms, key = eq["ycoms"].reshape(2 * n, -1), "gd"
            assert not sums.any() and all(v == (0, 0) for v in mo[key]), (cname, ty, name, "sum is not the identity")
            assert all(t.any() for t in terms) and all(g for row in G for g in row), (cname, ty, name, "identity term")
    if not eq["false"] and name != "dense":
        # every all-identity cell the model finds (claimed or not) is a cell the oracle calls good with f = 1
        cells = identity_cells(L, ty, r)
        if cells and not any(c[0] == "cells" for c in CLAIMS.get(name, ())):
            ok, lhs, rhs, _ = ref.verify_cells(cname, ty, m, n, eq["A"], eq["B"], eq["G"], eq["target"], eq["xcoms"],
                                               eq["ycoms"], eq["pi"], eq["theta"], crs_bytes)
            for c in cells:
                assert (lhs[c] == one).all() and (rhs[c] == one).all(), (cname, ty, name, "cell", c)


def selfcheck(cname, ty, batch=None):
    """Everything the batch claims, against oracle/gs_ref.c.  Returns the sorted names of the claims the type cannot hold
    (CANNOT[ty] for the named batch)."""
    from gpubatch import pool

    b = expected(cname, ty) if batch is None else batch
    assert [q["name"] for q in b["eqs"]] == [b["names"][e] for e in range(b["N"])]
    false_names = {b["names"][e] for e in b["false"]}
    if batch is None:
        assert b["N"] == N and b["names"] == [PATTERNS[e % P][0] for e in range(N)]
        assert false_names == set(FALSE_TWINS) and all(b["names"].count(nm) >= 2 for nm, _, _, _ in PATTERNS)
    cannot = set()
    list(pool().map(lambda eq: check_equation(cname, ty, eq, b["crs"], cannot), b["eqs"]))
    return sorted(cannot)

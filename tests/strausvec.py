"""Rows for the Straus lanes (k_var_multi{4,8}[w5][x2|x4], k_var_tab8) behind gs_mat_left_mul_com1/2 under the forced
shapes, a model of one lane on discrete logarithms, and the proof that the rows hold what they claim.
tests/test_straus_cpu.py runs it on the CPU, tests/test_gpu_straus_edges.py puts the rows on the device.

Pure Python on top of scalarvec.Model (decompose, recode, nd_of, eig); no engine import.  The model only CLASSIFIES the
additions of a lane; every expected point is the oracle's [log] generator.

  walk(cname, group, W, scalars, base_logs)   the device loop of jac_straus_run step by step: Walk(top, events, final)
  groups(k, tm)                               the balanced group sizes add_var_terms gives k terms
  rows(cname, group, k)                       [Row(label, kind, scalars)] in launch order; cols(k) the column logarithms
  selfcheck(cname, group, W, tm)              the conditions of DESIGN.md ("The Straus lanes ..."); returns what cannot be
                                              built, by name (CANNOT pins it)

Columns.  Column j of the call is the commitment (c.0, c.1) = (COLS[j][0] g, COLS[j][1] g): per component the bases
(P, -P, P, P, Q, -Q, Q, Q), then the identity and two half identities -- repeated, negated and identity bases as in
test_gpu_scalar_edges.test_mat_left_mul_table, in the order the built rows need.

Built rows.  Inside one lane the running sum meets the next table entry when everything added so far sums to that entry.
With a and b confined to ONE sub-scalar stream s (recombine, kept only if decompose maps them back to that stream alone):
  quad  (a, a, b, b) on (P, -P, P, P): a cancels in every window (`cancel`, then doublings and the next first addition on
        the identity); b = d 2^(W i) adds d eig^s P to the identity and then to itself (`double`) in window i.  a is
        shorter than b (i is the top window), longer with 0 < i < top, or longer with i = 0.
  pair  (a, a') on (P, -P), a' = a with the digit of window i negated: the windows above cancel, window i doubles.  This
        is the form that fits a two-term lane.
For k >= 8 the quads also sit on terms 4 .. 7 (Q), alone and behind a quad on P."""
import functools
from collections import namedtuple

import scalarvec as S

WIDTHS = (4, 5, 8)
# the k every forced group size runs at (test_gpu_straus_edges.py): k = 9 gives 5 + 4 under tm = 8, 3 x 3 under tm = 4 and
# a one-term group under tm = 2; k = 5 gives 3 + 2 under tm = 4; k = 1 and 2 are short groups in the 4- and 8-term instances
KS = {2: (8, 9), 4: (1, 5, 8, 9), 8: (1, 2, 8, 9)}
KS_TAB = (2, 8, 9)  # shared base tables (W = 8, groups of <= 8 terms)
COLS = [(2, 3), (-2, -3), (2, 3), (2, 3), (5, 7), (-5, -7), (5, 7), (5, 7), (0, 0), (1, 0), (0, 1)]
EDGE = ["r-1", "one", "nibbles_8", "nibbles_7", "(r+1)/2", "quints_10000"]
LABELS = ("generic", "acc_identity", "addend_identity", "double", "cancel")
# Streams that cannot be isolated: on BN254 the floor-rounded lattice reduction maps +-mag eig^s (s > 0) to sub-scalars in
# several streams for every magnitude the built rows need, so only stream 0 (small k: every c_i = 0) carries built rows.
CANNOT = {
    ("bls12_381", 1): [],
    ("bls12_381", 2): [],
    ("bn254", 1): ["stream1"],
    ("bn254", 2): ["stream1", "stream2", "stream3"],
}

Event = namedtuple("Event", "window slot term stream digit label")
Walk = namedtuple("Walk", "top events final")
Row = namedtuple("Row", "label kind scalars")


# ---- the lane model -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _digits(cname, group, W, k):
    m = S.model(cname)
    d = m.decompose(group, k)
    return tuple(tuple(S.recode(v, m.NL[group], W)) for v in d.mags), tuple(d.signs)


@functools.lru_cache(maxsize=None)
def _eigs(cname, group):
    m = S.model(cname)
    return tuple(pow(m.eig[group], s, m.r) for s in range(m.NS[group]))


def walk(cname, group, W, scalars, base_logs, order=None):
    """One lane of jac_straus_run<C, F, TMAX, W> over `scalars` (canonical) on the bases [base_logs[t]] generator: `top`
    as the kernel computes it, windows from `top` down with W doublings between them, slot k = t * NS + s inside a window;
    the running sum and every addend as logarithms mod `order` (r).  A zero digit adds nothing and has no event."""
    m = S.model(cname)
    r = order or m.r
    NS, ND = m.NS[group], S.nd_of(m.NL[group], W)
    eig = _eigs(cname, group)
    streams = []  # slot k -> (digits, negated, log of eig^s P_t)
    for t, k in enumerate(scalars):
        dg, sg = _digits(cname, group, W, k % r)
        for s in range(NS):
            streams.append((dg[s], sg[s], eig[s] * base_logs[t] % r))
    top = 0
    for dg, _, _ in streams:
        for i in range(ND - 1, top, -1):
            if dg[i] != 0:
                top = i
                break
    acc, events = 0, []
    for i in range(top, -1, -1):
        if i != top:
            acc = (acc << W) % r
        for k, (dg, neg, log) in enumerate(streams):
            a = dg[i]
            if a == 0:
                continue
            add = (-a if neg else a) * log % r
            if add == 0:
                label = "addend_identity"
            elif acc == 0:
                label = "acc_identity"
            elif acc == add:
                label = "double"
            elif (acc + add) % r == 0:
                label = "cancel"
            else:
                label = "generic"
            events.append(Event(i, k, k // NS, k % NS, a, label))
            acc = (acc + add) % r
    assert acc == sum(k * b for k, b in zip(scalars, base_logs)) % r, (cname, group, W, [hex(k) for k in scalars])
    return Walk(top, events, acc)


def groups(k, tm):
    """sizes of the balanced groups of at most tm terms (add_var_terms)"""
    ng = (k + tm - 1) // tm
    return [k // ng + (1 if g < k % ng else 0) for g in range(ng)]


def lanes_of(k, tm):
    """[(first term, size)] of the lanes one component of a row runs in"""
    out, t0 = [], 0
    for n in groups(k, tm):
        out.append((t0, n))
        t0 += n
    return out


def cols(k):
    return COLS[:k]


# ---- built rows ---------------------------------------------------------------------------------------------------------
def isolate(cname, group, s, mag):
    """the canonical scalar whose sub-scalars are `mag` in stream s and 0 elsewhere, or None"""
    m = S.model(cname)
    want = [mag if j == s else 0 for j in range(m.NS[group])]
    for sign in (0, 1):
        k = m.recombine(group, want, [sign] * m.NS[group])
        d = m.decompose(group, k)
        if list(d.mags) == want:
            assert m.recombine(group, d.mags, d.signs) == k
            return k
    return None


def _mag(digits, W):
    v = sum(d << (W * i) for i, d in enumerate(digits))
    assert v > 0
    return v


@functools.lru_cache(maxsize=None)
def built(cname, group, W):
    """({(stream, kind, where, #): scalars of the terms it occupies}, streams that could not be isolated)"""
    m = S.model(cname)
    half = 1 << (W - 1)
    out, failed = {}, []
    for s in range(m.NS[group]):
        iso = lambda digits: isolate(cname, group, s, _mag(digits, W))
        # (where, window of b, digits of a from window 0 up)
        shapes = [("top", 2, [-5, 3]), ("middle", 1, [-6, 2 - half, 7]), ("window0", 0, [half - 2, -4, 3])]
        got = {}
        for where, i, adig in shapes:
            a = iso(adig)
            for n, d in enumerate((half - 1, 3)):
                b = iso([0] * i + [d])
                got[(s, "quad", where, n)] = None if a is None or b is None else (a, a, b, b)
        for where, i in (("middle", 1), ("window0", 0)):
            for n, dig in enumerate(([half - 1, 6, 2], [-5, 1 - half, 9])):
                other = list(dig)
                other[i] = -other[i]
                a, a2 = iso(dig), iso(other)
                got[(s, "pair", where, n)] = None if a is None or a2 is None else (a, a2)
        if all(v is None for v in got.values()):
            failed.append("stream%d" % s)
        else:
            assert all(v is not None for v in got.values()), (cname, group, W, s)
            out.update(got)
    return out, failed


def _built_rows(cname, group, k):
    rows = []
    for W in WIDTHS:
        for (s, kind, where, n), sc in sorted(built(cname, group, W)[0].items()):
            tag = "W%d stream %d %s %s #%d" % (W, s, kind, where, n)
            pad = lambda lst: list(lst) + [0] * (k - len(lst))
            if kind == "pair":
                if k >= 2:
                    rows.append(Row(tag, "built", pad(sc)))
            elif k >= 4:
                rows.append(Row(tag + " on P", "built", pad(sc)))
                if k >= 8 and n == 0:
                    rows.append(Row(tag + " on Q", "built", pad([0, 0, 0, 0] + list(sc))))
                    rows.append(Row(tag + " on P and Q", "built", pad(list(sc) * 2)))
    return rows


def _identity_rows(cname, k):
    m = S.model(cname)
    named = S.by_name(cname)
    rows = [Row("all zero", "identity", [0] * k)]
    for nm in EDGE:
        s = named[nm]
        if k >= 2:
            rows.append(Row("(s, s) on (P, -P), s = " + nm, "identity", [s, s] + [0] * (k - 2)))
        if k >= 3:
            rows.append(Row("(s, r - s) on (P, P), s = " + nm, "identity", [s, 0, m.r - s] + [0] * (k - 3)))
    return rows


def lane_count(nrows, k, tm, mo):
    """lanes of the launch: every (component, group) is a family of nrows outputs, mo to a lane"""
    return 2 * len(groups(k, tm)) * ((nrows + mo - 1) // mo)


def shapes_of(k):
    """(tm, mo) of every forced launch the rows of this k go through"""
    out = [(tm, mo) for tm, ks in KS.items() if k in ks for mo in (1, 2, 4)]
    return out + ([(8, 1)] if k in KS_TAB else [])


@functools.lru_cache(maxsize=None)
def rows(cname, group, k):
    """Table rows (k consecutive table scalars, shifted cyclically: every scalar visits every term position), identity
    and degenerate rows, built collisions -- the special rows spread evenly between the dense ones, so that every wave and
    every multi-output lane holds both.  The count is 3 (mod 4), and no forced launch has 0 or 1 (mod 64) lanes: dense
    rows are appended (the cyclic shift goes on) until both hold."""
    ks = S.scalars(cname)
    n = len(ks)
    special = _identity_rows(cname, k) + [Row("last term alone", "identity", [0] * (k - 1) + [ks[3]])]
    special += _built_rows(cname, group, k)
    ndense = n
    while (ndense + len(special)) % 4 != 3 or any(lane_count(ndense + len(special), k, tm, mo) % 64 in (0, 1)
                                                  for tm, mo in shapes_of(k)):
        ndense += 1
    dense = [Row("row %d (%s ...)" % (i, S.name_of(cname, ks[i % n])), "table", [ks[(i + j) % n] for j in range(k)])
             for i in range(ndense)]
    total, ns = ndense + len(special), len(special)
    out, si, di = [], 0, 0
    at = {(j * total) // ns for j in range(ns)}  # the first row is special, the last ones (the short lane) are dense
    for i in range(total):
        if i in at:
            out.append(special[si])
            si += 1
        else:
            out.append(dense[di])
            di += 1
    assert si == ns and di == ndense
    return out


def row_logs(cname, row, k):
    """the logarithms of the two components of the row's output"""
    r = S.model(cname).r
    return tuple(sum(v * c[comp] for v, c in zip(row.scalars, COLS[:k])) % r for comp in (0, 1))


# ---- proof of presence --------------------------------------------------------------------------------------------------
def _where(ev, top):
    return "top" if ev.window == top else "window0" if ev.window == 0 else "middle"


def selfcheck(cname, group, W, tm):
    """The rows of every k this group size runs at, walked lane by lane under window width W.  Asserts the conditions
    listed in DESIGN.md and returns the names of what could not be built (CANNOT[cname, group])."""
    m = S.model(cname)
    NS, NL = m.NS[group], m.NL[group]
    ND = S.nd_of(NL, W)
    table = S.scalars(cname)
    bl, failed = built(cname, group, W)
    isolated = sorted({key[0] for key in bl})
    assert 0 in isolated
    labels = set()
    at = {}  # (label, stream, where) -> count, over lanes that hold a built row
    after_cancel, sizes = 0, set()
    for k in (KS_TAB if W == 8 else KS[tm]):
        rws = rows(cname, group, k)
        assert len(rws) % 4 == 3
        for t, mo in shapes_of(k):
            assert lane_count(len(rws), k, t, mo) % 64 not in (0, 1)
        # both kinds of row in every block of 64 rows (a wave at one output per lane) and around every built row
        kinds = [rw.kind == "table" for rw in rws]
        # (k = 1 has two special rows, the zero scalar and the last-term row: nothing collides inside one term)
        for b0 in range(0, len(rws) - 63 if k > 1 else 0, 64):
            assert any(kinds[b0:b0 + 64]) and not all(kinds[b0:b0 + 64]), (k, b0)
        for i, rw in enumerate(rws):
            if rw.kind == "built":
                assert any(kinds[i - i % 4:i - i % 4 + 4]) and any(kinds[i - i % 2:i - i % 2 + 2]), (k, i)
        # every table scalar at every term position
        for j in range(k):
            assert {rw.scalars[j] for rw in rws if rw.kind == "table"} == set(table), (k, j)
        gs_ = lanes_of(k, tm)
        sizes.update(n for _, n in gs_)
        if len({n for _, n in gs_}) > 1:
            sizes.add("unequal")
        for rw in rws:
            for comp in (0, 1):
                total = 0
                for t0, n in gs_:
                    wk = walk(cname, group, W, rw.scalars[t0:t0 + n], [c[comp] for c in COLS[t0:t0 + n]])
                    total += wk.final
                    labels.update(ev.label for ev in wk.events)
                    if rw.kind != "built":
                        continue
                    cancel_at = None
                    for ev in wk.events:
                        key = (ev.label, ev.stream, _where(ev, wk.top))
                        at[key] = at.get(key, 0) + 1
                        if ev.label == "cancel" and 0 < ev.window:
                            cancel_at = ev.window
                        if ev.label == "acc_identity" and cancel_at is not None and ev.window < cancel_at:
                            after_cancel += 1
                assert total % m.r == row_logs(cname, rw, k)[comp], rw.label
            if rw.kind == "identity" and rw.label != "last term alone":
                assert row_logs(cname, rw, k) == (0, 0), rw.label
    assert labels == set(LABELS), sorted(set(LABELS) - labels)
    for s in isolated:
        for where in ("top", "middle", "window0"):
            for label in ("double", "cancel"):
                assert at.get((label, s, where), 0) >= 2, (cname, group, W, tm, label, s, where)
    if len(isolated) > 1:  # an entry that went through endo_apply
        assert any(at.get(("double", s, wh), 0) for s in isolated if s > 0 for wh in ("top", "middle", "window0"))
    assert after_cancel >= 2
    # nt = 1 (on the shared tables the shortest group run is two terms), nt = tm, unequal groups
    assert {2 if W == 8 else 1, tm, "unequal"} <= sizes, sizes
    if W == 8:
        decs = [m.decompose(group, k) for k in table]
        for s in range(NS):
            streams = [S.recode(d.mags[s], NL, 8) for d in decs]
            assert any(-128 in dg for dg in streams), s
            assert sum(1 for dg in streams if 127 in dg) >= 2, s
            assert any(d.mags[s] and max(i for i, v in enumerate(dg) if v) >= -(-d.mags[s].bit_length() // 8)
                       for d, dg in zip(decs, streams)), s
            can = S.stream_bound(cname, group, s) >= S.spare_threshold(ND, 8)
            assert any(dg[-1] == 1 for dg in streams) == can, (s, can)
    return failed

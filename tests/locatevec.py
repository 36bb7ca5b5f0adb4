"""Pure-Python model of the fault localisation of gs_verify_batch_rlc_locate.

A K-ary tree over N leaves: level 0 = the leaves, node (l, i) = the product of nodes (l - 1, i K .. i K + K - 1) that
exist, the root is the only node of the top level (level 0 itself when N = 1).  The descent checks the root, then every
child of every failing node; nothing is inferred from siblings.

  descend(passes, N, K) -> (ok[N], n_bad, n_checks)   passes(level, index) -> bool
  from_pairs(pairs, K, mul, eq) -> passes              pairs[e] = (W_e, T_e); a node passes iff prod W == prod T
"""


def level_sizes(N, K):
    """nodes per level, leaves first"""
    assert N >= 1 and K >= 2
    sizes = [N]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + K - 1) // K)
    return sizes


def descend(passes, N, K):
    sizes = level_sizes(N, K)
    top = len(sizes) - 1
    ok = [1] * N
    checks = 1
    frontier = [] if passes(top, 0) else [0]
    if top == 0:
        for e in frontier:
            ok[e] = 0
        return ok, len(frontier), checks
    for level in range(top - 1, -1, -1):
        nxt = []
        for p in frontier:
            for c in range(p * K, min(p * K + K, sizes[level])):
                checks += 1
                if not passes(level, c):
                    nxt.append(c)
        frontier = nxt
    for e in frontier:
        ok[e] = 0
    return ok, len(frontier), checks


def from_pairs(pairs, K, mul, eq):
    """The predicate over products of per-leaf (W, T) pairs: the levels are built once, as the device keeps them."""
    levels = [list(pairs)]
    while len(levels[-1]) > 1:
        below, here = levels[-1], []
        for i in range(0, len(below), K):
            w, t = below[i]
            for w2, t2 in below[i + 1:i + K]:
                w, t = mul(w, w2), mul(t, t2)
            here.append((w, t))
        levels.append(here)

    def passes(level, index):
        w, t = levels[level][index]
        return bool(eq(w, t))

    return passes


def checks_formula(bad, N, K):
    """1 for the root plus the number of children of every failing internal node, when a node fails iff a bad leaf lies
    under it (no cancellation)."""
    sizes = level_sizes(N, K)
    checks = 1
    marked = set(bad)
    for level in range(1, len(sizes)):
        marked = {i // K for i in marked}
        for i in marked:
            checks += min(i * K + K, sizes[level - 1]) - i * K
    return checks

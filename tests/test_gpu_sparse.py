"""The sparse and degenerate batch of tests/sparsevec.py under every forced kernel shape.

test_gpu_variants.py puts RANDOM dense batches through every kernel shape the planner can pick; its degenerate inputs
(test_gpu_batch.py::test_edge_values_against_c_oracle) only ever meet the shapes planned for small batches, and are false
statements, on which a verifier that mishandles an identity answers "false" like a correct one.  Here every equation is
a TRUE statement carrying one degenerate pattern (identity variables / constants, sparse Gamma, commitments without
randomness, a dead component, a dead commitment, sums cancelling to the identity, everything the identity -- the
patterns and their proof of presence are in sparsevec.py, checked on the CPU by test_sparse_cpu.py), plus three named
false twins, and for every shape of test_gpu_variants.SHAPES, all four types, both curves:
  * commitments, pi and theta of EVERY equation equal the cached oracle bytes (oracle/gs_ref.c);
  * the exact verdicts equal the oracle's: 1 everywhere but on the false twins;
  * a second pass under the library's profile shows the kernels of expected_kernels and gives identical outputs.
The patterns change no plan (a plan depends on the type and the arity, never on the data), so the kernel names are those
of test_gpu_variants.expected_kernels as they stand.  The verifier is also run ALONE on the oracle's commitments and
proofs (a fault of the prover cannot then hide one of the verifier), and the batched verifier on the batch without and
with a false twin.  Every case makes its own engine and closes it; the oracle's arrays are computed once per (curve,
type) by sparsevec.expected and shared.

Wall time of this file next to test_gpu_variants.py (the yardstick, 104 cases of the same shape): see DESIGN.md 4.1."""
import fnmatch

import numpy as np
import pytest

import sparsevec as sv
from test_gpu_variants import SHAPES, expected_kernels

pytestmark = pytest.mark.gpu

CURVE_IDS = [("bls12_381", 0), ("bn254", 1)]
PAIR_SHAPE = "pair12_straus8x2w5_lane"


class Run:
    """One engine with `opts` over a batch of sparsevec (all of it, or the equations idx), arrays on the device."""

    def __init__(self, cid, batch, opts=None, idx=None):
        import torch

        import groth_sahai_rs_amd as gs

        self.b, self.idx = batch, list(range(batch["N"])) if idx is None else list(idx)
        self.N, self.ty, self.m, self.n = len(self.idx), batch["ty"], batch["m"], batch["n"]
        self.eng = gs.Engine(cid, 0)
        try:
            for k, v in (opts or {}).items():
                self.eng.set_option(k, v)
            self.eng.set_crs(batch["crs"])
            self.h = {k: sv.pack(batch, k, self.idx) for k in sv.IN_KEYS + sv.OUT_KEYS + ("verdict",)}
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
            self.d = {k: dev(self.h[k]) for k in sv.IN_KEYS}
            self.out = {k: torch.zeros(self.h[k].size, dtype=torch.uint8, device="cuda:0") for k in sv.OUT_KEYS}
            self.ok = torch.full((self.N,), 7, dtype=torch.uint8, device="cuda:0")
        except BaseException:
            self.eng.close()
            raise

    def close(self):
        self.eng.close()

    def name(self, e):
        return "%s (equation %d)" % (self.b["names"][self.idx[e]], self.idx[e])

    def prove(self):
        d, o = self.d, self.out
        self.eng.prove_batch_dev(self.ty, self.N, self.m, self.n, d["X"], d["Y"], d["A"], d["B"], d["G"], d["R"], d["S"],
                                 d["T"], o["xcoms"], o["ycoms"], o["pi"], o["theta"])
        self.eng.sync()

    def proofs(self, oracle):
        """the four proof arrays on the device: the prover's outputs, or the oracle's"""
        import torch

        if not oracle:
            return [self.out[k] for k in sv.OUT_KEYS]
        return [torch.from_numpy(self.h[k]).to("cuda:0") for k in sv.OUT_KEYS]

    def verify(self, oracle=False):
        d = self.d
        self.ok.fill_(7)
        self.eng.verify_batch_dev(self.ty, self.N, self.m, self.n, d["A"], d["B"], d["G"], d["target"],
                                  *self.proofs(oracle), self.ok)
        self.eng.sync()
        return self.ok.cpu().numpy()

    def rlc(self, oracle=True):
        import os

        import torch

        d = self.d
        raw = np.frombuffer(os.urandom(self.N * 32), dtype=np.uint64).copy()
        raw[raw == 0] = 1
        rho = torch.from_numpy(raw.view(np.int64)).to("cuda:0")
        acc = torch.empty(2 * self.eng.GT, dtype=torch.uint8, device="cuda:0")
        self.eng.verify_batch_rlc_dev(self.ty, self.N, self.m, self.n, d["A"], d["B"], d["G"], d["target"],
                                      *self.proofs(oracle), rho, acc)
        self.eng.sync()
        return self.eng.gt_finalize(acc.cpu().numpy())

    def check_outputs(self, what):
        for k in sv.OUT_KEYS:
            got, want = self.out[k].cpu().numpy().reshape(self.N, -1), self.h[k].reshape(self.N, -1)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (what, k, [self.name(e) for e in bad[:6]])

    def check_verdicts(self, ok, what):
        bad = np.nonzero(ok != self.h["verdict"])[0]
        assert bad.size == 0, (what, "verdict", [(self.name(e), int(ok[e])) for e in bad[:6]])


def check_batch(cid, batch, opts, expect, what):
    """prove + verify against the oracle's arrays; with `expect`, again under the profile: kernel names, same outputs"""
    assert [int(v) for v in sv.pack(batch, "verdict")] == [0 if e in batch["false"] else 1 for e in range(batch["N"])]
    r = Run(cid, batch, opts)
    try:
        r.prove()
        r.check_outputs(what)
        r.check_verdicts(r.verify(), what)
        if expect is not None:
            r.eng.prof_enable(True)
            r.eng.prof_reset()
            for o in r.out.values():
                o.zero_()
            r.prove()
            ok = r.verify()
            names = [p[0] for p in r.eng.prof_get()]
            r.eng.prof_enable(False)
            for want in expect:
                assert any(fnmatch.fnmatchcase(nm, want) for nm in names), (what, want, names)
            r.check_outputs(what + ("profiled pass",))
            r.check_verdicts(ok, what + ("profiled pass",))
        return r.h
    finally:
        r.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("ty", [0, 1, 2, 3])
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_sparse_batch_under_forced_shapes(cname, cid, ty, shape):
    o = SHAPES[shape]
    check_batch(cid, sv.expected(cname, ty), o, expected_kernels(ty, sv.M, sv.N_, o), (cname, ty, shape))


@pytest.mark.parametrize("ty", [0, 1, 2, 3])
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_sparse_batch_planned(cname, cid, ty):
    """no option set: the shapes the planner picks for 72 equations"""
    check_batch(cid, sv.expected(cname, ty), None, None, (cname, ty, "planned"))


@pytest.mark.parametrize("ty", [0, 1, 2, 3])
def test_claims_a_type_cannot_hold_are_the_pinned_ones(ty):
    """Nothing is skipped silently: the claims of sparsevec.CLAIMS that a type cannot hold (a commitment to a SCALAR without
    randomness is x (u1 + (O, p1)), with no dead component) are exactly these."""
    pinned = {
        0: [],
        1: ["RST_zero:ycoms.0", "S_zero:ycoms.0", "false_RST_zero:ycoms.0"],
        2: ["RST_zero:xcoms.0", "R_row_zero:xcoms.0", "R_zero:xcoms.0", "false_RST_zero:xcoms.0"],
        3: ["RST_zero:cells", "RST_zero:xcoms.0", "RST_zero:ycoms.0", "R_row_zero:xcoms.0", "R_zero:xcoms.0",
            "S_zero:ycoms.0", "false_RST_zero:xcoms.0", "false_RST_zero:ycoms.0"],
    }
    assert sv.selfcheck("bn254", ty) == pinned[ty]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("ty", [0, 3])
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_verifier_alone_on_oracle_proofs(cname, cid, ty, shape):
    """The verifier never sees the prover's output here: commitments, pi and theta are the oracle's."""
    r = Run(cid, sv.expected(cname, ty), SHAPES[shape])
    try:
        r.check_verdicts(r.verify(oracle=True), (cname, ty, shape, "verifier alone"))
    finally:
        r.close()


@pytest.mark.parametrize("shape", [None, PAIR_SHAPE])
@pytest.mark.parametrize("ty", [0, 1, 2, 3])
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_batched_verifier(cname, cid, ty, shape):
    """verify_batch_rlc on the oracle's proofs: the batch without the false twins is accepted; with ONE false twin put
    back (one of each family in turn) it is rejected.  Planned, and under one pair-lane shape."""
    b = sv.expected(cname, ty)
    true = [e for e in range(b["N"]) if e not in b["false"]]
    opts = SHAPES[shape] if shape else None
    r = Run(cid, b, opts, true)
    try:
        assert r.rlc() == 1, (cname, ty, shape, "true statements rejected")
    finally:
        r.close()
    for fam in sv.FALSE_TWINS:
        e = [k for k in b["false"] if b["names"][k] == fam][0]
        r = Run(cid, b, opts, sorted(true + [e]))
        try:
            assert r.rlc() == 0, (cname, ty, shape, fam, "accepted")
        finally:
            r.close()


# ---- tree folds at small arity ------------------------------------------------------------------------------------
FOLD_ARITY = 8
FOLD_OPTS = dict(miller_twin=0, miller_ch=1, var_tm=1)
_FOLD = {}


def fold_patterns():
    by = {p[0]: p for p in sv.PATTERNS}

    def diag_alt(L, K):  # diagonal Gamma, every second constant the identity
        sv._keep(lambda i, j, m, n: i == j)(L, K)
        L["a"][1::2] = [0] * len(L["a"][1::2])
        L["b"][0::2] = [0] * len(L["b"][0::2])

    return [("gamma_diagonal_alternate_constants", diag_alt, None, False), by["RST_zero"], by["cancel_x"],
            by["false_RST_zero"]]


def fold_batch(cname, ty):
    if (cname, ty) not in _FOLD:
        _FOLD[(cname, ty)] = sv.build_batch(cname, ty, FOLD_ARITY, FOLD_ARITY, fold_patterns(), 4, 0xF01D + ty)
    return _FOLD[(cname, ty)]


@pytest.mark.parametrize("ty", [0, 3])
@pytest.mark.parametrize("cname,cid", CURVE_IDS)
def test_tree_folds_meet_identity_partials(cname, cid, ty):
    """k_cell_fold (GT) and k_slot_fold (G1 / G2) only run above 16 partials per cell / per output component.  With one
    pair per Miller task and one term per Straus lane (miller_ch = 1, var_tm = 1) every pair and every term is its own
    partial, and the smallest m = n at which the profile shows BOTH folds is 8 (cells of 3 m + 4 = 28 pairs fold from
    m = 5 on; the proof elements sum 2 m + 2 terms per component: 18 at m = 8, 16 at m = 7).  Three true statements whose
    partials are mostly identities -- a diagonal Gamma with every second constant the identity, R = S = T = 0, the
    cancelling pattern on all m rows -- and one false twin, against the oracle.  PPE shows both folds.  The same four
    equations of QuadEqu run at this arity too, against the oracle alone: its profile shows neither fold up to m = 9
    (measured with the same options), so no kernel name is asserted for it."""
    b = fold_batch(cname, ty)
    assert b["false"] == [3]
    sv.selfcheck(cname, ty, b)
    check_batch(cid, b, FOLD_OPTS, ["k_cell_fold", "k_slot_fold.*"] if ty == 0 else [], (cname, ty, "folds"))

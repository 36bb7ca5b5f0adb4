"""One table of named engine calls for the tests of a context's history and stream (tests/test_gpu_ctx_history.py,
tests/test_gpu_streams.py).

A call is a closure over fixed, seeded inputs: host arrays in, named output arrays out.  Its EXPECTED bytes are what a
fresh context gives on the default stream with a full synchronisation, and that fresh result is held to the oracle
(oracle/gs_ref_py.py: commit_and_prove, verify, g_mul, multi_pairing, gt_pow, left_mul) before it is cached -- on every
entry while N <= 5, else on four sampled entries that include the first, the last and every forged one.  The tests then
compare byte for byte with these bytes after other calls, on other streams and beside other contexts, so their
reference is the oracle and not merely another run of the same code.

Names are tuples:
  ("prove", ty, N, m, n)                     gs_prove_batch_dev                     ("prove_host", ...) gs_prove_batch
  ("verify", ty, N, m, n, flavour)           gs_verify_batch_dev                    ("verify_host", ...) gs_verify_batch
  ("rlc", ty, N, m, n, flavour, count)       gs_verify_batch_rlc_dev, then gs_gt_finalize over `count` copies of the pair
  ("rlc_host", ty, N, m, n, flavour)         gs_verify_batch_rlc
  ("locate", ty, N, m, n, flavour)           gs_verify_batch_rlc_locate_dev
  ("eqrlc", ty, N, m, n, flavour)            gs_verify_equation_rlc_dev, then gs_gt_finalize
  ("stmtrlc", ty, S, E, flavour)             gs_verify_statements_rlc_dev: S statements of E equations, shared commitments
  ("rerand", ty, N, m, n)                    gs_rerandomize_batch_dev               ("rerand_host", ...) gs_rerandomize_batch
  ("commit", kind, N, m)                     gs_commit_{g1,g2,fr_b1,fr_b2}_dev over the (kind's type, N, m, m) batch's variables
  ("extract", group, N, m)                   gs_extract_g1_dev / _g2_dev over the commitments of the PPE (N, m, m) batch
  ("xscalar", N)                             gs_extract_scalar_b1_dev (16-bit scalars, 2^8 baby steps)
  ("gmul", group, N)  ("mpair", N, k)  ("gtpow", N)  ("leftmul", group, rows, k)  ("validate", group, N)
  ("mixed", N)                               gs_verify_mixed_dev: a forged PPE (2,3) part and a valid QUAD (4,4) part
flavour: "valid" | "forged" (FORGED_AT(N) entries carry a well-formed wrong theta).
Every batch of a curve lives under ONE CRS (that of Workload at SEED), whose binding key is known."""
import ctypes
import os
import sys

import numpy as np

from gsutil import REPO, curve

sys.path.insert(0, os.path.join(REPO, "oracle"))

CURVES = [(0, "bls12_381"), (1, "bn254")]
SEED = 4242
TYPES = (0, 1, 2, 3)
NS = (1, 5, 65, 300)  # one lane, a few, one lane past a wave, a partial last workgroup
SHAPES = ((1, 1), (2, 3), (4, 4), (6, 2))
GROW = (1024, 4, 4)  # the grower of every family: later calls of a sequence are smaller than what its buffers hold
DEV = "cuda:0"
DLOG_LOG2, DLOG_BITS = 8, 16


# acc[0] of the batched verifiers is the UN-exponentiated Miller product (include/gs_amd.h): tabulated CRS lines and
# stepped ones differ by factors of a proper subfield, which the final exponentiation removes.  Its bytes therefore
# follow these options (name: default); verdicts, and every other family's bytes, follow none.
ACC_OPTIONS = {"line_tables": 1}
ACC_FAMILIES = ("rlc", "rlc_host", "locate", "eqrlc")


def FORGED_AT(N):
    return (0,) if N == 1 else tuple(sorted({N // 3, N - 1}))


def sample(N, forged=()):
    """indices held to the oracle: all while N <= 5, else first, last, two in between and every forged one"""
    if N <= 5:
        return list(range(N))
    return sorted({0, N - 1, N // 2, (2 * N) // 3 + 1} | set(forged))


class Call:
    def __init__(self, name, ins, outs, run, post=None, oracle=None, host=False, key=False, dlog=False, alias=None):
        self.name, self.ins, self.outs, self.run, self.post, self.oracle = name, ins, outs, run, post, oracle
        self.host, self.key, self.dlog, self.alias = host, key, dlog, alias


def pack(out):
    return b"".join(np.ascontiguousarray(out[k]).view(np.uint8).tobytes() for k in sorted(out))


def diff(got, want):
    """where two packed results differ (for assertion messages)"""
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return "sizes %d != %d" % (a.size, b.size)
    w = np.nonzero(a != b)[0]
    return "%d of %d bytes differ, first at %d" % (w.size, a.size, w[0]) if w.size else "equal"


def device_buffers(call):
    """inputs uploaded, outputs filled with 0xFF (a kernel that leaves part of an output unwritten shows)"""
    import torch

    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in call.ins.items()}
    for k, nb in call.outs.items():
        d[k] = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return d


def run_plain(eng, call):
    """the call on the engine's current stream, a sync, the outputs (dict of host arrays)"""
    if call.host:
        out = call.run(eng, dict(call.ins))
    else:
        d = device_buffers(call)
        call.run(eng, d)
        eng.sync()
        out = {k: d[k].cpu().numpy() for k in call.outs}
    if call.post:
        out.update(call.post(eng, out))
    return out


class World:
    """Everything of one curve: the CRS and its key, an anchor engine that keeps the CRS tables alive (a fresh context
    then shares them instead of building 1.8 GB), the batches and the oracle-checked expected bytes."""

    def __init__(self, cid, cname):
        import groth_sahai_rs_amd as gs
        from groth_sahai_rs_amd.workload import CURVES as WC, SplitMix64, Workload, _limbs

        self.gs, self.cid, self.cname, self.c = gs, cid, cname, curve(cname)
        self.r = WC[cid]["r"]
        self.eng = gs.Engine(cid, 0)
        wl = Workload(self.eng, ty=0, N=1, m=1, n=1, seed=SEED, corrupt_every=0)
        self.crs, self.p1, self.p2, self.gt = wl.crs.copy(), wl.g1_gen.copy(), wl.g2_gen.copy(), wl.gt_gen.copy()
        sm = SplitMix64(SEED)  # the draws of Workload's CRS: al, be, a1, a2, t1, t2
        sc = [(sm.next() | (sm.next() << 64) | (sm.next() << 128)) % self.r for _ in range(6)]
        self.fr = lambda vals: np.array([_limbs(v * (1 << 256) % self.r, 4) for v in vals],
                                        dtype=np.uint64).reshape(-1).view(np.uint8)
        self.key = self.fr([sc[2], sc[3]])
        self.rng = np.random.default_rng(SEED + cid)
        self.batches, self.calls, self.want, self.eqb, self.ins = {}, {}, {}, {}, {}
        self.Workload = Workload

    def scalars(self, count):
        raw = self.rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        return [(int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192) % self.r for a, b, c, d in raw]

    # ---- fresh contexts ------------------------------------------------------------------------------------------
    def fresh(self, crs=None):
        e = self.gs.Engine(self.cid, 0)
        e.set_crs(self.crs if crs is None else crs)
        return e

    def prepare(self, eng, call):
        """the context state a call needs beyond the CRS: the binding key, the dlog table"""
        if call.key and not getattr(eng, "_ctxhist_key", False):
            eng.set_extraction_key(self.key)
            eng._ctxhist_key = True  # (the tests that drop the key or the CRS reset this)
        if call.dlog and eng.dlog_table(1) is None:
            eng.dlog_prepare(1, self.p1, DLOG_LOG2)

    def expected(self, name, opts=()):
        """oracle-checked bytes of a fresh context on the default stream.  opts: ((option, value), ...) set in that
        fresh context first -- only for ACC_OPTIONS, which the un-exponentiated accumulator acc[0] of the batched
        verifiers is a function of (its verdict is not, and the oracle check is the same)."""
        self.expected_many([(name, opts)])
        return self.want[(name, tuple(opts))]

    def expected_many(self, pairs):
        """expected() for many (name, opts): the fresh runs one after the other, then all their oracle checks side by
        side (the oracle is C behind ctypes; its own per-entry pool is another one, so nothing waits on itself)"""
        first = []  # the proofs the other calls take as inputs: a wave of their own, so that they are made once
        for name, _ in pairs:
            first += [(d, ()) for d in self.deps(name) if (d, ()) not in self.want and (d, ()) not in first]
        if first and [p for p in pairs if (p[0], tuple(p[1])) not in first]:
            self.expected_many(first)
        todo = []
        for name, opts in pairs:
            key = (name, tuple(opts))
            if key in self.want or any(k == key for k, _, _ in todo):
                continue
            call = self.call(name)
            if call.alias is not None:  # a host-pointer form: the bytes of its device form
                self.expected_many([(call.alias, opts)])
                self.want[key] = self.want[(call.alias, tuple(opts))]
                continue
            e = self.fresh()
            try:
                for k, v in opts:
                    e.set_option(k, v)
                self.prepare(e, call)
                out = run_plain(e, call)
            finally:
                e.close()
            todo.append((key, call, out))
        if len(todo) == 1:
            if todo[0][1].oracle:
                todo[0][1].oracle(todo[0][2])
        elif todo:
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=8) as ex:
                list(ex.map(lambda t: t[1].oracle(t[2]) if t[1].oracle else None, todo))
        for key, call, out in todo:  # cached only once the oracle agreed
            self.want[key] = pack(out)

    @staticmethod
    def deps(name):
        f = name[0]
        if f in ("prove", "verify", "verify_host", "rlc", "rlc_host", "locate", "rerand", "rerand_host", "prove_host"):
            return [("prove",) + tuple(name[1:5])]
        if f == "commit":
            return [("prove", dict(g1=0, g2=0, fr_b1=3, fr_b2=3)[name[1]], name[2], name[3], name[3])]
        if f == "extract":
            return [("prove", 0, name[2], name[3], name[3])]
        if f == "mixed":
            return [("prove", 0, name[1], 2, 3), ("prove", 3, name[1], 4, 4)]
        return []

    def inputs(self, ty, N, m, n):
        """host arrays of a satisfied batch (Workload at SEED)"""
        key = (ty, N, m, n)
        if key not in self.ins:
            wl = self.Workload(self.eng, ty=ty, N=N, m=m, n=n, seed=SEED, corrupt_every=0)
            assert (wl.crs == self.crs).all()
            b = {k: getattr(wl, k).cpu().numpy() for k in ("X", "Y", "A", "B", "Gamma", "R", "S", "T", "target")}
            b["sh"] = wl.sh
            self.ins[key] = b
        return self.ins[key]

    # ---- batches -------------------------------------------------------------------------------------------------
    def batch(self, ty, N, m, n):
        """host arrays of a satisfied batch and its proof; the proof is the fresh, oracle-checked result of the
        ("prove", ty, N, m, n) call"""
        key = (ty, N, m, n)
        if key not in self.batches:
            b = dict(self.inputs(ty, N, m, n))
            self.batches[key] = b
            want = np.frombuffer(self.expected(("prove", ty, N, m, n)), np.uint8)
            sz = self.eng._sizes(ty, N, m, n)
            o = 0
            for k in sorted(("xcoms", "ycoms", "pi", "theta")):  # pack() order
                b[k] = want[o:o + sz[k]].copy()
                o += sz[k]
            # the forged flavour: a well-formed wrong theta (the two G1 components of its first commitment swapped)
            th = b["theta"].copy().reshape(N, -1)
            g1 = self.eng.G1
            for e in FORGED_AT(N):
                th[e, :2 * g1] = np.concatenate([th[e, g1:2 * g1], th[e, :g1]])
            b["theta_forged"] = th.reshape(-1)
        return self.batches[key]

    def vargs(self, b, flavour):
        return dict(A=b["A"], B=b["B"], Gamma=b["Gamma"], target=b["target"], xcoms=b["xcoms"], ycoms=b["ycoms"],
                    pi=b["pi"], theta=b["theta_forged" if flavour == "forged" else "theta"])

    def cut(self, ty, N, m, n, arrays, e):
        sz = self.eng._sizes(ty, N, m, n)
        return {k: a[e * (sz[k] // N):(e + 1) * (sz[k] // N)] for k, a in arrays.items()}

    def oracle_verdicts(self, ty, N, m, n, v, idx):
        import gs_ref_py as ref
        from gpubatch import pool

        def one(e):
            a = self.cut(ty, N, m, n, v, e)
            return ref.verify(self.cname, ty, m, n, a["A"], a["B"], a["Gamma"], a["target"], a["xcoms"], a["ycoms"],
                              a["pi"], a["theta"], self.crs)

        return dict(zip(idx, pool().map(one, idx)))

    def rho(self, N):
        raw = np.random.default_rng(SEED + 17 * N).integers(1, 1 << 63, size=4 * N, dtype=np.uint64)
        return raw.view(np.uint8)

    # ---- the table -----------------------------------------------------------------------------------------------
    def call(self, name):
        if name not in self.calls:
            self.calls[name] = getattr(self, "_" + name[0])(*name[1:])
            self.calls[name].name = name
        return self.calls[name]

    def _prove(self, ty, N, m, n):
        import gs_ref_py as ref
        from gpubatch import pool

        b = self.inputs(ty, N, m, n)
        keys = ("X", "Y", "A", "B", "Gamma", "R", "S", "T")
        ins = {k: b[k] for k in keys}
        sz = self.eng._sizes(ty, N, m, n)
        outs = {k: sz[k] for k in ("xcoms", "ycoms", "pi", "theta")}

        def run(eng, d):
            eng.prove_batch_dev(ty, N, m, n, *(d[k] for k in keys), d["xcoms"], d["ycoms"], d["pi"], d["theta"])

        def oracle(out):
            def one(e):
                a = self.cut(ty, N, m, n, ins, e)
                o = ref.commit_and_prove(self.cname, ty, m, n, *(a[k] for k in keys), self.crs)
                g = self.cut(ty, N, m, n, out, e)
                return [k for k in outs if not (o[k] == g[k]).all()]

            idx = sample(N)
            bad = [(e, r) for e, r in zip(idx, pool().map(one, idx)) if r]
            assert not bad, ("fresh prove differs from the oracle", self.cname, ty, N, m, n, bad[:4])

        return Call(None, ins, outs, run, oracle=oracle)

    def _prove_host(self, ty, N, m, n):
        c = self.call(("prove", ty, N, m, n))
        keys = ("X", "Y", "A", "B", "Gamma", "R", "S", "T")
        return Call(None, c.ins, c.outs, lambda eng, d: eng.prove_batch(ty, N, m, n, *(d[k] for k in keys)), host=True,
                    alias=("prove", ty, N, m, n))

    VK = ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta")

    def _verdict_oracle(self, ty, N, m, n, flavour, ins, verdicts):
        """verdicts(out) -> ok[N]: equal to the known forged set everywhere and to the oracle on the sample"""
        forged = FORGED_AT(N) if flavour == "forged" else ()

        def oracle(out):
            ok = verdicts(out)
            want = np.ones(N, dtype=np.uint8)
            want[list(forged)] = 0
            assert (ok == want).all(), ("fresh verdicts", self.cname, ty, N, m, n, flavour, np.nonzero(ok != want)[0][:8])
            ref = self.oracle_verdicts(ty, N, m, n, ins, sample(N, forged))
            assert all(ok[e] == v for e, v in ref.items()), ("oracle verdicts", self.cname, ty, N, m, n, flavour, ref)

        return oracle

    def _verify(self, ty, N, m, n, flavour):
        ins = self.vargs(self.batch(ty, N, m, n), flavour)

        def run(eng, d):
            eng.verify_batch_dev(ty, N, m, n, *(d[k] for k in self.VK), d["ok"])

        return Call(None, ins, dict(ok=N), run, oracle=self._verdict_oracle(ty, N, m, n, flavour, ins, lambda o: o["ok"]))

    def _verify_host(self, ty, N, m, n, flavour):
        c = self.call(("verify", ty, N, m, n, flavour))
        return Call(None, c.ins, c.outs, lambda eng, d: dict(ok=eng.verify_batch(ty, N, m, n, *(d[k] for k in self.VK))),
                    host=True, alias=("verify", ty, N, m, n, flavour))

    def _all_oracle(self, ty, N, m, n, flavour, ins):
        """ok_all == (no forged entry), and the sampled entries have the oracle's verdict"""
        forged = FORGED_AT(N) if flavour == "forged" else ()

        def oracle(out):
            assert int(out["ok_all"][0]) == (0 if forged else 1), ("fresh batched verdict", self.cname, ty, N, m, n, flavour)
            ref = self.oracle_verdicts(ty, N, m, n, ins, sample(N, forged))
            assert all(v == (0 if e in forged else 1) for e, v in ref.items()), ("oracle verdicts", ref)

        return oracle

    def _rlc(self, ty, N, m, n, flavour, count):
        ins = self.vargs(self.batch(ty, N, m, n), flavour)
        rins = dict(ins, rho=self.rho(N))

        def run(eng, d):
            eng.verify_batch_rlc_dev(ty, N, m, n, *(d[k] for k in self.VK), d["rho"], d["acc"])

        def post(eng, out):
            return dict(ok_all=np.array([eng.gt_finalize(np.tile(out["acc"], count))], dtype=np.uint8))

        return Call(None, rins, dict(acc=2 * self.eng.GT), run, post=post, oracle=self._all_oracle(ty, N, m, n, flavour, ins))

    def _rlc_host(self, ty, N, m, n, flavour):
        c = self.call(("rlc", ty, N, m, n, flavour, 1))

        def run(eng, d):
            ok_all, acc = eng.verify_batch_rlc(ty, N, m, n, *(d[k] for k in self.VK), d["rho"].view(np.uint64))
            return dict(acc=acc, ok_all=np.array([ok_all], dtype=np.uint8))

        return Call(None, c.ins, c.outs, run, host=True, alias=("rlc", ty, N, m, n, flavour, 1))

    def _locate(self, ty, N, m, n, flavour):
        ins = self.vargs(self.batch(ty, N, m, n), flavour)
        rins = dict(ins, rho=self.rho(N))

        def run(eng, d):
            eng.verify_batch_rlc_locate_dev(ty, N, m, n, *(d[k] for k in self.VK), d["rho"], d["acc"], d["ok"], d["info"])

        base = self._verdict_oracle(ty, N, m, n, flavour, ins, lambda o: o["ok"])

        def oracle(out):
            base(out)
            assert int(out["info"].view(np.uint32)[0]) == (len(FORGED_AT(N)) if flavour == "forged" else 0)

        return Call(None, rins, dict(acc=2 * self.eng.GT, ok=N, info=8), run, oracle=oracle)

    def _eqrlc(self, ty, N, m, n, flavour):
        import eqrlcdata
        import gs_ref_py as ref
        from gpubatch import pool

        if (ty, N, m, n) not in self.eqb:
            self.eqb[(ty, N, m, n)] = eqrlcdata.make_batch(self.cname, self.cid, ty, N, m, n, seed=SEED)
        bt = self.eqb[(ty, N, m, n)]
        assert (bt.crs == self.crs).all()
        forged = FORGED_AT(N) if flavour == "forged" else ()
        cat = lambda k: np.concatenate([p[k] for p in bt.proofs])
        th = cat("theta").reshape(N, -1)
        g1 = self.eng.G1
        for e in forged:
            th[e, :2 * g1] = np.concatenate([th[e, g1:2 * g1], th[e, :g1]])
        ins = dict(A=bt.const["A"], B=bt.const["B"], Gamma=bt.const["G"], target=bt.const["target"], xcoms=cat("xcoms"),
                   ycoms=cat("ycoms"), pi=cat("pi"), theta=th.reshape(-1), rho=self.rho(N))

        def run(eng, d):
            eng.verify_equation_rlc_dev(ty, N, m, n, *(d[k] for k in self.VK), d["rho"], d["acc"])

        def post(eng, out):
            return dict(ok_all=np.array([eng.gt_finalize(out["acc"])], dtype=np.uint8))

        def oracle(out):
            assert int(out["ok_all"][0]) == (0 if forged else 1), ("fresh equation verdict", self.cname, ty, N, m, n, flavour)
            per = lambda k, e: ins[k].reshape(N, -1)[e]

            def one(e):
                return ref.verify(self.cname, ty, m, n, ins["A"], ins["B"], ins["Gamma"], ins["target"], per("xcoms", e),
                                  per("ycoms", e), per("pi", e), per("theta", e), self.crs)

            idx = sample(N, forged)
            got = dict(zip(idx, pool().map(one, idx)))
            assert all(v == (0 if e in forged else 1) for e, v in got.items()), ("oracle verdicts", got)

        return Call(None, ins, dict(acc=2 * self.eng.GT), run, post=post, oracle=oracle)

    def _stmtrlc(self, ty, S, E, flavour):
        """S statements of E equations each over the shared variables of stmtutil.StatementInputs (the shape follows the
        type); forged: one equation of statement S // 2 (and of the last one) carries a wrong theta"""
        import gs_ref_py as ref
        from gpubatch import pool
        from stmtutil import StatementInputs

        if "stmt" not in self.eqb:
            self.eqb["stmt"] = StatementInputs(self.eng, seed=SEED)
            assert (self.eqb["stmt"].crs == self.crs).all()
        st = self.eqb["stmt"]
        forged = FORGED_AT(S) if flavour == "forged" else ()
        parts, g1 = [], self.eng.G1
        for s in range(S):
            p = st.part(ty, E)
            m, n = p["m"], p["n"]
            o = self.eng.prove_statement(ty, E, m, n, *(p[k] for k in ("X", "Y", "A", "B", "Gamma", "R", "S", "T")))
            p.update({k: np.ascontiguousarray(v).reshape(-1) for k, v in o.items()})
            if s in forged:
                th = p["theta"].reshape(E, -1)
                th[E // 2, :2 * g1] = np.concatenate([th[E // 2, g1:2 * g1], th[E // 2, :g1]])
            parts.append(p)
        cat = lambda k: np.concatenate([np.ascontiguousarray(p[k]).view(np.uint8).reshape(-1) for p in parts])
        ins = {k: cat(k) for k in self.VK}
        ins["rho"] = self.rho(S * E)

        def run(eng, d):
            eng.verify_statements_rlc_dev(ty, S, E, m, n, *(d[k] for k in self.VK), d["rho"], d["acc"], d["ok"])

        def oracle(out):
            want = np.ones(S, dtype=np.uint8)
            want[list(forged)] = 0
            assert (out["ok"] == want).all(), ("fresh statement verdicts", self.cname, ty, S, E, flavour, out["ok"])
            sz = self.eng._sizes(ty, E, m, n, True)

            def one(se):
                s, e = se
                p = parts[s]
                c = lambda k: np.ascontiguousarray(p[k]).view(np.uint8).reshape(-1)[e * (sz[k] // E):(e + 1) * (sz[k] // E)]
                return ref.verify(self.cname, ty, m, n, c("A"), c("B"), c("Gamma"), c("target"), p["xcoms"], p["ycoms"],
                                  c("pi"), c("theta"), self.crs)

            idx = [(s, e) for s in sample(S, forged) for e in sorted({0, E // 2, E - 1})]
            got = dict(zip(idx, pool().map(one, idx)))
            assert all(v == (0 if (s in forged and e == E // 2) else 1) for (s, e), v in got.items()), ("oracle verdicts", got)

        return Call(None, ins, dict(acc=S * 2 * self.eng.GT, ok=S), run, oracle=oracle)

    RK = ("A", "B", "Gamma", "xcoms", "ycoms", "pi", "theta", "R", "S", "T")

    def _rerand(self, ty, N, m, n):
        b = self.batch(ty, N, m, n)
        kx, ky = b["sh"]["kx"], b["sh"]["ky"]
        ins = {k: b[k] for k in self.RK[:7]}
        ins.update(R=self.fr(self.scalars(N * m * kx)), S=self.fr(self.scalars(N * n * ky)), T=self.fr(self.scalars(N * ky * kx)))
        sz = self.eng._sizes(ty, N, m, n)
        onames = ("xcoms_out", "ycoms_out", "pi_out", "theta_out")
        outs = {k: sz[k[:-4]] for k in onames}

        def run(eng, d):
            eng.rerandomize_batch_dev(ty, N, m, n, *(d[k] for k in self.RK), *(d[k] for k in onames))

        def oracle(out):  # the oracle has no rerandomizer: its verifier accepts the new proofs, and they are new
            v = dict(A=b["A"], B=b["B"], Gamma=b["Gamma"], target=b["target"], xcoms=out["xcoms_out"],
                     ycoms=out["ycoms_out"], pi=out["pi_out"], theta=out["theta_out"])
            ref = self.oracle_verdicts(ty, N, m, n, v, sample(N))
            assert all(x == 1 for x in ref.values()), ("oracle rejects a rerandomized proof", self.cname, ty, N, m, n, ref)
            for k in onames:
                assert (out[k].reshape(N, -1) != b[k[:-4]].reshape(N, -1)).any(axis=1).all(), k

        return Call(None, ins, outs, run, oracle=oracle)

    def _rerand_host(self, ty, N, m, n):
        c = self.call(("rerand", ty, N, m, n))

        def run(eng, d):
            o = eng.rerandomize_batch(ty, N, m, n, *(d[k] for k in self.RK))
            return {k + "_out": v for k, v in o.items()}

        return Call(None, c.ins, c.outs, run, host=True, alias=("rerand", ty, N, m, n))

    def _commit(self, kind, N, m):
        """the commitments of a batch's variables through the commit entry: the bytes the prover gave (oracle-checked)"""
        ty = dict(g1=0, g2=0, fr_b1=3, fr_b2=3)[kind]
        b = self.batch(ty, N, m, m)
        x = kind in ("g1", "fr_b1")
        ins = dict(v=b["X" if x else "Y"], r=b["R" if x else "S"])
        want = b["xcoms" if x else "ycoms"]
        fn = "gs_commit_%s_dev" % kind

        def run(eng, d):
            eng._chk(getattr(eng.lib, fn)(eng.ctx, ctypes.c_size_t(N * m), ctypes.c_void_p(d["v"].data_ptr()),
                                          ctypes.c_void_p(d["r"].data_ptr()), ctypes.c_void_p(d["out"].data_ptr())))

        def oracle(out):
            assert (out["out"] == want).all(), ("fresh commit differs from the prover's commitments", self.cname, kind, N, m)

        return Call(None, ins, dict(out=want.size), run, oracle=oracle)

    def _extract(self, group, N, m):
        """opening the PPE batch's commitments gives back its witness"""
        b = self.batch(0, N, m, m)
        ins = dict(coms=b["xcoms" if group == 1 else "ycoms"])
        want = b["X" if group == 1 else "Y"]

        def oracle(out):
            assert (out["out"] == want).all(), ("fresh extraction is not the witness", self.cname, group, N, m)

        return Call(None, ins, dict(out=want.size), lambda eng, d: eng.extract_dev(group, d["coms"], d["out"]),
                    oracle=oracle, key=True)

    def _xscalar(self, N):
        xs = [int(v) for v in np.random.default_rng(SEED + N).integers(0, 1 << DLOG_BITS, size=N)]
        xs[0], xs[-1] = 0, (1 << DLOG_BITS) - 1
        want = self.fr(xs)
        coms = self.eng.commit("fr_b1", want.view(np.uint64), self.fr(self.scalars(N)).view(np.uint64)).reshape(-1)

        def oracle(out):
            assert out["found"].all() and (out["out"] == want).all(), ("fresh scalar extraction", self.cname, N)

        return Call(None, dict(coms=coms), dict(out=N * 32, found=N),
                    lambda eng, d: eng.extract_scalar_dev(1, d["coms"], DLOG_BITS, d["out"], d["found"]), oracle=oracle,
                    key=True, dlog=True)

    def _points(self, group, N):
        ks = self.fr(self.scalars(N))
        base = self.p1 if group == 1 else self.p2
        return self.eng.g_mul_batch(group, base, ks.view(np.uint64), broadcast=True).reshape(-1)

    def _gmul(self, group, N):
        import gs_ref_py as ref
        from gpubatch import pool

        gsz = self.eng.G1 if group == 1 else self.eng.G2
        ins = dict(p=self._points(group, N), k=self.fr(self.scalars(N)))
        ins["k"][:32] = 0  # a zero scalar: the identity

        def oracle(out):
            idx = sample(N)
            one = lambda e: ref.g_mul(self.cname, group, ins["p"][e * gsz:(e + 1) * gsz], ins["k"][e * 32:(e + 1) * 32])
            for e, w in zip(idx, pool().map(one, idx)):
                assert (out["out"][e * gsz:(e + 1) * gsz] == w).all(), ("fresh g_mul", self.cname, group, N, e)

        return Call(None, ins, dict(out=N * gsz), lambda eng, d: eng.g_mul_batch_dev(group, N, d["p"], False, d["k"], d["out"]),
                    oracle=oracle)

    def _mpair(self, N, k):
        import gs_ref_py as ref
        from gpubatch import pool

        E = self.eng
        ins = dict(P=self._points(1, N * k), Q=self._points(2, N * k))

        def oracle(out):
            idx = sample(N)
            one = lambda e: ref.multi_pairing(self.cname, k, ins["P"][e * k * E.G1:(e + 1) * k * E.G1],
                                              ins["Q"][e * k * E.G2:(e + 1) * k * E.G2])
            for e, w in zip(idx, pool().map(one, idx)):
                assert (out["out"][e * E.GT:(e + 1) * E.GT] == w).all(), ("fresh multi_pairing", self.cname, N, k, e)

        return Call(None, ins, dict(out=N * E.GT), lambda eng, d: eng.multi_pairing_batch_dev(N, k, d["P"], d["Q"], d["out"]),
                    oracle=oracle)

    def _gtpow(self, N):
        import gs_ref_py as ref
        from gpubatch import pool

        GT = self.eng.GT
        ins = dict(base=self.gt, k=self.fr(self.scalars(N)))

        def oracle(out):
            idx = sample(N)
            one = lambda e: ref.gt_pow(self.cname, self.gt, ins["k"][e * 32:(e + 1) * 32])
            for e, w in zip(idx, pool().map(one, idx)):
                assert (out["out"][e * GT:(e + 1) * GT] == w).all(), ("fresh gt_pow", self.cname, N, e)

        return Call(None, ins, dict(out=N * GT), lambda eng, d: eng.gt_pow_batch_dev(N, d["base"], d["k"], d["out"]),
                    oracle=oracle)

    def _leftmul(self, group, rows, k):
        import gs_ref_py as ref

        col = self._points(group, 2 * k)  # k commitments
        ins = dict(lhs=self.fr(self.scalars(rows * k)), col=col)

        def oracle(out):
            assert (out["out"].reshape(-1) == ref.left_mul(self.cname, group, rows, k, ins["lhs"], col)).all(), "fresh left_mul"

        return Call(None, ins, dict(out=0), lambda eng, d: dict(out=eng.mat_left_mul(group, rows, k, d["lhs"], d["col"])),
                    oracle=oracle, host=True)

    def _validate(self, group, N):
        """subgroup points, the identity, and points with x and y swapped (off the curve)"""
        gsz = self.eng.G1 if group == 1 else self.eng.G2
        pts = self._points(group, N).reshape(N, gsz).copy()
        want = np.ones(N, dtype=np.uint8)
        for e in range(0, N, 3):
            pts[e] = np.concatenate([pts[e, gsz // 2:], pts[e, :gsz // 2]])
            want[e] = 0
        if N > 1:
            pts[N - 1], want[N - 1] = 0, 1

        def run(eng, d):
            eng._chk(eng.lib.gs_validate_points_dev(eng.ctx, group, ctypes.c_size_t(N), ctypes.c_void_p(d["pts"].data_ptr()),
                                                    ctypes.c_void_p(d["ok"].data_ptr())))

        def oracle(out):
            assert (out["ok"] == want).all(), ("fresh validate_points", self.cname, group, N, out["ok"], want)

        return Call(None, dict(pts=pts.reshape(-1)), dict(ok=N), run, oracle=oracle)

    def _mixed(self, N):
        """two parts in one call; each part's verdicts are those of its own (oracle-checked) verify call"""
        parts = [(0, N, 2, 3, "forged"), (3, N, 4, 4, "valid")]
        ins = {}
        for i, (ty, n_, m, n, fl) in enumerate(parts):
            ins.update({"%s%d" % (k, i): v for k, v in self.vargs(self.batch(ty, n_, m, n), fl).items()})

        def run(eng, d):
            eng.verify_mixed_dev([dict(ty=ty, N=n_, m=m, n=n, ok=d["ok%d" % i], **{k: d["%s%d" % (k, i)] for k in self.VK})
                                  for i, (ty, n_, m, n, fl) in enumerate(parts)])

        def oracle(out):
            for i, (ty, n_, m, n, fl) in enumerate(parts):
                assert out["ok%d" % i].tobytes() == self.expected(("verify", ty, n_, m, n, fl)), ("fresh mixed part", i)

        return Call(None, ins, {"ok0": N, "ok1": N}, run, oracle=oracle)


_WORLDS = {}


def world(cid, cname):
    if cid not in _WORLDS:
        _WORLDS[cid] = World(cid, cname)
    return _WORLDS[cid]


# ---- running a call on a caller's stream ------------------------------------------------------------------------------
FILLER_MIN_MS = 20.0  # a whole small batch takes 17.5-19 ms (README): nothing mis-streamed lands after the inputs
_FILLER = {}


def filler(stream):
    """Bounded work on `stream` (a chain of matmuls sized once per session for about twice FILLER_MIN_MS); returns the
    two events around it.  Never a spin on a flag."""
    import torch

    if not _FILLER:
        a = torch.rand(4096, 4096, device=DEV)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):  # the second pass is timed: the first pays for library loading
            e0.record()
            x = a
            for _ in range(8):
                x = torch.mm(x, a) * (1.0 / 2048)
            e1.record()
            torch.cuda.synchronize()
        per = max(e0.elapsed_time(e1) / 8, 1e-3)
        _FILLER.update(a=a, n=int(2.0 * FILLER_MIN_MS / per) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        x = _FILLER["a"]
        for _ in range(_FILLER["n"]):
            x = torch.mm(x, _FILLER["a"]) * (1.0 / 2048)
        e1.record(stream)
    return e0, e1


def stage(call, ins=None):
    """device copies of the inputs (`ins`, default the call's own) and 0xFF-filled buffers for inputs and outputs; the
    device is synchronised afterwards"""
    import torch

    ins = call.ins if ins is None else ins
    src = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ins.items()}
    d = {k: torch.full((v.numel(),), 0xFF, dtype=torch.uint8, device=DEV) for k, v in src.items()}
    for k, nb in call.outs.items():
        d[k] = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return src, d


def enqueue(eng, call, stream, staged=None, fill=True):
    """The call on a caller's stream, nothing synchronised afterwards: the buffers hold 0xFF until the real inputs are
    copied in ON the stream, behind a filler when `fill`; the outputs are cloned on the stream.  `stream` None: the
    default stream (no filler).  `staged`: what stage() returned (then nothing here synchronises before the call
    either).  Returns a handle for collect()."""
    import torch

    assert not call.host
    src, d = staged if staged is not None else stage(call)
    eng.set_stream(stream.cuda_stream if stream is not None else 0)
    ev = filler(stream) if fill and stream is not None else None
    with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
        for k in src:
            d[k].copy_(src[k], non_blocking=True)
        call.run(eng, d)
        clones = {k: d[k].clone() for k in call.outs}
    return dict(src=src, d=d, clones=clones, ev=ev, stream=stream)


def collect(h, call, which="clones"):
    """the outputs of an enqueued call once its stream has been synchronised, and the filler's milliseconds (asserted
    to be at least FILLER_MIN_MS)"""
    out = {k: h[which][k].cpu().numpy() for k in call.outs}
    ms = None
    if h["ev"] is not None:
        ms = h["ev"][0].elapsed_time(h["ev"][1])
        assert ms >= FILLER_MIN_MS, "the filler took %.1f ms, below the %.0f ms window" % (ms, FILLER_MIN_MS)
    return out, ms


def on_stream(eng, call, stream, sync="stream", fill=True):
    """A launch, memset or copy that the engine sends anywhere but the caller's stream (or to a side stream that does
    not wait for it) runs during the filler, on 0xFF inputs, or after the clones were taken.  A detector with a wide
    window, not a proof.  Returns (outputs, filler milliseconds).
    sync="engine": gs_sync alone, then blocking copies of the output buffers themselves."""
    h = enqueue(eng, call, stream, fill=fill)
    if sync == "stream":
        stream.synchronize()
        out, ms = collect(h, call)
    else:
        eng.sync()
        out, ms = collect(h, call, "d")
        stream.synchronize()
    if call.post:
        out.update(call.post(eng, out))
    return out, ms


def unpack(call, packed):
    """pack() undone for a device call without a post step: dict of its output arrays"""
    a, o, out = np.frombuffer(packed, np.uint8), 0, {}
    for k in sorted(call.outs):
        out[k] = a[o:o + call.outs[k]]
        o += call.outs[k]
    assert o == a.size
    return out

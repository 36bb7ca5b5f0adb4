"""What the host plans and launches, as text that two builds of the library can be compared by.  For a fixed list of
small calls, one line per case on stdout: the count and a hash of the library's `[plan]` lines for the case (under
GS_PLAN_TRACE: every task table the planner uploads with name, size and content hash, and the lane shapes it chose),
then every kernel launched as `name launches lanes work`, in first-seen order.  No times.  The `[plan]` lines themselves
go to stderr, for finding what changed when a hash does.  A refactor of the plan-building code must leave stdout
byte-identical:
    python tools/plan_digest.py > head.txt
    GS_AMD_LIB=/path/to/parent/libgs_amd.so python tools/plan_digest.py > parent.txt
profiles/plan_digest/ keeps such a pair.  Inputs are valid group elements (a Workload's prove); its arrays are reused,
as prefixes, for the statement and one-equation forms, so whether a check passes is not part of the digest."""
import hashlib
import os
import sys
import tempfile

os.environ["GS_PLAN_TRACE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import Workload

TYPES = ((gs.GS_PPE, "PPE"), (gs.GS_MSMEG1, "MSMEG1"), (gs.GS_MSMEG2, "MSMEG2"), (gs.GS_QUAD, "QuadEqu"))
DEFAULTS = dict(miller_twin=-1, endo=1, coop_fe=1, locate_k=0, eq_pi=-1)
VERIFY_KEYS = ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta")
PROVE_KEYS = ("X", "Y", "A", "B", "Gamma", "R", "S", "T")
RERAND_KEYS = ("A", "B", "Gamma", "xcoms", "ycoms", "pi", "theta", "R", "S", "T")


class Cases:
    def __init__(self, eng, curve_name):
        self.eng, self.curve = eng, curve_name
        eng.prof_enable(True)

    def run(self, label, fn, **opts):
        """one case: the options, the call, then its launches"""
        for k, v in opts.items():
            self.eng.set_option(k, v)
        tag = "%s %s%s" % (self.curve, label, "".join(" %s=%d" % kv for kv in sorted(opts.items())))
        print("[plan] == " + tag, file=sys.stderr, flush=True)
        self.eng.prof_reset()
        # the library writes its [plan] lines to file descriptor 2: into a file for the length of the call
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                fn()
                self.eng.sync()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            err = tmp.read()
        sys.stderr.buffer.write(err)
        sys.stderr.flush()
        plan = [ln for ln in err.split(b"\n") if ln.startswith(b"[plan]")]
        launches = {name: n for name, _, n in self.eng.prof_get()}
        kernels = ["%s %d %d %d" % (name, launches[name], lanes, work)
                   for name, (lanes, work) in self.eng.prof_get_work().items()]
        print("%s: plan %d %s: %s" % (tag, len(plan), hashlib.sha256(b"\n".join(plan)).hexdigest()[:16], ", ".join(kernels)),
              flush=True)
        for k in opts:
            self.eng.set_option(k, DEFAULTS[k])


def host_arrays(wl):
    return {k: getattr(wl, k).cpu().numpy() for k in set(VERIFY_KEYS + PROVE_KEYS)}


def shape_cases(cs, ty, tname, m, n):
    eng = cs.eng
    wl = Workload(eng, ty=ty, N=9, m=m, n=n, corrupt_every=0)
    wl.prove()
    eng.sync()
    h = host_arrays(wl)
    rho = np.random.default_rng(7).integers(1, 1 << 63, size=4 * 9, dtype=np.uint64)

    def take(keys, N, shared=False, one_equation=False, copies=1):
        """the first bytes of the workload's arrays, as many as a call of N equations wants"""
        want = eng._sizes(ty, N, m, n, shared)
        if one_equation:
            want.update({k: eng._sizes(ty, 1, m, n)[k] for k in ("A", "B", "Gamma", "target")})
        return [h[k][: copies * want[k]] for k in keys]

    lab = "%s %dx%d " % (tname, m, n)
    cs.run(lab + "verify_batch N=3", lambda: eng.verify_batch(ty, 3, m, n, *take(VERIFY_KEYS, 3)))
    if (m, n) == (2, 3):
        for twin in range(4):
            cs.run(lab + "verify_batch N=3", lambda: eng.verify_batch(ty, 3, m, n, *take(VERIFY_KEYS, 3)), miller_twin=twin)
    cs.run(lab + "verify_batch_rlc N=3", lambda: eng.verify_batch_rlc(ty, 3, m, n, *take(VERIFY_KEYS, 3), rho[:12]))
    cs.run(lab + "verify_batch_rlc_locate N=9",
           lambda: eng.verify_batch_rlc_locate(ty, 9, m, n, *take(VERIFY_KEYS, 9), rho), locate_k=2)
    for form in (0, 1):
        cs.run(lab + "verify_equation_rlc N=3",
               lambda: eng.verify_equation_rlc(ty, 3, m, n, *take(VERIFY_KEYS, 3, one_equation=True), rho[:12]), eq_pi=form)
    cs.run(lab + "verify_statements_rlc S=2 E=3",
           lambda: eng.verify_statements_rlc(ty, 2, 3, m, n, *take(VERIFY_KEYS, 3, shared=True, copies=2), rho[:24]))
    cs.run(lab + "prove_batch N=3", lambda: eng.prove_batch(ty, 3, m, n, *take(PROVE_KEYS, 3)))
    cs.run(lab + "prove_statement E=3", lambda: eng.prove_statement(ty, 3, m, n, *take(PROVE_KEYS, 3, shared=True)))
    cs.run(lab + "rerandomize_batch N=3", lambda: eng.rerandomize_batch(ty, 3, m, n, *take(RERAND_KEYS, 3)))
    cs.run(lab + "rerandomize_statement E=3",
           lambda: eng.rerandomize_statement(ty, 3, m, n, *take(RERAND_KEYS, 3, shared=True)))
    return h


def main():
    for curve, cname in ((0, "bls12_381"), (1, "bn254")):
        eng = gs.Engine(curve, 0)
        cs = Cases(eng, cname)
        kept = {}
        for ty, tname in TYPES:
            for m, n in ((1, 1), (2, 3)):
                kept[tname] = shape_cases(cs, ty, tname, m, n)
        # commitments of each kind: group elements from the PPE workload, scalars from the QuadEqu one
        ppe, quad = kept["PPE"], kept["QuadEqu"]
        for kind, vars_, count, vsz in (("g1", ppe["X"], 2, eng.G1), ("g2", ppe["Y"], 3, eng.G2),
                                        ("fr_b1", quad["X"], 2, eng.FR), ("fr_b2", quad["Y"], 3, eng.FR)):
            rand = ppe["R"][: count * 2 * eng.FR] if kind in ("g1", "g2") else quad["R"][: count * eng.FR]
            cs.run("commit %s" % kind, lambda: eng.commit(kind, vars_[: count * vsz], rand))
        # m n >= 1024: Gamma is prepared one lane per entry, the verifier's Gamma^T c runs on shared base tables
        for ty, tname in ((gs.GS_PPE, "PPE"), (gs.GS_QUAD, "QuadEqu")):
            wl = Workload(eng, ty=ty, N=1, m=32, n=32, corrupt_every=0)
            wl.prove()
            eng.sync()
            h = host_arrays(wl)
            args = [h[k] for k in VERIFY_KEYS]
            rho = np.arange(1, 5, dtype=np.uint64)
            cs.run("%s 32x32 verify_batch N=1" % tname, lambda: eng.verify_batch(ty, 1, 32, 32, *args))
            cs.run("%s 32x32 verify_batch_rlc N=1" % tname, lambda: eng.verify_batch_rlc(ty, 1, 32, 32, *args, rho))
        # forced shapes on the last small workload (QuadEqu 2 x 3) and on PPE 2 x 3
        rho = np.random.default_rng(7).integers(1, 1 << 63, size=4 * 9, dtype=np.uint64)
        for tname, ty in (("PPE", gs.GS_PPE), ("QuadEqu", gs.GS_QUAD)):
            h, (m, n) = kept[tname], (2, 3)
            lab = "%s %dx%d " % (tname, m, n)
            v3 = [h[k][: eng._sizes(ty, 3, m, n)[k]] for k in VERIFY_KEYS]
            st = [h[k][: 2 * eng._sizes(ty, 3, m, n, True)[k]] for k in VERIFY_KEYS]
            cs.run(lab + "verify_batch_rlc N=3", lambda: eng.verify_batch_rlc(ty, 3, m, n, *v3, rho[:12]), endo=0)
            cs.run(lab + "verify_batch N=3", lambda: eng.verify_batch(ty, 3, m, n, *v3), coop_fe=2)
            cs.run(lab + "verify_statements_rlc S=2 E=3",
                   lambda: eng.verify_statements_rlc(ty, 2, 3, m, n, *st, rho[:24]), coop_fe=2)
        eng.close()


if __name__ == "__main__":
    main()

"""The statement-batched verifier against the two verifiers that existed before it, device-resident, BLS12-381:
PPE 4x4 and QuadEqu 4x4, S statements of E equations with S * E = 2^14, E in {1, 4, 16, 64}.  Three entries on the SAME
proofs:
    stmt_rlc   gs_verify_statements_rlc_dev         S statements, shared commitments, one verdict per statement
    exact      gs_verify_batch_dev                  S * E equations, the statement's commitments replicated E times
    batch_rlc  gs_verify_batch_rlc_dev              the same replicated batch, one verdict for all of it
The timings alternate on ONE device in one run (entry by entry within each repetition); the median of the repetitions
is reported, with the per-kernel times of the new entry from a profiled run of its own.
    python tools/stmt_rlc_rate.py [--log2 14] [--reps 7] [--out profiles/stmt_rlc] [--E 16 64] [--types PPE]
With GS_PLAN_TRACE=1 in the environment the engine prints the lane plan of every Straus pass and Miller launch on stderr
(profiles/stmt_rlc/plan_trace_ppe.txt was made that way)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import CURVES, Workload, _limbs


class Statements:
    """S statements of E satisfied equations each, proven on the device; arrays in the replicated-batch layout
    ([S * E] equations, every equation with its own copy of its statement's commitments) and the shared one."""

    def __init__(self, eng, ty, S, E, m, n, seed):
        dev = "cuda:0"
        self.eng, self.ty, self.S, self.E, self.m, self.n = eng, ty, S, E, m, n
        N = S * E
        wl = Workload(eng, ty=ty, N=1, m=1, n=1, seed=seed, corrupt_every=0)  # the CRS and its generators
        r = CURVES[eng.curve]["r"]
        rng = np.random.default_rng(seed)
        sh = eng.shape(ty)
        kx, ky = sh["kx"], sh["ky"]

        def scalars(count):
            raw = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
            return [(int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192) % r for a, b, c, d in raw]

        def fr(vals):
            a = np.array([_limbs(v * (1 << 256) % r, 4) for v in vals], dtype=np.uint64)
            return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)

        gen = {1: torch.from_numpy(wl.g1_gen.copy()).to(dev), 2: torch.from_numpy(wl.g2_gen.copy()).to(dev)}

        def elems(vals, group, isg):
            k = fr(vals)
            if not isg:
                return k
            out = torch.empty(len(vals) * (eng.G1 if group == 1 else eng.G2), dtype=torch.uint8, device=dev)
            eng.g_mul_batch_dev(group, len(vals), gen[group], True, k, out)
            return out

        rep = lambda vals, per: [v for s in range(S) for _ in range(E) for v in vals[s * per:(s + 1) * per]]
        xs, ys = scalars(S * m), scalars(S * n)                       # one list of variables per statement
        rr, ss = scalars(S * m * kx), scalars(S * n * ky)             # and one commit randomness
        a, b, gam = scalars(N * n), scalars(N * m), scalars(N * m * n)
        tg = []
        for e in range(N):
            s = e // E
            t = sum(a[e * n + j] * ys[s * n + j] for j in range(n)) + sum(xs[s * m + i] * b[e * m + i] for i in range(m))
            t += sum(xs[s * m + i] * gam[(e * m + i) * n + j] % r * ys[s * n + j] for i in range(m) for j in range(n))
            tg.append(t % r)
        X, Y = elems(rep(xs, m), 1, sh["xg"]), elems(rep(ys, n), 2, sh["yg"])
        self.A, self.B, self.Gamma = elems(a, 1, sh["xg"]), elems(b, 2, sh["yg"]), fr(gam)
        kt = fr(tg)
        if ty == gs.GS_PPE:
            self.target = torch.empty(N * eng.GT, dtype=torch.uint8, device=dev)
            eng.gt_pow_batch_dev(N, torch.from_numpy(wl.gt_gen.copy()).to(dev), kt, self.target)
        else:
            self.target = kt
        R, Sr, T = fr(rep(rr, m * kx)), fr(rep(ss, n * ky)), fr(scalars(N * ky * kx))
        empty = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.xcoms, self.ycoms = empty(N * m * eng.COM1), empty(N * n * eng.COM2)
        self.pi, self.theta = empty(N * kx * eng.COM2), empty(N * ky * eng.COM1)
        eng.prove_batch_dev(ty, N, m, n, X, Y, self.A, self.B, self.Gamma, R, Sr, T, self.xcoms, self.ycoms, self.pi, self.theta)
        eng.sync()
        # the same randomness gives the same commitment: equation 0 of a statement holds the statement's
        self.xshared = self.xcoms.view(S, E, -1)[:, 0].contiguous().view(-1)
        self.yshared = self.ycoms.view(S, E, -1)[:, 0].contiguous().view(-1)
        assert bool((self.xcoms.view(S, E, -1) == self.xshared.view(S, 1, -1)).all())
        raw = np.frombuffer(os.urandom(N * 32), dtype=np.uint64).copy()
        raw[raw == 0] = 1
        self.rho = torch.from_numpy(raw.view(np.int64)).to(dev)
        self.ok_s, self.ok_n = empty(S), empty(N)
        self.acc_s, self.acc_1 = empty(S * 2 * eng.GT), empty(2 * eng.GT)

    def stmt_rlc(self):
        self.eng.verify_statements_rlc_dev(self.ty, self.S, self.E, self.m, self.n, self.A, self.B, self.Gamma, self.target,
                                           self.xshared, self.yshared, self.pi, self.theta, self.rho, self.acc_s, self.ok_s)

    def exact(self):
        self.eng.verify_batch_dev(self.ty, self.S * self.E, self.m, self.n, self.A, self.B, self.Gamma, self.target,
                                  self.xcoms, self.ycoms, self.pi, self.theta, self.ok_n)

    def batch_rlc(self):
        self.eng.verify_batch_rlc_dev(self.ty, self.S * self.E, self.m, self.n, self.A, self.B, self.Gamma, self.target,
                                      self.xcoms, self.ycoms, self.pi, self.theta, self.rho, self.acc_1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=14)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "stmt_rlc"))
    ap.add_argument("--E", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--types", nargs="*", default=["PPE", "QuadEqu"], help="which of PPE, QuadEqu to run")
    args = ap.parse_args()
    assert args.reps >= 5
    eng = gs.Engine(0, 0)
    rows = []
    for ty, name in ((gs.GS_PPE, "PPE"), (gs.GS_QUAD, "QuadEqu")):
        if name not in args.types:
            continue
        for E in args.E:
            S = (1 << args.log2) // E
            st = Statements(eng, ty, S, E, 4, 4, 20241230 + E)
            entries = [("stmt_rlc", st.stmt_rlc), ("exact", st.exact), ("batch_rlc", st.batch_rlc)]
            for _, fn in entries:  # warm-up: plans, scratch, tables
                fn()
            eng.sync()
            assert bool(st.ok_s.all()) and bool(st.ok_n.all()) and eng.gt_finalize_dev(st.acc_1, 1) == 1
            ms = {k: [] for k, _ in entries}
            for _ in range(args.reps):
                for k, fn in entries:  # alternate: every repetition times the three entries one after the other
                    eng.sync()
                    t0 = time.perf_counter()
                    fn()
                    eng.sync()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in ms.items()}
            eng.prof_enable(True)
            eng.prof_reset()
            st.stmt_rlc()
            eng.sync()
            kernels = {nm: round(t, 4) for nm, t, _ in eng.prof_get()}
            eng.prof_enable(False)
            row = dict(type=name, m=4, n=4, S=S, E=E, reps=args.reps, median_ms={k: round(v, 4) for k, v in med.items()},
                       min_ms={k: round(min(v), 4) for k, v in ms.items()}, max_ms={k: round(max(v), 4) for k, v in ms.items()},
                       equations_per_s={k: round(S * E / v * 1e3) for k, v in med.items()},
                       speedup_over_exact=round(med["exact"] / med["stmt_rlc"], 3),
                       speedup_over_batch_rlc=round(med["batch_rlc"] / med["stmt_rlc"], 3), stmt_rlc_kernels_ms=kernels)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del st
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rate_2p%d.json" % args.log2), "w") as f:
        json.dump(dict(curve="bls12_381", device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

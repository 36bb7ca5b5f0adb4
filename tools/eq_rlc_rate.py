"""The batched verifier for N proofs of ONE equation against the two verifiers that existed before it, device-resident,
BLS12-381, 4 x 4, PPE and QuadEqu, N = 2^12, 2^14, 2^16.  The proofs are one proven equation rerandomized N times
(gs_rerandomize_batch_dev): what a verifier of re-shown credentials receives.  Entries on the SAME proofs:
    eq_rlc      gs_verify_equation_rlc_dev   constants once, "eq_pi" planned
    eq_rlc_pi0  the same, "eq_pi" = 0        pi paired per proof
    eq_rlc_pi1  the same, "eq_pi" = 1        pi folded in G2 across the batch
    batch_rlc   gs_verify_batch_rlc_dev      the YARDSTICK: the constants replicated N times
    exact       gs_verify_batch_dev          the same replicated batch, one verdict per proof (for context)
The timings alternate on ONE device in one run (entry by entry within each repetition, in an order that changes from
repetition to repetition so that no entry always follows the same one); the median of the repetitions is reported, with
the per-kernel times of both forms of the new entry from profiled calls of their own.
    python tools/eq_rlc_rate.py [--log2 12 14 16] [--reps 7] [--out profiles/eq_rlc] [--types PPE QuadEqu]"""
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


class Showings:
    """N rerandomizations of one proven equation; the constants once (eq_*) and replicated N times (rep_*)"""

    def __init__(self, eng, ty, N, m, n, seed):
        dev = "cuda:0"
        self.eng, self.ty, self.N, self.m, self.n = eng, ty, N, m, n
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

        def fresh(count):  # uniform below 2^252 < r: Montgomery-form randomness for the rerandomization
            raw = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
            raw[:, 3] &= np.uint64((1 << 60) - 1)
            return torch.from_numpy(raw.view(np.uint8).reshape(-1)).to(dev)

        gen = {1: torch.from_numpy(wl.g1_gen.copy()).to(dev), 2: torch.from_numpy(wl.g2_gen.copy()).to(dev)}

        def elems(vals, group, isg):
            k = fr(vals)
            if not isg:
                return k
            out = torch.empty(len(vals) * (eng.G1 if group == 1 else eng.G2), dtype=torch.uint8, device=dev)
            eng.g_mul_batch_dev(group, len(vals), gen[group], True, k, out)
            return out

        xs, ys, a, b, gam = scalars(m), scalars(n), scalars(n), scalars(m), scalars(m * n)
        t = sum(a[j] * ys[j] for j in range(n)) + sum(xs[i] * b[i] for i in range(m))
        t = (t + sum(xs[i] * gam[i * n + j] % r * ys[j] for i in range(m) for j in range(n))) % r
        X, Y = elems(xs, 1, sh["xg"]), elems(ys, 2, sh["yg"])
        self.A, self.B, self.Gamma = elems(a, 1, sh["xg"]), elems(b, 2, sh["yg"]), fr(gam)
        if ty == gs.GS_PPE:
            self.target = torch.empty(eng.GT, dtype=torch.uint8, device=dev)
            eng.gt_pow_batch_dev(1, torch.from_numpy(wl.gt_gen.copy()).to(dev), fr([t]), self.target)
        else:
            self.target = fr([t])
        empty = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
        one = [empty(m * eng.COM1), empty(n * eng.COM2), empty(kx * eng.COM2), empty(ky * eng.COM1)]
        eng.prove_batch_dev(ty, 1, m, n, X, Y, self.A, self.B, self.Gamma, fr(scalars(m * kx)), fr(scalars(n * ky)),
                            fr(scalars(ky * kx)), *one)
        eng.sync()
        rep = lambda tt: tt.repeat(N)
        self.rep_A, self.rep_B, self.rep_Gamma, self.rep_target = rep(self.A), rep(self.B), rep(self.Gamma), rep(self.target)
        self.xcoms, self.ycoms = empty(N * m * eng.COM1), empty(N * n * eng.COM2)
        self.pi, self.theta = empty(N * kx * eng.COM2), empty(N * ky * eng.COM1)
        eng.rerandomize_batch_dev(ty, N, m, n, self.rep_A, self.rep_B, self.rep_Gamma, *[rep(o) for o in one],
                                  fresh(N * m * kx), fresh(N * n * ky), fresh(N * ky * kx), self.xcoms, self.ycoms, self.pi,
                                  self.theta)
        eng.sync()
        raw = np.frombuffer(os.urandom(N * 32), dtype=np.uint64).copy()
        raw[raw == 0] = 1
        self.rho = torch.from_numpy(raw.view(np.int64)).to(dev)
        self.ok_n = empty(N)
        self.acc_e, self.acc_1 = empty(2 * eng.GT), empty(2 * eng.GT)

    def eq_rlc(self, pi_form=-1):
        self.eng.set_option("eq_pi", pi_form)
        self.eng.verify_equation_rlc_dev(self.ty, self.N, self.m, self.n, self.A, self.B, self.Gamma, self.target,
                                         self.xcoms, self.ycoms, self.pi, self.theta, self.rho, self.acc_e)

    def exact(self):
        self.eng.verify_batch_dev(self.ty, self.N, self.m, self.n, self.rep_A, self.rep_B, self.rep_Gamma, self.rep_target,
                                  self.xcoms, self.ycoms, self.pi, self.theta, self.ok_n)

    def batch_rlc(self):
        self.eng.verify_batch_rlc_dev(self.ty, self.N, self.m, self.n, self.rep_A, self.rep_B, self.rep_Gamma,
                                      self.rep_target, self.xcoms, self.ycoms, self.pi, self.theta, self.rho, self.acc_1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "eq_rlc"))
    ap.add_argument("--types", nargs="*", default=["PPE", "QuadEqu"], help="which of PPE, QuadEqu to run")
    args = ap.parse_args()
    assert args.reps >= 5
    eng = gs.Engine(0, 0)
    rows = []
    for ty, name in ((gs.GS_PPE, "PPE"), (gs.GS_QUAD, "QuadEqu")):
        if name not in args.types:
            continue
        for lg in args.log2:
            N = 1 << lg
            sw = Showings(eng, ty, N, 4, 4, 20260101 + lg)
            entries = [("eq_rlc", lambda: sw.eq_rlc(-1)), ("eq_rlc_pi0", lambda: sw.eq_rlc(0)),
                       ("eq_rlc_pi1", lambda: sw.eq_rlc(1)), ("batch_rlc", sw.batch_rlc), ("exact", sw.exact)]
            for k, fn in entries:  # warm-up: plans, scratch, tables -- and every entry accepts the batch
                fn()
                eng.sync()
                if k.startswith("eq_rlc"):
                    assert eng.gt_finalize_dev(sw.acc_e, 1) == 1, k
            assert bool(sw.ok_n.all()) and eng.gt_finalize_dev(sw.acc_1, 1) == 1
            assert bool((sw.acc_e[eng.GT:] == sw.acc_1[eng.GT:]).all())  # the same target side, byte for byte
            ms = {k: [] for k, _ in entries}
            for rep in range(args.reps):
                # alternate: every repetition times the five entries one after the other, in an order that changes from
                # repetition to repetition (stride 1, 2, 3, 4 through the list), so that every entry follows each of the
                # others in turn: a call reads 3-8 % faster right after `exact` than after another combined check
                step, L = 1 + rep % (len(entries) - 1), len(entries)
                assert L == 5  # (a prime: every stride visits every entry)
                for k, fn in [entries[(rep + i * step) % L] for i in range(L)]:
                    eng.sync()
                    t0 = time.perf_counter()
                    fn()
                    eng.sync()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in ms.items()}
            kernels = {}
            for form in (0, 1):
                eng.prof_enable(True)
                eng.prof_reset()
                sw.eq_rlc(form)
                eng.sync()
                kernels["eq_pi_%d" % form] = {nm: round(t, 4) for nm, t, _ in eng.prof_get()}
                eng.prof_enable(False)
            eng.set_option("eq_pi", -1)
            row = dict(type=name, m=4, n=4, N=N, reps=args.reps, median_ms={k: round(v, 4) for k, v in med.items()},
                       min_ms={k: round(min(v), 4) for k, v in ms.items()}, max_ms={k: round(max(v), 4) for k, v in ms.items()},
                       proofs_per_s={k: round(N / v * 1e3) for k, v in med.items()},
                       ratio_batch_rlc_over_eq_rlc=round(med["batch_rlc"] / med["eq_rlc"], 4),
                       ratio_batch_rlc_over_pi0=round(med["batch_rlc"] / med["eq_rlc_pi0"], 4),
                       ratio_batch_rlc_over_pi1=round(med["batch_rlc"] / med["eq_rlc_pi1"], 4),
                       ratio_exact_over_eq_rlc=round(med["exact"] / med["eq_rlc"], 4), eq_rlc_kernels_ms=kernels)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del sw
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rate.json"), "w") as f:
        json.dump(dict(curve="bls12_381", device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

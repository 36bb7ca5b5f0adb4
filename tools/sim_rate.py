"""What simulating a proof costs next to making it honestly: gs_simulate_batch_dev against gs_prove_batch_dev (commitments
included: the YARDSTICK of the derived condition of DESIGN.md 6.9 -- the simulator does no more group work than the prover
on the same shape, so a simulate call should not take longer), device-resident, 4 x 4, BLS12-381, under ONE hiding CRS:
MSMEG1 and QuadEqu at N = 2^12 and 2^16, MSMEG2 at 2^16.
The two entries alternate within every repetition, in one process on one device (the order flips from repetition to
repetition); after a warm-up the median of the repetitions is reported with the yardstick's own spread, and the
per-kernel times of each entry from a profiled call of its own.  The batch's constants and targets are the workload's;
the simulator is given uniform coordinates Rc, Sc, Tf and never sees a witness.  Both outputs are verified once.
    python tools/sim_rate.py [--reps 7] [--out profiles/simulate]"""
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
from groth_sahai_rs_amd.workload import SplitMix64, Workload, _limbs


def install_hiding_crs(eng, wl, seed):
    """The hiding CRS over the workload's generators and scalars (Workload draws al, be, a1, a2, t1, t2 from
    SplitMix64(seed) and installs the binding form), and its trapdoor."""
    sm, r = SplitMix64(seed), wl.r
    sc = [(sm.next() | (sm.next() << 64) | (sm.next() << 128)) % r for _ in range(6)][2:]
    mont = np.array([_limbs(v * (1 << 256) % r, 4) for v in sc], dtype=np.uint64)
    hid = eng.crs_generate(wl.g1_gen, wl.g2_gen, mont, hiding=True)
    binding = np.ascontiguousarray(wl.crs).view(np.uint8).reshape(-1)
    assert (hid[:2 * eng.G1] == binding[:2 * eng.G1]).all(), "u0 differs: the scalars are not the workload's"
    eng.set_crs(hid)
    eng.set_simulation_key(mont[2:4])


def profile(eng, fn):
    eng.prof_enable(True)
    eng.prof_reset()
    fn()
    eng.sync()
    kernels = {nm: round(t, 4) for nm, t, _ in eng.prof_get()}
    eng.prof_enable(False)
    return kernels


def measure(eng, ty, name, N, reps, seed):
    m = n = 4
    wl = Workload(eng, ty=ty, N=N, m=m, n=n, seed=seed, corrupt_every=0)
    install_hiding_crs(eng, wl, seed)
    out = {k: torch.zeros_like(getattr(wl, k)) for k in ("xcoms", "ycoms", "pi", "theta")}
    # the workload's R, S, T are uniform scalars of the right shapes: the simulator's Rc, Sc, Tf
    simulate = lambda: eng.simulate_batch_dev(ty, N, m, n, wl.A, wl.B, wl.Gamma, wl.target, wl.R, wl.S, wl.T,
                                              out["xcoms"], out["ycoms"], out["pi"], out["theta"])
    entries = [("simulate", simulate), ("prove", wl.prove)]
    for _, fn in entries:  # warm-up: plans, scratch, tables
        fn()
        eng.sync()
    wl.verify()  # the honest proofs, under the hiding CRS
    eng.sync()
    assert bool(wl.ok.all()), "honest proofs rejected"
    ok = torch.zeros(N, dtype=torch.uint8, device=wl.ok.device)
    eng.verify_batch_dev(ty, N, m, n, wl.A, wl.B, wl.Gamma, wl.target, out["xcoms"], out["ycoms"], out["pi"],
                         out["theta"], ok)
    eng.sync()
    assert bool(ok.all()), "simulated proofs rejected"
    ms = {k: [] for k, _ in entries}
    for rep in range(reps):
        for k, fn in (entries if rep % 2 == 0 else entries[::-1]):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratio = med["simulate"] / med["prove"]
    # the margin: the spread of the yardstick's own samples in this run, relative to its median
    margin = (max(ms["prove"]) - min(ms["prove"])) / med["prove"]
    return dict(curve="bls12_381", type=name, m=m, n=n, N=N, reps=reps,
                median_ms={k: round(v, 4) for k, v in med.items()},
                min_ms={k: round(min(v), 4) for k, v in ms.items()}, max_ms={k: round(max(v), 4) for k, v in ms.items()},
                equations_per_s={k: round(N / v * 1e3) for k, v in med.items()},
                ratio_simulate_over_prove=round(ratio, 4), yardstick_spread=round(margin, 4),
                simulate_not_slower=bool(ratio <= 1.0 + margin),
                simulate_kernels_ms=profile(eng, simulate), prove_kernels_ms=profile(eng, wl.prove))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "simulate"))
    args = ap.parse_args()
    assert args.reps >= 5
    plan = [(gs.GS_MSMEG1, "MSMEG1", 12), (gs.GS_MSMEG1, "MSMEG1", 16), (gs.GS_QUAD, "QuadEqu", 12),
            (gs.GS_QUAD, "QuadEqu", 16), (gs.GS_MSMEG2, "MSMEG2", 16)]
    eng = gs.Engine(0, 0)
    rows = []
    for ty, name, lg in plan:
        row = measure(eng, ty, name, 1 << lg, args.reps, 20260301 + lg)
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rate.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
    missed = [(r["type"], r["N"], r["ratio_simulate_over_prove"]) for r in rows if not r["simulate_not_slower"]]
    if missed:
        print("MISSED: simulate slower than gs_prove_batch_dev beyond the yardstick's spread at %s" % missed, flush=True)


if __name__ == "__main__":
    main()

"""What drawing the prover's randomness on the device costs: the drawn entries against the entries that are handed
ready-made R, S, T, on one box, BLS12-381, PPE 4 x 4, N = 2^12 and 2^16, median of --reps repetitions after a warm-up,
the entries alternating within every repetition (the order flips from repetition to repetition).
  1. the generator alone: k_rand_fr for the 20 N scalars of a prove (gs_rand_fr_dev, one call), k_rand_rho for the 4 N
     exponents of a batched check (gs_rand_rho_dev);
  2. host pointers: gs_prove_batch_drawn with R_out = S_out = T_out = NULL, and with all three returned, against
     gs_prove_batch given ready-made arrays (the YARDSTICK: that entry is unchanged);
  3. device pointers: the same pair of _dev entries.
The expectation to check: the drawn host form with NULL outputs is not slower than gs_prove_batch, because it stages
20 N scalars less.  The margin is the spread (min to max) of this run's own repetitions of the yardstick.  What a host
thread pays to draw the 20 N scalars is NOT measured here.
    python tools/rand_rate.py [--reps 7] [--out profiles/rand]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import Workload


def timed(eng, entries, reps):
    for _, fn in entries:  # warm-up: plans, scratch, staging buffers
        fn()
        eng.sync()
    ms = {k: [] for k, _ in entries}
    for rep in range(reps):
        for k, fn in (entries if rep % 2 == 0 else entries[::-1]):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return dict(median_ms={k: round(statistics.median(v), 4) for k, v in ms.items()},
                min_ms={k: round(min(v), 4) for k, v in ms.items()}, max_ms={k: round(max(v), 4) for k, v in ms.items()})


def measure(eng, N, reps, seed):
    ty, m, n = gs.GS_PPE, 4, 4
    wl = Workload(eng, ty=ty, N=N, m=m, n=n, seed=seed, corrupt_every=0)
    eng.rand_set_key(os.urandom(32))
    dev = wl.xcoms.device
    e = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
    row = dict(curve="bls12_381", type="PPE", m=m, n=n, N=N, reps=reps)
    # 1. the generator alone
    nfr, nrho = 20 * N, 4 * N
    fr_out, rho_out = e(nfr * 32), e(nrho * 8)
    ms = timed(eng, [("rand_fr", lambda: eng.rand_fr_dev(gs.capi.GS_RAND_USER, 1, 0, nfr, fr_out)),
                     ("rand_rho", lambda: eng.rand_rho_dev(1, 0, nrho, rho_out))], reps)
    row["generator"] = dict(scalars=nfr, exponents=nrho, **stats(ms))
    row["generator"]["scalars_per_s"] = round(nfr / statistics.median(ms["rand_fr"]) * 1e3)
    row["generator"]["exponents_per_s"] = round(nrho / statistics.median(ms["rand_rho"]) * 1e3)
    # 3. device pointers
    ins = (wl.X, wl.Y, wl.A, wl.B, wl.Gamma)
    outs = (wl.xcoms, wl.ycoms, wl.pi, wl.theta)
    rst = [torch.empty_like(t) for t in (wl.R, wl.S, wl.T)]
    stream = [0]

    def next_stream():
        stream[0] += 1
        return stream[0]

    ms = timed(eng, [("prove_batch_dev", wl.prove),
                     ("drawn_dev_null", lambda: eng.prove_batch_drawn_dev(ty, N, m, n, *ins, next_stream(), None, None,
                                                                          None, *outs)),
                     ("drawn_dev_returned", lambda: eng.prove_batch_drawn_dev(ty, N, m, n, *ins, next_stream(), *rst,
                                                                              *outs))], reps)
    wl.verify()
    eng.sync()
    assert bool(wl.ok.all()), "drawn proofs rejected"
    row["dev"] = stats(ms)
    y = ms["prove_batch_dev"]
    row["dev"]["yardstick_spread"] = round((max(y) - min(y)) / statistics.median(y), 4)
    for k in ("drawn_dev_null", "drawn_dev_returned"):
        row["dev"]["ratio_" + k] = round(statistics.median(ms[k]) / statistics.median(y), 4)
    # 2. host pointers (pageable numpy arrays, as a caller's slices are)
    hin = [t.cpu().numpy() for t in ins]
    hR, hS, hT = (t.cpu().numpy() for t in (wl.R, wl.S, wl.T))
    out = {k: t.cpu().numpy().copy() for k, t in zip(("xcoms", "ycoms", "pi", "theta"), outs)}
    # (every entry writes into the same preallocated arrays: allocating 226 MB of outputs per call at 2^16 is not what
    # is being compared)
    out_rst = dict(out, R=hR.copy(), S=hS.copy(), T=hT.copy())
    ms = timed(eng, [("prove_batch", lambda: eng.prove_batch(ty, N, m, n, *hin, hR, hS, hT, out=out)),
                     ("drawn_null", lambda: eng.prove_batch_drawn(ty, N, m, n, *hin, next_stream(), out=out)),
                     ("drawn_returned", lambda: eng.prove_batch_drawn(ty, N, m, n, *hin, next_stream(), out=out_rst))],
               reps)
    ok = eng.verify_batch(ty, N, m, n, *hin[2:], wl.target.cpu().numpy(), *(out[k] for k in ("xcoms", "ycoms", "pi", "theta")))
    assert bool(ok.all()), "drawn proofs (host form) rejected"
    row["host"] = stats(ms)
    y = ms["prove_batch"]
    margin = (max(y) - min(y)) / statistics.median(y)
    row["host"]["yardstick_spread"] = round(margin, 4)
    for k in ("drawn_null", "drawn_returned"):
        row["host"]["ratio_" + k] = round(statistics.median(ms[k]) / statistics.median(y), 4)
    row["host"]["scalar_bytes_not_staged"] = 20 * N * 32
    row["host"]["drawn_null_not_slower"] = bool(row["host"]["ratio_drawn_null"] <= 1.0 + margin)
    eng.rand_set_key(None)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "rand"))
    ap.add_argument("--log2", type=int, nargs="*", default=[12, 16])
    args = ap.parse_args()
    assert args.reps >= 5
    eng = gs.Engine(0, 0)
    rows = []
    os.makedirs(args.out, exist_ok=True)
    for lg in args.log2:
        row = measure(eng, 1 << lg, args.reps, 20261021 + lg)
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(os.path.join(args.out, "rate.json"), "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
            f.write("\n")
    eng.close()
    missed = [(r["N"], r["host"]["ratio_drawn_null"]) for r in rows if not r["host"]["drawn_null_not_slower"]]
    if missed:
        print("MISSED: gs_prove_batch_drawn (NULL outputs) slower than gs_prove_batch beyond the yardstick's spread at %s"
              % missed, flush=True)


if __name__ == "__main__":
    main()

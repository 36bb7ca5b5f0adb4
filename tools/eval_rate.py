"""What evaluating an equation costs next to proving and verifying it: gs_eval_batch_dev and gs_check_witness_batch_dev
against the entries a caller had before them, device-resident, 4 x 4, N = 2^12, 2^14, 2^16: BLS12-381 PPE and MSMEG1, and
BN254 PPE at 2^16.  Entries on the SAME batch in the same run:
    eval          gs_eval_batch_dev            the targets from the witness
    check         gs_check_witness_batch_dev   one byte per equation: does the witness satisfy it
    prove         gs_prove_batch_dev           commit_and_prove of the batch
    verify        gs_verify_batch_dev          the exact verifier on those proofs (the YARDSTICK of the derived condition:
                                               PPE evaluation is 8 stepped pairs, one final exponentiation and an n-output
                                               Gamma sum per equation; verify is 40 pairs, 4 final exponentiations and a
                                               2n-output Gamma sum -- evaluation must take less time at every N)
    multi_pairing gs_multi_pairing_batch_dev   k = m + n ARBITRARY pairs per row (PPE only): the one pairing tool a caller
                                               had, and it does none of the Gamma work
The timings alternate on ONE device in one run (entry by entry within each repetition, in an order that changes from
repetition to repetition so that no entry always follows the same one); the median of the repetitions is reported, with
the per-kernel times of the evaluation from a profiled call of its own.
    python tools/eval_rate.py [--log2 12 14 16] [--reps 7] [--out profiles/eval]"""
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


def measure(eng, cname, ty, name, N, reps, seed):
    m = n = 4
    wl = Workload(eng, ty=ty, N=N, m=m, n=n, seed=seed, corrupt_every=0)
    dev = wl.target.device
    mine = torch.zeros_like(wl.target)
    ok = torch.zeros(N, dtype=torch.uint8, device=dev)
    ins = (wl.X, wl.Y, wl.A, wl.B, wl.Gamma)
    entries = [("eval", lambda: eng.eval_batch_dev(ty, N, m, n, *ins, mine)),
               ("check", lambda: eng.check_witness_batch_dev(ty, N, m, n, *ins, wl.target, ok)),
               ("prove", wl.prove), ("verify", wl.verify)]
    if ty == gs.GS_PPE:
        # arbitrary pairs: the batch's own X and A as the G1 arguments, B and Y as the G2 arguments (k = m + n per row)
        P = torch.cat([wl.X.view(N, -1), wl.A.view(N, -1)], dim=1).contiguous().view(-1)
        Q = torch.cat([wl.B.view(N, -1), wl.Y.view(N, -1)], dim=1).contiguous().view(-1)
        gt = torch.zeros(N * eng.GT, dtype=torch.uint8, device=dev)
        entries.append(("multi_pairing", lambda: eng.multi_pairing_batch_dev(N, m + n, P, Q, gt)))
    for _, fn in entries:  # warm-up: plans, scratch, tables -- and every entry is right about the batch
        fn()
        eng.sync()
    assert bool((mine == wl.target).all()), "evaluation differs from the discrete-log targets"
    assert bool(ok.all()) and bool(wl.ok.all())
    ms = {k: [] for k, _ in entries}
    L = len(entries)
    for rep in range(reps):
        # every repetition times the entries one after the other, rotated and (odd repetitions) reversed, so that no
        # entry always follows the same one
        order = [entries[(rep + i) % L] for i in range(L)]
        if rep % 2:
            order.reverse()
        for k, fn in order:
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    eng.prof_enable(True)
    eng.prof_reset()
    entries[0][1]()
    eng.sync()
    kernels = {nm: round(t, 4) for nm, t, _ in eng.prof_get()}
    eng.prof_enable(False)
    row = dict(curve=cname, type=name, m=m, n=n, N=N, reps=reps, median_ms={k: round(v, 4) for k, v in med.items()},
               min_ms={k: round(min(v), 4) for k, v in ms.items()}, max_ms={k: round(max(v), 4) for k, v in ms.items()},
               equations_per_s={k: round(N / v * 1e3) for k, v in med.items()},
               ratio_verify_over_eval=round(med["verify"] / med["eval"], 4),
               ratio_prove_plus_verify_over_check=round((med["prove"] + med["verify"]) / med["check"], 4),
               eval_below_verify=bool(med["eval"] < med["verify"]), eval_kernels_ms=kernels)
    if "multi_pairing" in med:
        row["ratio_multi_pairing_over_eval"] = round(med["multi_pairing"] / med["eval"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "eval"))
    args = ap.parse_args()
    assert args.reps >= 5
    plan = [(0, "bls12_381", gs.GS_PPE, "PPE", lg) for lg in args.log2]
    plan += [(0, "bls12_381", gs.GS_MSMEG1, "MSMEG1", lg) for lg in args.log2]
    plan += [(1, "bn254", gs.GS_PPE, "PPE", max(args.log2))]
    rows, eng, cur = [], None, None
    for cid, cname, ty, name, lg in plan:
        if cur != cid:
            if eng:
                eng.close()
            eng, cur = gs.Engine(cid, 0), cid
        row = measure(eng, cname, ty, name, 1 << lg, args.reps, 20260201 + lg)
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rate.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
    # the derived condition: PPE evaluation below the exact verifier at every measured N
    bad = [(r["curve"], r["N"]) for r in rows if r["type"] == "PPE" and not r["eval_below_verify"]]
    if bad:
        sys.exit("PPE evaluation is not faster than gs_verify_batch_dev at %s: the plan is wrong" % bad)


if __name__ == "__main__":
    main()

"""Fault localisation of the batched verifier against the verifiers that existed before it, device-resident, BLS12-381,
2^16 PPE 4 x 4, with b corrupted proofs (a proof's pi replaced by its neighbour's: well-formed, wrong) placed once
spread evenly over the batch and once in one contiguous run:
    locate      gs_verify_batch_rlc_locate_dev      combined check + descent of the kept product tree
    rlc         gs_verify_batch_rlc_dev             this build's combined check alone
    exact       gs_verify_batch_dev                 40 pairs and 4 final exponentiations per equation
    parent_rlc  gs_verify_batch_rlc_dev of ANOTHER build of the library (--parent: tools/build_variant.sh from the parent
                commit), in a child process of its own on the same device, once before and once after everything else:
                its samples are the yardstick for "b = 0 costs what the combined check cost before" and their spread
Every figure is the median of --reps (>= 5) timed calls after a warm-up call, all in ONE run on ONE device.  Per b also
info[1] (node checks of the descent) and the per-kernel times of the new kernels from a profiled call of its own.
    python tools/locate_rate.py [--log2 16] [--reps 7] [--parent groth_sahai_rs_amd/lib/var/parent.so] [--out profiles/locate]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import Workload


def timed(eng, fn, reps):
    fn()  # warm-up: plans, scratch, tables
    eng.sync()
    ms = []
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                samples_ms=[round(v, 4) for v in ms])


def fresh_rho(N):
    raw = np.frombuffer(os.urandom(N * 32), dtype=np.uint64).copy()
    raw[raw == 0] = 1
    return torch.from_numpy(raw.view(np.int64)).to("cuda:0")


def workload(eng, log2):
    wl = Workload(eng, ty=gs.GS_PPE, N=1 << log2, m=4, n=4, seed=20241220, corrupt_every=0)
    wl.prove()
    eng.sync()
    return wl


def rlc_only(args):
    """child mode: the combined check of whichever library GS_AMD_LIB names, one JSON line"""
    eng = gs.Engine(0, 0)
    wl = workload(eng, args.log2)
    rho = fresh_rho(wl.N)
    acc = torch.empty(2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    ms = timed(eng, lambda: eng.verify_batch_rlc_dev(wl.ty, wl.N, 4, 4, wl.A, wl.B, wl.Gamma, wl.target, wl.xcoms, wl.ycoms,
                                                     wl.pi, wl.theta, rho, acc), args.reps)
    assert eng.gt_finalize_dev(acc, 1) == 1
    eng.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps(dict(lib=os.path.relpath(gs.lib_path(), root), **stats(ms))), flush=True)


def parent_run(args):
    if not args.parent:
        return None
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rlc-only", "--log2", str(args.log2), "--reps",
                        str(args.reps)], env=dict(os.environ, GS_AMD_LIB=os.path.abspath(args.parent)),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--b", type=int, nargs="*", default=[0, 1, 16, 256, 4096, 16384, 65536])
    ap.add_argument("--parent", default="", help="another build of the library whose gs_verify_batch_rlc_dev is the yardstick")
    ap.add_argument("--out", default=os.path.join("profiles", "locate"))
    ap.add_argument("--rlc-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.reps >= 5
    if args.rlc_only:
        return rlc_only(args)
    parent = [parent_run(args)]
    eng = gs.Engine(0, 0)
    wl = workload(eng, args.log2)
    N = wl.N
    stride = 2 * eng.COM2
    clean = wl.pi.clone()
    acc = torch.empty(2 * eng.GT, dtype=torch.uint8, device="cuda:0")
    ok = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    info = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    a = (wl.A, wl.B, wl.Gamma, wl.target, wl.xcoms, wl.ycoms, wl.pi, wl.theta)

    def plant(idx):
        wl.pi.copy_(clean)
        if len(idx):
            i = torch.tensor(idx, dtype=torch.int64, device="cuda:0")
            wl.pi.view(N, stride)[i] = clean.view(N, stride)[(i + 1) % N]
        torch.cuda.synchronize()

    rows = []
    for b in args.b:
        b = min(b, N)
        places = [("spread", [i * N // b for i in range(b)])] if b else [("none", [])]
        if 1 < b < N:
            places.append(("run", list(range(N // 3, N // 3 + b))))
        for place, idx in places:
            plant(idx)
            rho = fresh_rho(N)
            locate = lambda: eng.verify_batch_rlc_locate_dev(wl.ty, N, 4, 4, *a, rho, acc, ok, info)
            rlc = lambda: eng.verify_batch_rlc_dev(wl.ty, N, 4, 4, *a, rho, acc)
            exact = lambda: eng.verify_batch_dev(wl.ty, N, 4, 4, *a, ok)
            row = dict(b=b, placement=place)
            # alternate the three entries repetition by repetition
            for fn in (locate, rlc, exact):
                fn()
            eng.sync()
            ms = dict(locate=[], rlc=[], exact=[])
            for _ in range(args.reps):
                for k, fn in (("locate", locate), ("rlc", rlc), ("exact", exact)):
                    eng.sync()
                    t0 = time.perf_counter()
                    fn()
                    eng.sync()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            for k in ms:
                row[k] = stats(ms[k])
            assert sorted(torch.nonzero(ok == 0).view(-1).tolist()) == sorted(idx), "the exact verifier's verdicts"
            eng.prof_enable(True)
            eng.prof_reset()
            locate()
            eng.sync()
            prof = eng.prof_get()
            eng.prof_enable(False)
            assert sorted(torch.nonzero(ok == 0).view(-1).tolist()) == sorted(idx), "the located set"
            h = info.cpu().numpy().view(np.uint32)
            assert int(h[0]) == len(idx)
            row["node_checks"] = int(h[1])
            row["kernels_ms"] = {p[0]: round(p[1], 4) for p in prof if p[0].startswith("k_rlc_") or p[0] == "k_gt_export"}
            row["profiled_total_ms"] = round(sum(p[1] for p in prof), 4)
            row["locate_over_exact"] = round(row["locate"]["median_ms"] / row["exact"]["median_ms"], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    parent.append(parent_run(args))
    parent = [p for p in parent if p]
    out = dict(curve="bls12_381", type="PPE", m=4, n=4, log2=args.log2, reps=args.reps,
               device=torch.cuda.get_device_name(0), rows=rows)
    if parent:
        allms = [v for p in parent for v in p["samples_ms"]]
        out["parent_rlc"] = dict(runs=parent, median_ms=round(statistics.median(allms), 4), min_ms=round(min(allms), 4),
                                 max_ms=round(max(allms), 4))
        print(json.dumps(out["parent_rlc"]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "rate_2p%d.json" % args.log2), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Rerandomization against proving: device-resident time per batch of gs_rerandomize_batch_dev and of
gs_prove_batch_dev (with commitments) on the same batch, PPE 4x4 and QuadEqu 4x4.
    python tools/rerand_rate.py [log2 N ...]        (default: 12 16)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import Workload

eng = gs.Engine(0, 0)
for log2n in [int(a) for a in sys.argv[1:]] or [12, 16]:
    N = 1 << log2n
    for ty, name in ((gs.GS_PPE, "PPE"), (gs.GS_QUAD, "QuadEqu")):
        wl = Workload(eng, ty=ty, N=N, m=4, n=4, seed=20241223, corrupt_every=0)
        wl.prove()
        o = [torch.empty_like(t) for t in (wl.xcoms, wl.ycoms, wl.pi, wl.theta)]
        steps = max(3, min(20, (1 << 17) // N))

        def timed(fn):
            fn()
            fn()
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        # the proof's own randomness serves as R', S', T': the work does not depend on the values
        rer = lambda: eng.rerandomize_batch_dev(ty, N, 4, 4, wl.A, wl.B, wl.Gamma, wl.xcoms, wl.ycoms, wl.pi, wl.theta,
                                                wl.R, wl.S, wl.T, *o)
        t_prove, t_rer = timed(wl.prove), timed(rer)
        print("2^%d %s 4x4: prove (with commitments) %.2f ms (%.0f /s), rerandomize %.2f ms (%.0f /s), ratio %.2f"
              % (log2n, name, t_prove, N / t_prove * 1e3, t_rer, N / t_rer * 1e3, t_rer / t_prove), flush=True)
        del wl, o
eng.close()

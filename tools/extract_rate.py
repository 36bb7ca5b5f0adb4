"""Witness extraction against the generic scalar multiplication it replaces: device-resident time per batch, BLS12-381,
both groups.
  baseline  gs_g*_mul_batch_dev over a de-interleaved copy of c.0 with the key replicated per element -- what a caller
            had to do before gs_extract_*; the de-interleave and the subtraction c.1 - a c.0 are NOT charged to it, so it
            does strictly less work than the fused call
  extract   gs_extract_g*_dev: the multiplication with launch-uniform digits, the subtraction and the normalisation
The two alternate; the figure is the median of the alternations.
    python tools/extract_rate.py [log2 N ...]        (default: 12 16)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import CURVES, SplitMix64

ALTERNATIONS = 7
cv = CURVES[0]
r, p = cv["r"], cv["p"]
limbs = lambda v, n: [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]
fr = lambda vals: np.array([limbs(v * (1 << 256) % r, 4) for v in vals], dtype=np.uint64)
fq = lambda v: np.array(limbs(v * (1 << 384) % p, 6), dtype=np.uint64)

eng = gs.Engine(0, 0)
sm = SplitMix64(20250117)
a1, a2, t1, t2 = [(sm.next() | (sm.next() << 64) | (sm.next() << 128)) % r for _ in range(4)]
p1 = np.concatenate([fq(v) for v in cv["g1"]])
p2 = np.concatenate([fq(v) for v in cv["g2"]])
eng.set_crs(eng.crs_generate(p1, p2, fr([a1, a2, t1, t2])))
eng.set_extraction_key(fr([a1, a2]))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
rng = np.random.default_rng(7)

for log2n in [int(a) for a in sys.argv[1:]] or [12, 16]:
    N = 1 << log2n
    for group, gen, a in ((1, p1, a1), (2, p2, a2)):
        pt = eng.G1 if group == 1 else eng.G2
        # honest commitments of random group elements
        ks = rng.integers(0, 1 << 62, size=(N, 4), dtype=np.uint64)  # < r
        X = dev(eng.g_mul_batch(group, gen, ks, broadcast=True))
        rand = rng.integers(0, 1 << 62, size=(2 * N, 4), dtype=np.uint64)
        coms = dev(eng.commit("g1" if group == 1 else "g2", X.cpu().numpy(), rand))
        c0 = coms.view(N, 2, pt)[:, 0, :].contiguous().view(-1)  # the de-interleave, outside the timing
        key = dev(np.tile(fr([a]), (N, 1)))
        out_b, out_x = torch.empty_like(X), torch.empty_like(X)
        base = lambda: eng.g_mul_batch_dev(group, N, c0, False, key, out_b)
        fused = lambda: eng.extract_dev(group, coms, out_x)
        steps = max(3, min(20, (1 << 17) // N))

        def timed(fn):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        for fn in (base, fused, base, fused):  # warm-up
            fn()
        eng.sync()
        assert (out_x == X).all(), "extraction does not return the committed elements"
        tb, tx = [], []
        for _ in range(ALTERNATIONS):
            tb.append(timed(base))
            tx.append(timed(fused))
        mb, mx = statistics.median(tb), statistics.median(tx)
        print("2^%d G%d: g_mul_batch (key replicated) %.3f ms (%.0f /s) [%.3f .. %.3f], extract %.3f ms (%.0f /s) "
              "[%.3f .. %.3f], extract / baseline %.3f"
              % (log2n, group, mb, N / mb * 1e3, min(tb), max(tb), mx, N / mx * 1e3, min(tx), max(tx), mx / mb),
              flush=True)
eng.close()

"""Bounded discrete logarithms (gs_dlog_g*_dev): device-resident time per batch, BLS12-381, both groups.
  table      gs_dlog_prepare, timed on its own (it synchronises): the baby-step table and the giant-step table
  typical    x uniform in [0, 2^bits): a lane stops at its hit, a wave when its last lane has
  worst      no lane finds anything (x = 2^bits + i): every lane walks all 2^(bits - log2_table - 1) giant steps
Typical and worst alternate on one device; the figure is the median of the alternations.  The rate is giant steps per
second over all lanes, and Fq multiplications per second at the counts of DESIGN.md section 6.4 (6 per G1 step, 16 per
G2 step), for the worst case, where the number of steps is known exactly.
    python tools/dlog_rate.py [--quick] [log2 N ...]        (default: 12 16; --quick: bits 32 / log2_table 20 only)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import groth_sahai_rs_amd as gs
from groth_sahai_rs_amd.workload import CURVES

ALTERNATIONS = 5
MULS_PER_STEP = {1: 6, 2: 16}  # Fq multiplications per giant step
cv = CURVES[0]
r, p = cv["r"], cv["p"]
limbs = lambda v, n: [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]
fr = lambda vals: np.array([limbs(int(v) * (1 << 256) % r, 4) for v in vals], dtype=np.uint64)
fq = lambda v: np.array(limbs(v * (1 << 384) % p, 6), dtype=np.uint64)

args = [a for a in sys.argv[1:] if a != "--quick"]
quick = "--quick" in sys.argv[1:]
configs = [(32, 20)] if quick else [(32, 20), (32, 24), (40, 20), (40, 24)]
eng = gs.Engine(0, 0)
p1 = np.concatenate([fq(v) for v in cv["g1"]])
p2 = np.concatenate([fq(v) for v in cv["g2"]])
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
rng = np.random.default_rng(11)
prepared = {}

for log2n in [int(a) for a in args] or [12, 16]:
    N = 1 << log2n
    for bits, T in configs:
        steps_worst = 1 << (bits - T - 1)
        for group, gen in ((1, p1), (2, p2)):
            if prepared.get(group) != T:
                tt = []
                for _ in range(3):
                    eng.sync()
                    t0 = time.perf_counter()
                    eng.dlog_prepare(group, gen, T)
                    tt.append((time.perf_counter() - t0) * 1e3)
                prepared[group] = T
                print("table G%d log2_table %d: %.2f ms [%.2f .. %.2f] (%d MB)"
                      % (group, T, statistics.median(tt), min(tt), max(tt), (16 << T) >> 20), flush=True)
            xs_typ = rng.integers(0, 1 << bits, size=N, dtype=np.uint64)
            xs_wst = (1 << bits) + np.arange(N, dtype=np.uint64)
            P_typ = dev(eng.g_mul_batch(group, gen, fr(xs_typ), broadcast=True))
            P_wst = dev(eng.g_mul_batch(group, gen, fr(xs_wst), broadcast=True))
            out = torch.empty(N * 32, dtype=torch.uint8, device="cuda:0")
            found = torch.empty(N, dtype=torch.uint8, device="cuda:0")

            def timed(P):
                eng.sync()
                t0 = time.perf_counter()
                eng.dlog_dev(group, P, bits, out, found)
                eng.sync()
                return (time.perf_counter() - t0) * 1e3

            timed(P_typ)  # warm-up, and the check
            assert bool(found.all()) and (out.cpu().numpy().reshape(N, 32) == fr(xs_typ).view(np.uint8).reshape(N, 32)).all()
            timed(P_wst)
            assert not bool(found.any())
            tt, tw = [], []
            for _ in range(ALTERNATIONS):
                tt.append(timed(P_typ))
                tw.append(timed(P_wst))
            mt, mw = statistics.median(tt), statistics.median(tw)
            rate = N * steps_worst / mw * 1e3
            print("2^%d G%d bits %d log2_table %d (%d steps worst): typical %.2f ms [%.2f .. %.2f], worst %.2f ms "
                  "[%.2f .. %.2f] = %.3g steps/s = %.3g Fq mul/s (%.3g per lane of %d)"
                  % (log2n, group, bits, T, steps_worst, mt, min(tt), max(tt), mw, min(tw), max(tw), rate,
                     rate * MULS_PER_STEP[group], rate * MULS_PER_STEP[group] / min(N, 65536), min(N, 65536)), flush=True)
eng.close()

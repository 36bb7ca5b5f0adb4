"""Batch-scale parity (GPU): synthetic batches in the BASELINE shapes are proved on
the GPU and compared, equation by equation on a sample, with the C restatement of
the reference path (oracle/gs_ref.c); the whole batch goes through the
size-independent properties: every honest proof verifies, every corrupted one is
rejected, batched (RLC) and exact verdicts agree, prove-only == commit_and_prove."""
import os
import sys

import numpy as np
import pytest

from gsutil import REPO

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(REPO, "oracle"))


def _run(curve_id, cname, ty, N, m, n, sample):
    from gpubatch import run_batch

    run_batch(curve_id, cname, ty, N, m, n, sample)


@pytest.mark.parametrize("ty", [0, 1, 2, 3])
def test_baseline_shape_batches_bls12_381(ty):
    """m = n = 4 (BASELINE shape), 256 equations per type, 3 sampled against the C oracle."""
    _run(0, "bls12_381", ty, 256, 4, 4, [0, 101, 255])


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (2, 9)])
def test_ragged_shapes_ppe(shape):
    m, n = shape
    _run(0, "bls12_381", 0, 64, m, n, [0, 63])


def test_large_arity_ppe():
    """Towards the reference's large bench shape (benches/bench.rs:451-498, m = n = 334): a 40 x 33 PPE
    (1320 Gamma entries, > 2^8 terms per proof element) against the C oracle, prove and verify."""
    _run(0, "bls12_381", 0, 2, 40, 33, [1])


@pytest.mark.parametrize("ty", [1, 2, 3])
def test_large_arity_scalar_types(ty):
    """33 x 32 (>= 1024 Gamma entries): the one-lane-per-output-scalar preparation kernels (k_prep_prove_wide_a/b,
    k_fr_canonical) for the equation types whose rho / sigma scalars depend on Psi / Phi."""
    _run(0, "bls12_381", ty, 2, 33, 32, [0, 1])


def test_reference_large_bench_shape_334x334():
    """The reference's large bench statement (benches/bench.rs:451-498, 531-578): ONE PPE with m = n = 334.  Proof and
    commitments bit-exact against the C oracle (whose Gamma * d runs its rows on the host cores, like the reference's
    Rayon branch), verdict true, corrupted proof rejected.  This is the shape that needs the segmented tree folds
    (k_slot_fold: ~85 partial sums per proof element; k_cell_fold: ~110 Miller partials per cell)."""
    from gpubatch import run_batch

    run_batch(0, "bls12_381", 0, 1, 334, 334, [0], corrupt_every=1, expect=["k_slot_fold.g2", "k_cell_fold"], rlc=False)


@pytest.mark.parametrize("ty,m,n", [(1, 130, 70), (2, 70, 130), (3, 129, 128)])
def test_large_arity_folds_other_types(ty, m, n):
    """Tree folds on the other equation types (a few equations, every one against the oracle)."""
    _run(0, "bls12_381", ty, 3, m, n, [0, 1, 2])


def test_bn254_batch():
    _run(1, "bn254", 0, 128, 4, 4, [0, 77])
    _run(1, "bn254", 1, 64, 3, 2, [5])


def test_full_config1_batch_properties():
    """BASELINE configs[1]: 2^12 PPE 4x4 -- size-independent properties only (bench.py asserts the same)."""
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.workload import Workload

    eng = gs.Engine(0, 0)
    wl = Workload(eng, ty=0, N=4096, m=4, n=4, seed=20241221)
    wl.prove()
    bad = set(wl.corrupt())
    wl.verify()
    eng.sync()
    ok = wl.ok.cpu().numpy()
    assert len(bad) == 4 and [int(v) for v in ok] == [0 if i in bad else 1 for i in range(4096)]
    eng.close()


@pytest.mark.parametrize("launch", ["torchrun", "bare"])
@pytest.mark.parametrize("mode", ["exact", "rlc"])
def test_bench_two_rank_rehearsal(mode, launch):
    """bench.py with 2 ranks, under the driver's launch line (torchrun) AND as the bare `python bench.py --gpus 2`, which
    must start its own two ranks.  On a one-GPU box the ranks share cuda:0 and use gloo (GS_BENCH_BACKEND): this checks
    the launch contract, the per-rank seeds/shards, the barrier + max-over-ranks timing, the failure-count all-reduce
    inside the timed step (exact) and the accumulator all-gather (rlc); the numbers themselves mean nothing."""
    import json
    import subprocess

    env = dict(os.environ, GS_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    tail = [os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--log2n", "8", "--full",
            "--no-cpu", "--mode", mode]
    if launch == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", "29533" if mode == "exact" else "29534"] + tail
    else:
        cmd = [sys.executable] + tail
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 1 and line["scaling"] == "weak"
    assert line["config"]["total_equations"] == 512 and line["config"]["collective_backend"] == "gloo"
    assert line["config"]["rccl_ranks"] == 0 and line["config"]["distinct_devices"] == 1  # a rehearsal, and it says so
    if mode == "exact":
        assert line["config"]["rank_combined_check"] == {"corrupted_on_rank": 1, "failures_seen_by_every_rank": 4}
    assert line["value"] == pytest.approx(2 * 256 / (line["ms_per_step"] / 1e3), rel=1e-6)
    assert line["roofline"]["alu"]["frac"] > 0


def test_bench_inproc_rehearsal():
    """`bench.py --gpus 3 --inproc`: ONE process drives the shards through gs_ctx_create_multi and the device-pointer
    family (gs_multi_prove_batch_dev / _verify_batch_dev, persistent per-shard threads).  On a one-GPU box the three
    shards sit on GPU 0 (GS_BENCH_SHARED=1); the line must report the DISTINCT devices used, the block sizes and the
    strong-scaling contract, and the corrupted proofs of every shard must have been found (asserted inside)."""
    import json
    import subprocess

    env = dict(os.environ, GS_BENCH_SHARED="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "3", "--inproc", "--steps", "1", "--warmup", "1",
           "--log2n", "8", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["shards"] == 3 and line["config"]["devices"] == [0, 0, 0]
    assert line["config"]["total_equations"] == 768 and line["scaling"] == "weak"
    assert line["value"] == pytest.approx(768 / (line["ms_per_step"] / 1e3), rel=1e-6)


def test_bench_driver_line_rehearsal_four_ranks_and_eight_shards():
    """The driver's multi-GPU line, rehearsed as far as a one-GPU box allows.
      * `bench.py --gpus 4 --steps 2 --warmup 1` under gloo with the ranks sharing cuda:0 (the box admits at most six
        processes on its GPU -- this test process is one of them -- so the 8-rank line itself cannot be started here: a
        6-rank attempt was killed by the box's process guard; four ranks walk the same code: per-rank
        seeds and blocks, barrier + max-over-ranks timing, the failure-count all-reduce inside every timed step, the
        rank-combined verdict with corrupted proofs on the LAST rank only, cpu_baseline on rank 0);
      * `bench.py --gpus 8 --inproc` with EIGHT shards of 2^15 equations on the one GPU: 2^18 equations in all
        (configs[3]) through gs_ctx_create_multi and the device-pointer family, corrupted proofs found in every shard
        (asserted inside bench.py)."""
    import json
    import subprocess

    env = dict(os.environ, GS_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--log2n", "10",
           "--full", "--cpu-sample", "32"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 4 and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["config"]["total_equations"] == 4 * 1024 and line["config"]["equations_per_gpu"] == 1024
    assert line["config"]["rank_combined_check"]["corrupted_on_rank"] == 3
    assert line["config"]["rank_combined_check"]["failures_seen_by_every_rank"] == 4
    assert line["config"]["distinct_devices"] == 1 and line["config"]["rccl_ranks"] == 0
    assert line["cpu_baseline"]["value"] > 0  # N > 1 lines carry the CPU baseline too (rank 0's host cores)
    assert line["value"] == pytest.approx(4 * 1024 / (line["ms_per_step"] / 1e3), rel=1e-6)

    env = dict(os.environ, GS_BENCH_SHARED="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8", "--inproc", "--steps", "2", "--warmup", "1",
           "--log2n", "15", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["config"]["shards"] == 8 and line["config"]["total_equations"] == 1 << 18 and line["n_gpus"] == 1
    assert line["value"] == pytest.approx((1 << 18) / (line["ms_per_step"] / 1e3), rel=1e-6)


def test_bench_refuses_fewer_ranks_than_requested():
    """--gpus 4 under a 2-rank launch is an error (exit code 3), not a silently smaller job."""
    import subprocess

    env = dict(os.environ, GS_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29535", os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "1",
           "--log2n", "6", "--no-cpu"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode != 0 and "--gpus 4" in (r.stderr + r.stdout)


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain `bench.py --gpus 1` line carries the headline keys and nothing that --full adds; --dump-outputs writes
    the result buffers of the last timed step (u32 words as float64, verdicts as float32), identical for two runs with
    the same batch arguments (seeded inputs), every honest proof accepted."""
    import json
    import subprocess

    outs = []
    for steps in (2, 1):
        d = tmp_path / ("steps%d" % steps)
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
               "--log2n", "8", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == steps and not {"roofline", "also", "cpu_baseline"} & set(line)
        assert line["value"] == pytest.approx(256 / (line["ms_per_step"] / 1e3), rel=1e-6)
        arrs = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert sorted(arrs) == ["ok", "pi", "theta", "xcoms", "ycoms"]
        assert arrs["ok"].dtype == np.float32 and arrs["ok"].shape == (256,) and (arrs["ok"] == 1).all()
        for k in ("pi", "theta", "xcoms", "ycoms"):
            assert arrs[k].dtype == np.float64 and arrs[k].shape[0] == 256 and arrs[k].any()
        outs.append(arrs)
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("cname,cid", [("bls12_381", 0), ("bn254", 1)])
@pytest.mark.parametrize("ty", [0, 1, 2, 3])
def test_edge_values_against_c_oracle(cname, cid, ty):
    """Degenerate inputs the reference accepts silently: identity witnesses / constants, zero and r-1 scalars, zero
    Gamma rows, no randomness at all, repeated points.  Outputs must still equal the C restatement bit for bit and
    the verdicts (true or false -- the targets are no longer satisfied) must agree.

    The witnesses are patched and the targets kept, so the patched equations 0, 1, 3 and 4 are FALSE statements (the
    oracle's verdict on them is 0; equation 2, without randomness, keeps a satisfied target): a verifier that mishandles
    an identity answers 0 there as well, and this test cannot tell the two apart.  Degenerate equations that are TRUE
    statements, under every forced kernel shape, are in tests/test_gpu_sparse.py (batch: tests/sparsevec.py)."""
    import torch

    import groth_sahai_rs_amd as gs
    import gs_ref_py as ref
    from groth_sahai_rs_amd.workload import CURVES, Workload

    eng = gs.Engine(cid, 0)
    m, n, N = 3, 2, 8
    wl = Workload(eng, ty=ty, N=N, m=m, n=n, seed=4242 + ty, corrupt_every=0)
    sh = wl.sh
    kx, ky, sx, sy, st = sh["kx"], sh["ky"], sh["sx"], sh["sy"], sh["st"]
    r = CURVES[cid]["r"]
    mont = lambda v: torch.from_numpy(np.array([(v * (1 << 256) % r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)],
                                               dtype=np.uint64).view(np.uint8).copy()).to(wl.X.device)

    def put(t, e, per_eq, idx, size, val):  # element idx of equation e in a flat uint8 tensor
        o = e * per_eq * size + idx * size
        t[o:o + size] = val

    zero = lambda size: torch.zeros(size, dtype=torch.uint8, device=wl.X.device)
    rm1 = mont(r - 1)
    # e0: first X is the identity / zero scalar, first Gamma row zero
    put(wl.X, 0, m, 0, sx, zero(sx))
    for j in range(n):
        put(wl.Gamma, 0, m * n, j, 32, zero(32))
    # e1: first Y and first A are identity / zero, every B is identity / zero
    put(wl.Y, 1, n, 0, sy, zero(sy))
    put(wl.A, 1, n, 0, sx, zero(sx))
    for i in range(m):
        put(wl.B, 1, m, i, sy, zero(sy))
    # e2: no randomness at all
    wl.R[2 * m * kx * 32:3 * m * kx * 32] = 0
    wl.S[2 * n * ky * 32:3 * n * ky * 32] = 0
    wl.T[2 * ky * kx * 32:3 * ky * kx * 32] = 0
    # e3: Gamma = 0 and the commit randomness of X is r-1 everywhere
    wl.Gamma[3 * m * n * 32:4 * m * n * 32] = 0
    for i in range(m * kx):
        put(wl.R, 3, m * kx, i, 32, rm1)
    # e4: repeated variables / constants, Gamma of ones and r-1
    put(wl.X, 4, m, 1, sx, wl.X[4 * m * sx:4 * m * sx + sx].clone())
    put(wl.B, 4, m, 1, sy, wl.B[4 * m * sy:4 * m * sy + sy].clone())
    for k in range(m * n):
        put(wl.Gamma, 4, m * n, k, 32, mont(1) if k % 2 else rm1)
    wl.prove()
    wl.verify()
    eng.sync()
    host = lambda t: t.cpu().numpy()
    X, Y, A, B, G, R, S, T = map(host, (wl.X, wl.Y, wl.A, wl.B, wl.Gamma, wl.R, wl.S, wl.T))
    xc, yc, pi, th, tgt, ok = map(host, (wl.xcoms, wl.ycoms, wl.pi, wl.theta, wl.target, wl.ok))
    cut = lambda a, e, sz: a[e * sz:(e + 1) * sz]
    for e in range(6):  # 0..4 patched, 5 untouched
        out = ref.commit_and_prove(cname, ty, m, n, cut(X, e, m * sx), cut(Y, e, n * sy), cut(A, e, n * sx),
                                   cut(B, e, m * sy), cut(G, e, m * n * 32), cut(R, e, m * kx * 32),
                                   cut(S, e, n * ky * 32), cut(T, e, ky * kx * 32), wl.crs)
        for name, got, per in (("xcoms", xc, m * eng.COM1), ("ycoms", yc, n * eng.COM2), ("pi", pi, kx * eng.COM2),
                               ("theta", th, ky * eng.COM1)):
            assert (out[name] == cut(got, e, per)).all(), (ty, e, name)
        want = ref.verify(cname, ty, m, n, cut(A, e, n * sx), cut(B, e, m * sy), cut(G, e, m * n * 32), cut(tgt, e, st),
                          out["xcoms"], out["ycoms"], out["pi"], out["theta"], wl.crs)
        assert int(ok[e]) == want, (ty, e, "verdict")
    assert int(ok[5]) == 1 and int(ok[2]) == 1  # untouched / randomness-free proofs of true statements still verify
    eng.close()


@pytest.mark.parametrize("cname,cid", [("bls12_381", 0), ("bn254", 1)])
@pytest.mark.parametrize("ty", [0, 1, 2, 3])
def test_small_ragged_shapes_all_types(cname, cid, ty):
    """1 x 1, 2 x 3 and 3 x 1 equations of every type on both curves against the C oracle (the reference's own
    statements are 2 x 1); also the smallest batches (N = 1, 3), which take the side-stream and 3-lane paths."""
    for (m, n), N in (((1, 1), 1), ((2, 3), 3), ((3, 1), 5)):
        _run(cid, cname, ty, N, m, n, list(range(N)))

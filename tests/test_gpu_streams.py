"""The caller's stream (gs_set_stream), gs_sync, and two contexts side by side.

Every other GPU test leaves the context on the null stream, where legacy-stream semantics order all blocking work
implicitly: a launch, memset or copy sent to the wrong stream, or a missing event between the context's stream and its
non-blocking side and copy streams, cannot show.  torch and any caller with a stream of its own pass a non-blocking
stream.  Here the calls of tests/ctxhist.py run on such a stream behind a filler of bounded work (ctxhist.on_stream):
the real inputs only arrive on the stream after the filler, and the outputs are cloned on the stream before anything
synchronises.  The filler is asserted to take at least 20 ms (a whole small batch takes 17.5-19 ms).  That is a
detector with a wide window, not a proof.  Expected bytes: fresh context, default stream, held to the oracle."""
import threading

import numpy as np
import pytest

import ctxhist as H
from test_gpu_ctx_history import ORDER_FAMILIES, ORDER_VERIFIERS, precompute, run_order, second_crs

pytestmark = pytest.mark.gpu
CURVES = H.CURVES

# every _dev family at N in {5, 300} and (m, n) in {(4, 4), (2, 3)} (the mixed call: its own two parts)
DEV_CALLS = [
    ("prove", 0, 5, 4, 4), ("prove", 0, 300, 2, 3), ("prove", 0, 300, 4, 4), ("prove", 0, 5, 2, 3),
    ("verify", 0, 5, 4, 4, "forged"), ("verify", 0, 300, 2, 3, "forged"), ("verify", 0, 300, 4, 4, "valid"),
    ("verify", 0, 5, 2, 3, "valid"),
    ("rlc", 0, 5, 4, 4, "valid", 1), ("rlc", 0, 300, 2, 3, "forged", 1),
    ("locate", 0, 300, 4, 4, "forged"), ("locate", 0, 5, 2, 3, "forged"),
    ("eqrlc", 0, 5, 4, 4, "forged"), ("eqrlc", 0, 300, 2, 3, "valid"),
    ("stmtrlc", 0, 5, 2, "forged"), ("stmtrlc", 0, 3, 100, "valid"),
    ("rerand", 0, 5, 4, 4), ("rerand", 0, 300, 2, 3),
    ("commit", "g1", 5, 4), ("commit", "g2", 300, 4),
    ("gmul", 1, 300), ("gmul", 2, 5), ("mpair", 5, 3), ("mpair", 300, 2), ("gtpow", 300), ("gtpow", 5),
    ("validate", 1, 300), ("validate", 2, 5), ("mixed", 65),
]
KEYED_CALLS = [("extract", 1, 5, 4), ("extract", 2, 300, 4), ("xscalar", 300)]


def check(W, name, out, ms, where, seen):
    got, want = H.pack(out), W.expected(name)
    if ms is not None:
        seen.append(ms)
    assert got == want, "%s: %r (filler %s ms): %s" % (where, name, "%.1f" % ms if ms is not None else "-", H.diff(got, want))


# ---- a. every _dev family on a caller stream -------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("cid,cname", CURVES)
def test_dev_calls_on_a_caller_stream(cid, cname, overlap):
    import torch

    W = H.world(cid, cname)
    for nm in DEV_CALLS + KEYED_CALLS:
        W.expected(nm)
    eng, s, seen = W.fresh(), torch.cuda.Stream(), []
    try:
        eng.set_option("overlap", overlap)
        eng.set_stream(s.cuda_stream)
        for nm in DEV_CALLS:
            out, ms = H.on_stream(eng, W.call(nm), s)
            check(W, nm, out, ms, "caller stream, overlap %d" % overlap, seen)
        # a key, extractions, no key, the key again, extractions: each installation behind a filler on the stream
        for round_ in (1, 2):
            H.filler(s)
            eng.set_extraction_key(W.key)
            eng._ctxhist_key = True
            for nm in KEYED_CALLS:
                call = W.call(nm)
                W.prepare(eng, call)  # (the dlog table, once)
                out, ms = H.on_stream(eng, call, s)
                check(W, nm, out, ms, "caller stream, key installed for the %s time" % ("first", "second")[round_ - 1], seen)
            H.filler(s)
            eng.set_extraction_key(None)
            eng._ctxhist_key = False
            with pytest.raises(W.gs.GsError) as ei:
                H.on_stream(eng, W.call(KEYED_CALLS[0]), s, fill=False)
            assert ei.value.code == 3
            s.synchronize()
        print("filler: %.1f .. %.1f ms over %d calls" % (min(seen), max(seen), len(seen)))
    finally:
        s.synchronize()
        eng.close()


# ---- b. host-pointer entries on a caller stream ----------------------------------------------------------------------
HOST_CALLS = [("prove_host", 0, 300, 4, 4), ("verify_host", 0, 300, 4, 4, "forged"), ("rlc_host", 0, 300, 2, 3, "forged"),
              ("rerand_host", 0, 300, 2, 3), ("prove_host", 0, 5, 4, 4)]


@pytest.mark.parametrize("locked", [False, True])
@pytest.mark.parametrize("cid,cname", CURVES)
def test_host_calls_on_a_caller_stream(cid, cname, locked):
    import torch

    W = H.world(cid, cname)
    for nm in HOST_CALLS:
        W.expected(nm)
    eng, s = W.fresh(), torch.cuda.Stream()
    try:
        eng.set_stream(s.cuda_stream)
        for nm in HOST_CALLS:
            call = W.call(nm)
            ins = dict(call.ins)
            if locked:  # page-locked, registered arrays (gs_host_alloc): DMA straight from the caller's memory
                for k, v in call.ins.items():
                    ins[k] = eng.host_alloc(v.size)
                    ins[k][:] = v
            e0, e1 = H.filler(s)  # in flight on the stream while the blocking call is made
            out = call.run(eng, ins)
            s.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms >= H.FILLER_MIN_MS, "the filler took %.1f ms" % ms
            check(W, nm, out, ms, "host call, %s arrays" % ("page-locked" if locked else "pageable"), [])
            if locked:
                for k in call.ins:
                    eng.host_free(ins[k])
    finally:
        s.synchronize()
        eng.close()


# ---- c. gs_sync is enough --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,cname", CURVES)
def test_gs_sync_covers_the_side_streams(cid, cname):
    import torch

    W = H.world(cid, cname)
    names = [("prove", 0, 300, 4, 4), ("prove", 0, 5, 4, 4), ("verify", 0, 300, 2, 3, "forged"), ("rerand", 0, 300, 2, 3),
             ("rlc", 0, 300, 2, 3, "forged", 1)]
    for nm in names:
        W.expected(nm)
    eng, s = W.fresh(), torch.cuda.Stream()
    try:
        eng.set_option("overlap", 1)
        for nm in names:
            out, ms = H.on_stream(eng, W.call(nm), s, sync="engine")
            check(W, nm, out, ms, "gs_sync alone, then a blocking copy of the outputs", [])
    finally:
        s.synchronize()
        eng.close()


# ---- d. switching streams with work in flight ------------------------------------------------------------------------
def reversed_entries(arrs, N):
    return {k: np.ascontiguousarray(v.reshape(N, -1)[::-1]).reshape(-1) for k, v in arrs.items()}


@pytest.mark.parametrize("cid,cname", CURVES)
def test_switching_streams_with_work_in_flight(cid, cname):
    """gs_set_stream drains the context when the handle changes (include/gs_amd.h): the next call's kernels, on the new
    stream, write the very scratch buffers the old stream's kernels still read.  One shape throughout (the grower), so
    that no buffer regrows and syncs on its own; the second call's inputs are the first's with the entries reversed."""
    import torch

    W = H.world(cid, cname)
    name = ("prove", 0) + H.GROW
    N = H.GROW[0]
    call = W.call(name)
    want = H.unpack(call, W.expected(name))
    want_rev = H.pack(reversed_entries(want, N))
    ins_rev = reversed_entries(call.ins, N)
    eng, sa, sb = W.fresh(), torch.cuda.Stream(), torch.cuda.Stream()
    try:
        H.run_plain(eng, call)  # every buffer at its final size
        st1, st2, st3 = H.stage(call), H.stage(call, ins_rev), H.stage(call)
        h1 = H.enqueue(eng, call, sa, staged=st1)  # nothing synchronises from here to the end of the third call,
        h2 = H.enqueue(eng, call, sb, staged=st2)  # except gs_set_stream itself
        h3 = H.enqueue(eng, call, None, staged=st3)
        sa.synchronize()
        sb.synchronize()
        torch.cuda.synchronize()
        o1, ms1 = H.collect(h1, call)
        o2, ms2 = H.collect(h2, call)
        o3, _ = H.collect(h3, call)
        for tag, got, w in (("first, on stream A", H.pack(o1), W.expected(name)), ("second, on stream B", H.pack(o2), want_rev),
                            ("third, on the default stream", H.pack(o3), W.expected(name))):
            assert got == w, "%s (fillers %.1f, %.1f ms): %s" % (tag, ms1, ms2, H.diff(got, w))
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---- e. two contexts, two host threads, two streams, one device ------------------------------------------------------
def in_threads(*fns):
    errs = []

    def wrap(fn):
        def go():
            try:
                fn()
            except BaseException as e:  # noqa: B902 -- reported in the main thread
                errs.append(e)
        return go

    ts = [threading.Thread(target=wrap(fn)) for fn in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]


def stream_runner(eng, s, lock_every=0):
    """runs a call on stream `s`; lock_every = k: before every k-th call the context page-locks, touches and releases
    an array of its own (gs_host_unregister drains EVERY context of the process)"""
    count = [0]
    rng = np.random.default_rng(lock_every)

    def run(call):
        count[0] += 1
        if lock_every and count[0] % lock_every == 0:
            buf = eng.host_buffer(int(rng.integers(1, 64)) * 4096)
            eng.host_register(buf)
            buf[:] = 1
            eng.host_unregister(buf)
        if call.host:
            return H.run_plain(eng, call)
        out, _ = H.on_stream(eng, call, s, fill=False)
        return out
    return run


@pytest.mark.parametrize("variant", ["crs_switch", "page_locking"])
@pytest.mark.parametrize("cid,cname", CURVES)
def test_two_contexts_two_threads(cid, cname, variant):
    import torch

    W = H.world(cid, cname)
    precompute(W, ORDER_VERIFIERS)
    precompute(W, ORDER_FAMILIES)
    C2 = second_crs(W)
    P = ("prove", 0, 5, 4, 4)
    ea, eb = W.fresh(), W.fresh()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    half = len(ORDER_FAMILIES) // 2
    # (ORDER_FAMILIES switches endo off and on again inside its second half: the cut leaves both halves balanced)
    assert not any(st[0] == "opt" for st in ORDER_FAMILIES[:half])

    lock = 0 if variant == "crs_switch" else 3
    ra, rb = stream_runner(ea, sa, lock), stream_runner(eb, sb, lock and lock + 1)

    def first():
        run_order(W, ea, ORDER_VERIFIERS, ra)

    def second():
        run_order(W, eb, ORDER_FAMILIES[:half], rb)
        if variant == "crs_switch":  # drops its reference on the shared tables and takes it again, mid-way
            eb.set_crs(C2["crs"])
            eb._ctxhist_key = False
            got = H.pack(rb(W.call(P)))
            assert got == C2["prove"], "prove under the second CRS beside another context: " + H.diff(got, C2["prove"])
            eb.set_crs(W.crs)
        run_order(W, eb, ORDER_FAMILIES[half:], rb)

    try:
        in_threads(first, second)
    finally:
        torch.cuda.synchronize()
        ea.close()
        eb.close()

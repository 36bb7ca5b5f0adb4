"""Status codes of every prove / verify / rerandomize entry point of the C ABI (include/gs_amd.h) on the calls that
return before any array is used: empty batches, bad shapes, unknown types, a context without a CRS and a null pointer
at every required position.  Raw lib.* calls, as test_status_codes_and_empty_batches in test_gpu_parity.py.

No call here reaches a kernel: every one has either N = 0, a bad shape or type, no CRS, exactly one required
pointer nulled, or (once) an output laid over an input.  Every argument points at its own 4 KiB slice of a 64 KiB
buffer (numpy for the host entries, a device tensor for the _dev ones): the largest array of the N = 1, m = n = 1
shapes used is pi with 768 bytes, so no two arguments overlap and the locate host form's overlap refusal cannot answer
in place of the null check.  No host entry stages an array before it has checked every pointer, but the host forms
of the batched (RLC) verifiers read rho while checking, so the buffers stay valid memory and non-zero."""
import ctypes

import numpy as np
import pytest

from gsutil import curve

pytestmark = pytest.mark.gpu

OK, SHAPE, ARG, NOCRS = 0, 1, 3, 4
PROVE = ("X", "Y", "A", "B", "Gamma", "R", "S", "T", "xcoms", "ycoms", "pi", "theta")
VERIFY = ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta", "ok")
RERAND = ("A", "B", "Gamma", "xcoms", "ycoms", "pi", "theta", "R", "S", "T", "xcoms_out", "ycoms_out", "pi_out",
          "theta_out")
OPTIONAL_COMS = ("xcoms", "ycoms")

# name -> (pointer arguments, the ones that may be NULL, status of N = 0 with every pointer NULL)
ENTRIES = {}
for _sfx in ("", "_dev"):
    for _kind in ("batch", "statement"):
        ENTRIES["gs_prove_%s%s" % (_kind, _sfx)] = (PROVE, OPTIONAL_COMS, OK)
        ENTRIES["gs_verify_%s%s" % (_kind, _sfx)] = (VERIFY, (), OK)
        ENTRIES["gs_rerandomize_%s%s" % (_kind, _sfx)] = (RERAND, (), OK)
# the batched verifiers refuse an empty batch; a _dev form requires every array, the host forms may leave out acc,
# ok_all and info
ENTRIES["gs_verify_batch_rlc_dev"] = (VERIFY[:8] + ("rho", "acc"), (), ARG)
ENTRIES["gs_verify_batch_rlc"] = (VERIFY[:8] + ("rho", "acc", "ok_all"), ("acc", "ok_all"), ARG)
ENTRIES["gs_verify_batch_rlc_locate_dev"] = (VERIFY[:8] + ("rho", "acc", "ok", "info"), (), ARG)
ENTRIES["gs_verify_batch_rlc_locate"] = (VERIFY[:8] + ("rho", "acc", "ok", "info"), ("acc", "info"), ARG)
ENTRIES["gs_verify_statements_rlc_dev"] = (VERIFY[:8] + ("rho", "acc", "ok"), (), ARG)
ENTRIES["gs_verify_statements_rlc"] = (VERIFY[:8] + ("rho", "acc", "ok"), ("acc",), ARG)
MIXED = {"gs_prove_mixed": PROVE, "gs_prove_mixed_dev": PROVE, "gs_verify_mixed": VERIFY, "gs_verify_mixed_dev": VERIFY}


@pytest.fixture(scope="module")
def env():
    import torch

    import groth_sahai_rs_amd as gs

    c = curve("bls12_381")
    e = gs.Engine(0, 0)
    g = c.golden["crs"]
    e.set_crs(np.concatenate([c.com1(g["u"][0]), c.com1(g["u"][1]), c.com2(g["v"][0]), c.com2(g["v"][1]),
                              c.g1(g["g1"]), c.g2(g["g2"]), c.f12(g["gt"])]))
    fresh = gs.Engine(0, 0)  # no CRS
    host = np.ones(1 << 16, dtype=np.uint8)  # non-zero: gs_verify_batch_rlc rejects a zero rho with the same code
    dev = torch.ones(1 << 16, dtype=torch.uint8, device="cuda:0")
    yield dict(e=e, fresh=fresh, host=ctypes.c_void_p(host.ctypes.data), dev=ctypes.c_void_p(dev.data_ptr()),
               keep=(host, dev))
    fresh.close()
    e.close()


Z = ctypes.c_void_p(0)


def _buf(env, name):
    return env["dev"] if name.endswith("_dev") else env["host"]


def _slices(env, name, count):
    """one pointer per argument, 4 KiB apart"""
    base = _buf(env, name).value
    assert count * 4096 <= 1 << 16
    return [ctypes.c_void_p(base + 4096 * i) for i in range(count)]


def _call(env, name, ty, N, m, n, ptrs, ctx=None):
    """the statements pair takes (S, E) where the others take N: N = 1 is S = E = 1, a tuple is (S, E) itself"""
    counts = (N if isinstance(N, tuple) else (N, N)) if "statements" in name else (N,)
    return getattr(env["e"].lib, name)(ctx or env["e"].ctx, ty, *[ctypes.c_size_t(v) for v in counts], m, n, *ptrs)


def _err(env):
    return env["e"].lib.gs_last_error(env["e"].ctx) or b""


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_status(env, name):
    args, optional, empty_rc = ENTRIES[name]
    full = _slices(env, name, len(args))
    # N = 0 (S = 0 or E = 0) with every pointer NULL
    for empty in ((0, 1), (1, 0)) if "statements" in name else (0,):
        assert _call(env, name, 0, empty, 1, 1, [Z] * len(args)) == empty_rc, empty
    # empty variable lists (the reference panics, prove.rs:106-113)
    for m, n in ((0, 1), (1, 0), (-1, 2)):
        assert _call(env, name, 0, 1, m, n, full) == SHAPE, (m, n)
    # optional pointers: nulling them does not turn a shape error into an argument error
    if optional:
        assert _call(env, name, 0, 1, 0, 1, [Z if a in optional else p for a, p in zip(args, full)]) == SHAPE
    # unknown equation type
    assert _call(env, name, 7, 1, 1, 1, full) == ARG
    # no CRS
    assert _call(env, name, 0, 1, 1, 1, full, ctx=env["fresh"].ctx) == NOCRS
    # every required pointer, one at a time
    for i, a in enumerate(args):
        if a in optional:
            continue
        ptrs = list(full)
        ptrs[i] = Z
        for ty in (0, 3):
            assert _call(env, name, ty, 1, 1, 1, ptrs) == ARG, (a, ty)
            assert b"null pointer" in _err(env), (a, ty)


def test_locate_host_refuses_acc_over_target(env):
    """The one host form that refuses overlapping arrays (the C ABI with real data: test_gpu_locate.py)."""
    name = "gs_verify_batch_rlc_locate"
    args = ENTRIES[name][0]
    ptrs = _slices(env, name, len(args))
    ptrs[args.index("acc")] = ptrs[args.index("target")]
    assert _call(env, name, 0, 1, 1, 1, ptrs) == ARG
    assert b"overlaps" in _err(env)


def _parts(name, specs):
    """specs: (ty, N, m, n, shared, {field: pointer})"""
    from groth_sahai_rs_amd.capi import ProvePart, VerifyPart

    struct = ProvePart if "prove" in name else VerifyPart
    arr = (struct * max(len(specs), 1))()
    for a, (ty, N, m, n, shared, ptrs) in zip(arr, specs):
        a.equ_type, a.N, a.m, a.n, a.shared_vars = ty, N, m, n, shared
        for k, v in ptrs.items():
            setattr(a, k, v.value)
    return arr


@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_entry_status(env, name):
    fields = MIXED[name]
    optional = OPTIONAL_COMS if "prove" in name else ()
    lib, ctx = env["e"].lib, env["e"].ctx
    fn = getattr(lib, name)
    p = _buf(env, name)
    full = {k: p for k in fields}
    null = {k: Z for k in fields}
    one = lambda ty=0, N=1, m=1, n=1, shared=0, ptrs=full: _parts(name, [(ty, N, m, n, shared, ptrs)])
    # the part count and the part array
    for nparts in (-1, 9):
        assert fn(ctx, nparts, one()) == ARG
    assert fn(ctx, 0, Z) == OK
    assert fn(ctx, 0, one()) == OK
    assert fn(ctx, 1, Z) == ARG
    # no CRS
    assert fn(env["fresh"].ctx, 1, one()) == NOCRS
    for shared in (0, 1):
        # an empty part is skipped without touching its pointers
        assert fn(ctx, 1, one(N=0, shared=shared, ptrs=null)) == OK
        # shapes and types of a part
        for m, n in ((0, 1), (1, 0), (-1, 2)):
            assert fn(ctx, 1, one(m=m, n=n, shared=shared)) == SHAPE, (m, n)
        if optional:
            assert fn(ctx, 1, one(m=0, shared=shared, ptrs={k: Z if k in optional else p for k in fields})) == SHAPE
        assert fn(ctx, 1, one(ty=7, shared=shared)) == ARG
        # every required pointer of a part, one at a time
        for k in fields:
            if k in optional:
                continue
            for ty in (0, 3):
                assert fn(ctx, 1, one(ty=ty, shared=shared, ptrs=dict(full, **{k: Z}))) == ARG, (k, ty, shared)
                assert b"null pointer" in _err(env), (k, ty, shared)
    # a bad part after an empty one is still found
    bad = _parts(name, [(0, 0, 1, 1, 0, null), (0, 1, 0, 1, 0, full)])
    assert fn(ctx, 2, bad) == SHAPE
    # a part's shape is checked before its N = 0 makes it a no-op
    assert fn(ctx, 1, one(N=0, m=0, ptrs=null)) == SHAPE

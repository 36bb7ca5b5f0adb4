"""ctypes binding of include/gs_amd.h.  Buffers are numpy arrays (host entry
points) or torch CUDA tensors (``*_dev`` entry points, zero-copy via data_ptr)."""
import ctypes
import os

import numpy as np

GS_PPE, GS_MSMEG1, GS_MSMEG2, GS_QUAD = 0, 1, 2, 3
CURVE_BLS12_381, CURVE_BN254 = 0, 1
_ERR = {1: "GS_ERR_SHAPE", 2: "GS_ERR_DEVICE", 3: "GS_ERR_ARG", 4: "GS_ERR_NOCRS", 5: "GS_ERR_ALLOC"}

_HERE = os.path.dirname(os.path.abspath(__file__))

# every symbol include/gs_amd.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "gs_ctx_create", "gs_ctx_destroy", "gs_set_stream", "gs_set_option", "gs_sync", "gs_host_register",
    "gs_host_alloc", "gs_host_free",
    "gs_host_unregister", "gs_last_error", "gs_version", "gs_sizes",
    "gs_set_crs", "gs_crs_generate", "gs_crs_generate_hiding",
    "gs_commit_g1_dev", "gs_commit_g2_dev", "gs_commit_fr_b1_dev", "gs_commit_fr_b2_dev",
    "gs_commit_g1", "gs_commit_g2", "gs_commit_fr_b1", "gs_commit_fr_b2",
    "gs_prove_batch_dev", "gs_prove_batch", "gs_verify_batch_dev", "gs_verify_batch",
    "gs_verify_batch_rlc_dev", "gs_verify_batch_rlc", "gs_gt_finalize",
    "gs_verify_batch_rlc_locate_dev", "gs_verify_batch_rlc_locate",
    "gs_verify_statements_rlc_dev", "gs_verify_statements_rlc",
    "gs_verify_equation_rlc_dev", "gs_verify_equation_rlc",
    "gs_prove_statement_dev", "gs_prove_statement", "gs_verify_statement_dev", "gs_verify_statement",
    "gs_mat_left_mul_com1", "gs_mat_left_mul_com2", "gs_pairing_sum", "gs_fr_matmul",
    "gs_g1_mul_batch", "gs_g2_mul_batch", "gs_g1_mul_batch_dev", "gs_g2_mul_batch_dev",
    "gs_multi_pairing_batch", "gs_multi_pairing_batch_dev", "gs_gt_pow_batch_dev",
    "gs_wire_sizes", "gs_wire_encode_g1", "gs_wire_encode_g2", "gs_wire_decode_g1", "gs_wire_decode_g2",
    "gs_wire_encode_fr", "gs_wire_decode_fr", "gs_wire_encode_gt", "gs_wire_decode_gt",
    "gs_validate_points", "gs_validate_points_dev",
    "gs_prof_enable", "gs_prof_reset", "gs_prof_get", "gs_prof_get_work", "gs_prof_get_clock",
    "gs_ctx_create_multi", "gs_multi_destroy", "gs_multi_ndev", "gs_multi_ctx", "gs_multi_last_error",
    "gs_multi_uses_rccl", "gs_multi_shard", "gs_multi_set_crs", "gs_multi_prove_batch", "gs_multi_verify_batch",
    "gs_multi_verify_batch_rlc",
    "gs_ctx_create_multi_ex", "gs_multi_exchange_note", "gs_multi_sync", "gs_multi_set_option", "gs_multi_prove_batch_dev",
    "gs_multi_verify_batch_dev", "gs_multi_verify_batch_rlc_dev", "gs_gt_finalize_dev",
    "gs_prove_mixed_dev", "gs_prove_mixed", "gs_verify_mixed_dev", "gs_verify_mixed",
    "gs_rerandomize_batch_dev", "gs_rerandomize_batch", "gs_rerandomize_statement_dev", "gs_rerandomize_statement",
    "gs_set_extraction_key", "gs_extract_g1_dev", "gs_extract_g2_dev", "gs_extract_g1", "gs_extract_g2",
    "gs_dlog_prepare", "gs_dlog_g1_dev", "gs_dlog_g2_dev", "gs_dlog_g1", "gs_dlog_g2",
    "gs_extract_scalar_b1_dev", "gs_extract_scalar_b2_dev", "gs_extract_scalar_b1", "gs_extract_scalar_b2",
    "gs_eval_batch_dev", "gs_eval_batch", "gs_eval_statement_dev", "gs_eval_statement",
    "gs_check_witness_batch_dev", "gs_check_witness_batch", "gs_check_witness_statement_dev",
    "gs_check_witness_statement",
    "gs_set_simulation_key", "gs_simulate_batch_dev", "gs_simulate_batch", "gs_simulate_statement_dev",
    "gs_simulate_statement",
    "gs_rand_set_key", "gs_rand_fr_dev", "gs_rand_fr", "gs_rand_rho_dev", "gs_rand_rho",
    "gs_prove_batch_drawn_dev", "gs_prove_batch_drawn", "gs_prove_statement_drawn_dev", "gs_prove_statement_drawn",
    "gs_rerandomize_batch_drawn_dev", "gs_rerandomize_batch_drawn", "gs_rerandomize_statement_drawn_dev",
    "gs_rerandomize_statement_drawn",
]
# the generator's nonce domains (include/gs_amd.h: GS_RAND_*); callers' own draws use domains >= GS_RAND_USER
GS_RAND_PROVE_R, GS_RAND_PROVE_S, GS_RAND_PROVE_T = 0x0101, 0x0102, 0x0103
GS_RAND_RERAND_R, GS_RAND_RERAND_S, GS_RAND_RERAND_T = 0x0201, 0x0202, 0x0203
GS_RAND_RHO = 0x0301
GS_RAND_USER = 0x10000
_HEAD_ARGTYPES = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
# (..., X, Y, A, B, Gamma, uint64 stream, R_out, S_out, T_out, xcoms, ycoms, pi, theta)
_PROVE_DRAWN_ARGTYPES = _HEAD_ARGTYPES + [ctypes.c_void_p] * 5 + [ctypes.c_uint64] + [ctypes.c_void_p] * 7
# (..., A, B, Gamma, xcoms, ycoms, pi, theta, uint64 stream, R_out, S_out, T_out, the four outputs)
_RERAND_DRAWN_ARGTYPES = _HEAD_ARGTYPES + [ctypes.c_void_p] * 7 + [ctypes.c_uint64] + [ctypes.c_void_p] * 7
# (gs_ctx*, int equ_type, size_t N, int m, int n, X, Y, A, B, Gamma, ...): gs_eval_* end in target_out, gs_check_witness_*
# in target, ok
_EVAL_ARGTYPES = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
_CHECK_ARGTYPES = _EVAL_ARGTYPES + [ctypes.c_void_p]
# (size_t count, const void* in, unsigned bits, void* out_fr, void* found_u8) behind the context
_DLOG_ARGTYPES = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
GS_MIXED_MAX = 8
GS_MULTI_SHARED_DEVICES = 1


class ProvePart(ctypes.Structure):  # gs_prove_part
    _fields_ = [("equ_type", ctypes.c_int), ("N", ctypes.c_size_t), ("m", ctypes.c_int), ("n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("X", "Y", "A", "B", "Gamma", "R", "S", "T", "xcoms", "ycoms", "pi", "theta")] + \
               [("shared_vars", ctypes.c_int)]


class VerifyPart(ctypes.Structure):  # gs_verify_part
    _fields_ = [("equ_type", ctypes.c_int), ("N", ctypes.c_size_t), ("m", ctypes.c_int), ("n", ctypes.c_int)] + \
               [(k, ctypes.c_void_p) for k in ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta", "ok")] + \
               [("shared_vars", ctypes.c_int)]


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_ERR.get(code, "GS_ERR"), code, msg))
        self.code = code


def lib_path():
    # GS_AMD_LIB: load another build of the same library (A/B measurements); it is still a HIP build, never a fallback
    return os.environ.get("GS_AMD_LIB") or os.path.join(_HERE, "lib", "libgs_amd.so")


_LIB = None


def load_library():
    """Load the HIP extension; fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError(
                "groth_sahai_rs_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p
            )
        try:
            # PyTorch-ROCm bundles its own HIP runtime; when both end up in one process torch's copy must be
            # loaded first, otherwise its device discovery fails ("No HIP GPUs are available")
            import torch  # noqa: F401
        except ImportError:
            pass
        _LIB = ctypes.CDLL(p)
        _LIB.gs_last_error.restype = ctypes.c_char_p
        _LIB.gs_version.restype = ctypes.c_char_p
        _LIB.gs_dlog_prepare.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint]
        for n in SYMBOLS:
            if n.startswith(("gs_dlog_g", "gs_extract_scalar_")):
                getattr(_LIB, n).argtypes = _DLOG_ARGTYPES
            elif n.startswith(("gs_eval_", "gs_check_witness_")) and hasattr(_LIB, n):
                # (hasattr: GS_AMD_LIB may name an older build for an A/B run of the entries it does have; calling an
                # entry it lacks still fails loudly, with ctypes' AttributeError)
                getattr(_LIB, n).argtypes = _EVAL_ARGTYPES if n.startswith("gs_eval_") else _CHECK_ARGTYPES
            elif (n.startswith("gs_rand_") or n.endswith(("_drawn", "_drawn_dev"))) and hasattr(_LIB, n):
                # 64-bit stream numbers and offsets: ctypes would pass a bare Python int as a C int
                f = getattr(_LIB, n)
                if n == "gs_rand_set_key":
                    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
                elif n.startswith("gs_rand_fr"):
                    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t,
                                  ctypes.c_void_p]
                elif n.startswith("gs_rand_rho"):
                    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p]
                else:
                    f.argtypes = _PROVE_DRAWN_ARGTYPES if n.startswith("gs_prove_") else _RERAND_DRAWN_ARGTYPES
    return _LIB


def _p(a):
    """void* of a numpy array, torch tensor or None."""
    if a is None:
        return ctypes.c_void_p(0)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return ctypes.c_void_p(a.ctypes.data)
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    # torch tensor
    assert a.is_contiguous()
    return ctypes.c_void_p(a.data_ptr())


def _u8(a):
    """Flat uint8 view of anything numpy can hold contiguously."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _nbytes(a):
    if isinstance(a, np.ndarray):
        return a.nbytes
    return a.numel() * a.element_size()  # torch tensor


def _need(code_name, arrays):
    """Every (name, array, bytes) must hold exactly that many bytes: the C ABI takes bare pointers, so a short proof
    (lengths come from the wire) would otherwise be read past its end.  The reference panics at this point
    (pairing_sum / left_mul asserts, data_structures.rs:495,705): GS_ERR_SHAPE."""
    for name, a, want in arrays:
        if a is None:
            continue
        got = _nbytes(a)
        if got != want:
            raise GsError(1, "%s: %s holds %d bytes, the shape needs %d" % (code_name, name, got, want))


class Engine:
    """One gs_ctx: one GPU, one stream, one CRS."""

    def __init__(self, curve=CURVE_BLS12_381, device=0):
        self.lib = load_library()
        self.curve = curve
        self.ctx = ctypes.c_void_p()
        rc = self.lib.gs_ctx_create(curve, device, ctypes.byref(self.ctx))
        if rc != 0:
            raise GsError(rc, "gs_ctx_create failed (no usable HIP device? there is no CPU fallback)")
        sz = (ctypes.c_size_t * 6)()
        self.lib.gs_sizes(curve, sz)
        self.FQ, self.FR, self.G1, self.G2, self.GT, self.CRS = [int(x) for x in sz]
        self.COM1, self.COM2 = 2 * self.G1, 2 * self.G2

    def close(self):
        if self.ctx:
            # registrations are process-wide and outlive the context: release what THIS engine registered while the
            # arrays are still alive (a stale start -> bytes entry would make a later array that lands on the same
            # addresses pass for page-locked and be moved by DMA against a dead registration)
            for addr in list(getattr(self, "_allocs", {})):
                try:
                    self.lib.gs_host_free(self.ctx, ctypes.c_void_p(addr))
                except Exception:
                    pass
                self._allocs.pop(addr, None)
            for addr in list(getattr(self, "_registered", {})):
                try:
                    self.lib.gs_host_unregister(self.ctx, ctypes.c_void_p(addr))
                except Exception:
                    pass
                self._registered.pop(addr, None)
            self.lib.gs_ctx_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise GsError(rc, (self.lib.gs_last_error(self.ctx) or b"").decode())

    # -- context ------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._chk(self.lib.gs_set_stream(self.ctx, ctypes.c_void_p(stream_handle)))

    def sync(self):
        self._chk(self.lib.gs_sync(self.ctx))

    @staticmethod
    def host_buffer(nbytes):
        """A uint8 array on a fresh anonymous mapping of its own (page-aligned, never part of the allocator's heap):
        what to hand to host_register.  Heap memory is reused without being unmapped, and the runtime may still hold
        its own pin of a freed buffer at the same addresses (include/gs_amd.h, gs_host_register)."""
        import mmap

        return np.frombuffer(mmap.mmap(-1, max(int(nbytes), 1)), dtype=np.uint8)[:nbytes]

    def host_alloc(self, nbytes):
        """A uint8 array over gs_host_alloc memory: pre-faulted, page-locked, registered (DMA-direct in every
        host-pointer call).  Freed by host_free / close."""
        ptr = ctypes.c_void_p()
        self._chk(self.lib.gs_host_alloc(self.ctx, ctypes.c_size_t(max(int(nbytes), 1)), ctypes.byref(ptr)))
        buf = (ctypes.c_uint8 * max(int(nbytes), 1)).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=np.uint8)[:nbytes]
        if not hasattr(self, "_allocs"):
            self._allocs = {}
        self._allocs[ptr.value] = arr
        return arr

    def host_free(self, arr):
        addr = arr.ctypes.data
        self._chk(self.lib.gs_host_free(self.ctx, ctypes.c_void_p(addr)))
        getattr(self, "_allocs", {}).pop(addr, None)

    def host_register(self, arr):
        """Page-lock a numpy array the caller reuses across host-pointer calls (gs_host_register): the pipeline then
        moves it by DMA directly, without the staging copy."""
        addr = arr.ctypes.data
        self._chk(self.lib.gs_host_register(self.ctx, ctypes.c_void_p(addr), ctypes.c_size_t(arr.nbytes)))
        # the registration must not outlive the memory: hold the array (for host_buffer() that is the mmap) until
        # host_unregister / close
        if not hasattr(self, "_registered"):
            self._registered = {}
        self._registered[addr] = arr

    def host_unregister(self, arr):
        addr = arr.ctypes.data
        self._chk(self.lib.gs_host_unregister(self.ctx, ctypes.c_void_p(addr)))
        getattr(self, "_registered", {}).pop(addr, None)

    def set_option(self, key, value):
        """Planner override (include/gs_amd.h, gs_set_option): miller_twin, miller_ch, var_tm, var_mo, var_w, red_k, coop_fe, line_tables,
        overlap; locate_k (0 | 2 | 4 | 8): the arity of verify_batch_rlc_locate's product tree; eq_pi (-1 | 0 | 1): whether
        verify_equation_rlc pairs pi per proof or folds it across the batch in G2.  Results never change,
        only which kernel shapes run (locate_k changes which nodes exist, hence info[1] and what can cancel)."""
        self._chk(self.lib.gs_set_option(self.ctx, key.encode(), int(value)))

    def set_crs(self, crs):
        crs = np.ascontiguousarray(crs).view(np.uint8).reshape(-1)
        assert crs.size == self.CRS, (crs.size, self.CRS)
        self._crs = crs
        self._chk(self.lib.gs_set_crs(self.ctx, _p(crs)))

    def crs_generate(self, p1, p2, scalars, hiding=False):
        """CRS bytes of the reference's shape from generators p1, p2 and scalars (a1, a2, t1, t2); hiding=True gives
        the simulation key of generator.rs:65-77."""
        out = self._out(self.CRS)
        fn = self.lib.gs_crs_generate_hiding if hiding else self.lib.gs_crs_generate
        p1, p2, scalars = _u8(p1), _u8(p2), _u8(scalars)  # named: the buffers must outlive the call
        self._chk(fn(self.ctx, _p(p1), _p(p2), _p(scalars), _p(out)))
        return out

    # -- shapes ---------------------------------------------------------------
    def shape(self, ty):
        xg, yg = ty in (GS_PPE, GS_MSMEG1), ty in (GS_PPE, GS_MSMEG2)
        return dict(xg=xg, yg=yg, kx=2 if xg else 1, ky=2 if yg else 1, sx=self.G1 if xg else self.FR,
                    sy=self.G2 if yg else self.FR,
                    st={GS_PPE: self.GT, GS_MSMEG1: self.G1, GS_MSMEG2: self.G2, GS_QUAD: self.FR}[ty])

    def _sizes(self, ty, N, m, n, shared=False):
        """Bytes of every array of a batch: the table of csrc/gs_layout.h (tests/test_layout.py holds the two against
        each other).  shared: a Statement -- ONE copy of X, Y, R, S and of the commitments for all N equations."""
        sh = self.shape(ty)
        kx, ky, sx, sy, fr, com1, com2 = sh["kx"], sh["ky"], sh["sx"], sh["sy"], self.FR, self.COM1, self.COM2
        V = 1 if shared else N
        return dict(X=V * m * sx, Y=V * n * sy, A=N * n * sx, B=N * m * sy, Gamma=N * m * n * fr, R=V * m * kx * fr,
                    S=V * n * ky * fr, T=N * ky * kx * fr, target=N * sh["st"], xcoms=V * m * com1, ycoms=V * n * com2,
                    pi=N * kx * com2, theta=N * ky * com1, ok=N)

    def _check(self, fn, ty, N, m, n, shared, **arrays):
        """Type, shape and the byte length of every array that is not None (`name_out` is sized like `name`).
        Returns the size table."""
        if not (0 <= ty <= 3) or m < 1 or n < 1:
            raise GsError(1, "%s: bad equation type or empty variable list" % fn)
        want = self._sizes(ty, N, m, n, shared)
        _need(fn, [(k, a, want[k[:-4] if k.endswith("_out") else k]) for k, a in arrays.items()])
        return want

    def _check_prove(self, fn, ty, N, m, n, X, Y, A, B, Gamma, R, S, T, xcoms=None, ycoms=None, pi=None, theta=None):
        return self._check(fn, ty, N, m, n, False, X=X, Y=Y, A=A, B=B, Gamma=Gamma, R=R, S=S, T=T, xcoms=xcoms,
                           ycoms=ycoms, pi=pi, theta=theta)

    def _check_verify(self, fn, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta):
        return self._check(fn, ty, N, m, n, False, A=A, B=B, Gamma=Gamma, target=target, xcoms=xcoms, ycoms=ycoms,
                           pi=pi, theta=theta)

    # -- host entry points (numpy uint8/uint64 arrays) --------------------------
    def _out(self, nbytes):
        return np.zeros(nbytes, dtype=np.uint8)

    def commit(self, kind, vars_, rand):
        fn = {"g1": self.lib.gs_commit_g1, "g2": self.lib.gs_commit_g2, "fr_b1": self.lib.gs_commit_fr_b1,
              "fr_b2": self.lib.gs_commit_fr_b2}[kind]
        vsz = {"g1": self.G1, "g2": self.G2, "fr_b1": self.FR, "fr_b2": self.FR}[kind]
        osz = self.COM1 if kind in ("g1", "fr_b1") else self.COM2
        v = np.ascontiguousarray(vars_).view(np.uint8).reshape(-1)
        r = np.ascontiguousarray(rand).view(np.uint8).reshape(-1)
        n = v.size // vsz
        out = self._out(n * osz)
        self._chk(fn(self.ctx, ctypes.c_size_t(n), _p(v), _p(r), _p(out)))
        return out.reshape(n, osz)

    def prove_batch(self, ty, N, m, n, X, Y, A, B, Gamma, R, S, T, want_coms=True, out=None):
        """`out`: dict of preallocated uint8 arrays xcoms, ycoms, pi, theta to write into (e.g. page-locked ones)."""
        X, Y, A, B, Gamma, R, S, T = map(_u8, (X, Y, A, B, Gamma, R, S, T))
        want = self._check_prove("gs_prove_batch", ty, N, m, n, X, Y, A, B, Gamma, R, S, T)
        if out is not None:
            xc, yc, pi, th = (out.get(k) for k in ("xcoms", "ycoms", "pi", "theta"))
            self._check_prove("gs_prove_batch", ty, N, m, n, *(None,) * 8, xc, yc, pi, th)
            if pi is None or th is None:
                raise GsError(3, "gs_prove_batch: out needs pi and theta")
        else:
            xc = self._out(want["xcoms"]) if want_coms else None
            yc = self._out(want["ycoms"]) if want_coms else None
            pi, th = self._out(want["pi"]), self._out(want["theta"])
        self._chk(self.lib.gs_prove_batch(self.ctx, ty, ctypes.c_size_t(N), m, n, _p(X), _p(Y), _p(A), _p(B), _p(Gamma),
                                          _p(R), _p(S), _p(T), _p(xc), _p(yc), _p(pi), _p(th)))
        return dict(xcoms=xc, ycoms=yc, pi=pi, theta=th)

    def _check_rerand(self, fn, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T, outs=(None,) * 4,
                      shared=False):
        xo, yo, po, to = outs
        return self._check(fn, ty, N, m, n, shared, A=A, B=B, Gamma=Gamma, xcoms=xcoms, ycoms=ycoms, pi=pi,
                           theta=theta, R=R, S=S, T=T, xcoms_out=xo, ycoms_out=yo, pi_out=po, theta_out=to)

    def _rerand_host(self, fn, shared, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T):
        args = list(map(_u8, (A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T)))
        want = self._check_rerand(fn, ty, N, m, n, *args, shared=shared)
        xo, yo, po, to = (self._out(want[k]) for k in ("xcoms", "ycoms", "pi", "theta"))
        self._chk(getattr(self.lib, fn)(self.ctx, ty, ctypes.c_size_t(N), m, n, *[_p(a) for a in args], _p(xo), _p(yo),
                                        _p(po), _p(to)))
        return dict(xcoms=xo, ycoms=yo, pi=po, theta=to)

    def rerandomize_batch(self, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T):
        """Fresh commitments and proofs for N proven equations from fresh randomness R', S', T' (gs_rerandomize_batch):
        no witness.  R', S', T' must be uniform, fresh and secret."""
        return self._rerand_host("gs_rerandomize_batch", False, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta,
                                 R, S, T)

    def rerandomize_statement(self, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T):
        """A Statement's shared commitments xcoms[m], ycoms[n] (updated once with R'[m], S'[n]) and its E proofs
        (gs_rerandomize_statement)."""
        return self._rerand_host("gs_rerandomize_statement", True, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta,
                                 R, S, T)

    # -- simulation with the hiding CRS's trapdoor ---------------------------------------------------------------
    def set_simulation_key(self, key):
        """Install the trapdoor (t1, t2) of the installed hiding CRS: two Montgomery Fr (gs_set_simulation_key); None
        forgets it.  A wrong key or a binding CRS raises GsError code 3 and installs nothing."""
        if key is None:
            self._chk(self.lib.gs_set_simulation_key(self.ctx, _p(None)))
            return
        key = np.ascontiguousarray(key).view(np.uint8).reshape(-1)
        _need("gs_set_simulation_key", [("key", key, 2 * self.FR)])
        self._chk(self.lib.gs_set_simulation_key(self.ctx, _p(key)))

    def _simulate(self, fn, ty, N, m, n, A, B, Gamma, target, Rc, Sc, Tf, outs=None, want_coms=True):
        """gs_simulate_*, host and _dev forms: the byte-length checks of _check_prove (Rc, Sc, Tf are sized like R, S,
        T) before the ABI is crossed, then the call.  A host form allocates its outputs, a _dev form takes them in
        `outs` = (xcoms, ycoms, pi, theta), the first two may be None."""
        dev, shared = fn.endswith("_dev"), "_statement" in fn
        ins = (A, B, Gamma, target, Rc, Sc, Tf)
        if any(a is None for a in ins):
            raise GsError(3, "%s: every input array is required" % fn)
        if not dev:
            ins = tuple(_u8(a) for a in ins)
        want = self._check(fn, ty, N, m, n, shared, **dict(zip(("A", "B", "Gamma", "target", "R", "S", "T"), ins)))
        if dev:
            if outs is None or outs[2] is None or outs[3] is None:
                raise GsError(3, "%s: pi and theta are required" % fn)
        else:
            outs = (self._out(want["xcoms"]) if want_coms else None, self._out(want["ycoms"]) if want_coms else None,
                    self._out(want["pi"]), self._out(want["theta"]))
        self._check(fn, ty, N, m, n, shared, **dict(zip(("xcoms", "ycoms", "pi", "theta"), outs)))
        self._chk(getattr(self.lib, fn)(self.ctx, ty, ctypes.c_size_t(N), m, n, *[_p(a) for a in ins + tuple(outs)]))
        return dict(zip(("xcoms", "ycoms", "pi", "theta"), outs))

    def simulate_batch(self, ty, N, m, n, A, B, Gamma, target, Rc, Sc, Tf, want_coms=True):
        """Commitments and proofs of N equations WITHOUT a witness, from the installed trapdoor (gs_simulate_batch):
        Rc[N][m][kx], Sc[N][n][ky] are the commitments' coordinates in u / v, Tf[N][ky][kx] the free proof scalars, all
        uniform, fresh and secret.  GS_PPE is refused."""
        return self._simulate("gs_simulate_batch", ty, N, m, n, A, B, Gamma, target, Rc, Sc, Tf, want_coms=want_coms)

    def simulate_statement(self, ty, E, m, n, A, B, Gamma, target, Rc, Sc, Tf, want_coms=True):
        """E equations over ONE simulated commitment set Rc[m][kx], Sc[n][ky]; Tf[E][ky][kx] (gs_simulate_statement)."""
        return self._simulate("gs_simulate_statement", ty, E, m, n, A, B, Gamma, target, Rc, Sc, Tf,
                              want_coms=want_coms)

    def simulate_batch_dev(self, ty, N, m, n, A, B, Gamma, target, Rc, Sc, Tf, xcoms, ycoms, pi, theta):
        """Device form (torch tensors): only enqueues on the context's stream."""
        self._simulate("gs_simulate_batch_dev", ty, N, m, n, A, B, Gamma, target, Rc, Sc, Tf, (xcoms, ycoms, pi, theta))

    def simulate_statement_dev(self, ty, E, m, n, A, B, Gamma, target, Rc, Sc, Tf, xcoms, ycoms, pi, theta):
        self._simulate("gs_simulate_statement_dev", ty, E, m, n, A, B, Gamma, target, Rc, Sc, Tf,
                       (xcoms, ycoms, pi, theta))

    # -- randomness drawn on the device (keyed, counter-addressed ChaCha20) ------------------------------------------
    def rand_set_key(self, key):
        """Install the generator's 32-byte key (gs_rand_set_key); None forgets it.  The key comes from a CSPRNG, and a
        (key, stream) pair serves ONE call of one operation."""
        if key is None:
            self._chk(self.lib.gs_rand_set_key(self.ctx, _p(None)))
            return
        key = np.frombuffer(bytes(key), dtype=np.uint8) if isinstance(key, (bytes, bytearray)) else _u8(key)
        _need("gs_rand_set_key", [("key", key, 32)])
        self._chk(self.lib.gs_rand_set_key(self.ctx, _p(key)))

    @staticmethod
    def _u64(fn, **vals):
        for k, v in vals.items():
            if not 0 <= v < (1 << (32 if k == "domain" else 64)):
                raise GsError(3, "%s: %s does not fit its %d bits" % (fn, k, 32 if k == "domain" else 64))

    def rand_fr_dev(self, domain, stream, first, count, out):
        """count uniform Fr of (domain, stream), elements first .. first + count - 1, into a device tensor."""
        self._u64("gs_rand_fr_dev", stream=stream, first=first, count=count, domain=domain)
        _need("gs_rand_fr_dev", [("out", out, count * self.FR)])
        self._chk(self.lib.gs_rand_fr_dev(self.ctx, domain, stream, first, count, _p(out)))

    def rand_fr(self, domain, stream, first, count, out=None):
        self._u64("gs_rand_fr", stream=stream, first=first, count=count, domain=domain)
        if first + count > (1 << 32):  # (before the output is allocated: the C ABI refuses the same draw)
            raise GsError(1, "gs_rand_fr: first + count > 2^32")
        if out is None:
            out = self._out(count * self.FR)
        _need("gs_rand_fr", [("out", out, count * self.FR)])
        self._chk(self.lib.gs_rand_fr(self.ctx, domain, stream, first, count, _p(out)))
        return out

    def rand_rho_dev(self, stream, first, count, out):
        """count non-zero 64-bit exponents of the rho stream `stream` into a device tensor."""
        self._u64("gs_rand_rho_dev", stream=stream, first=first, count=count)
        _need("gs_rand_rho_dev", [("out", out, count * 8)])
        self._chk(self.lib.gs_rand_rho_dev(self.ctx, stream, first, count, _p(out)))

    def rand_rho(self, stream, first, count, out=None):
        self._u64("gs_rand_rho", stream=stream, first=first, count=count)
        if first + count > (1 << 35):
            raise GsError(1, "gs_rand_rho: (first + count + 7) div 8 > 2^32")
        if out is None:
            out = np.zeros(count, dtype=np.uint64)
        _need("gs_rand_rho", [("out", out, count * 8)])
        self._chk(self.lib.gs_rand_rho(self.ctx, stream, first, count, _p(out)))
        return out

    def _prove_drawn(self, fn, ty, N, m, n, X, Y, A, B, Gamma, stream, rst=None, outs=None, want_coms=True,
                     want_rand=True, out=None):
        """gs_prove_*_drawn, host and _dev forms: the length checks of the siblings, then the call.  A host form
        allocates its outputs (R, S, T too when want_rand) or writes into the preallocated uint8 arrays of the dict
        `out` (keys R, S, T, xcoms, ycoms, pi, theta; pi and theta required); a _dev form takes rst = (R_out, S_out,
        T_out), each may be None, and outs = (xcoms, ycoms, pi, theta), the first two may be None."""
        dev, shared = fn.endswith("_dev"), "_statement" in fn
        ins = (X, Y, A, B, Gamma)
        if any(a is None for a in ins):
            raise GsError(3, "%s: every input array is required" % fn)
        self._u64(fn, stream=stream)
        if not dev:
            ins = tuple(_u8(a) for a in ins)
        want = self._check(fn, ty, N, m, n, shared, **dict(zip(("X", "Y", "A", "B", "Gamma"), ins)))
        if dev:
            rst = (None,) * 3 if rst is None else tuple(rst)
            if outs is None or outs[2] is None or outs[3] is None:
                raise GsError(3, "%s: pi and theta are required" % fn)
        elif out is not None:
            rst = tuple(out.get(k) for k in ("R", "S", "T"))
            outs = tuple(out.get(k) for k in ("xcoms", "ycoms", "pi", "theta"))
            if outs[2] is None or outs[3] is None:
                raise GsError(3, "%s: out needs pi and theta" % fn)
        else:
            rst = tuple(self._out(want[k]) if want_rand else None for k in ("R", "S", "T"))
            outs = (self._out(want["xcoms"]) if want_coms else None, self._out(want["ycoms"]) if want_coms else None,
                    self._out(want["pi"]), self._out(want["theta"]))
        names = ("R", "S", "T", "xcoms", "ycoms", "pi", "theta")
        self._check(fn, ty, N, m, n, shared, **dict(zip(names, rst + tuple(outs))))
        self._chk(getattr(self.lib, fn)(self.ctx, ty, N, m, n, *[_p(a) for a in ins], stream,
                                        *[_p(a) for a in rst + tuple(outs)]))
        return dict(zip(names, rst + tuple(outs)))

    def prove_batch_drawn(self, ty, N, m, n, X, Y, A, B, Gamma, stream, want_coms=True, want_rand=True, out=None):
        """gs_prove_batch with R, S, T drawn on the device from (the installed key, stream); they come back under "R",
        "S", "T" when want_rand.  `out`: preallocated arrays to write into, as prove_batch takes them."""
        return self._prove_drawn("gs_prove_batch_drawn", ty, N, m, n, X, Y, A, B, Gamma, stream, want_coms=want_coms,
                                 want_rand=want_rand, out=out)

    def prove_statement_drawn(self, ty, E, m, n, X, Y, A, B, Gamma, stream, want_coms=True, want_rand=True, out=None):
        return self._prove_drawn("gs_prove_statement_drawn", ty, E, m, n, X, Y, A, B, Gamma, stream,
                                 want_coms=want_coms, want_rand=want_rand, out=out)

    def prove_batch_drawn_dev(self, ty, N, m, n, X, Y, A, B, Gamma, stream, R_out, S_out, T_out, xcoms, ycoms, pi,
                              theta):
        self._prove_drawn("gs_prove_batch_drawn_dev", ty, N, m, n, X, Y, A, B, Gamma, stream, (R_out, S_out, T_out),
                          (xcoms, ycoms, pi, theta))

    def prove_statement_drawn_dev(self, ty, E, m, n, X, Y, A, B, Gamma, stream, R_out, S_out, T_out, xcoms, ycoms, pi,
                                  theta):
        self._prove_drawn("gs_prove_statement_drawn_dev", ty, E, m, n, X, Y, A, B, Gamma, stream,
                          (R_out, S_out, T_out), (xcoms, ycoms, pi, theta))

    def _rerand_drawn(self, fn, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream, rst=None, outs=None,
                      want_rand=True):
        """gs_rerandomize_*_drawn, host and _dev forms (see _prove_drawn); all four outputs are required."""
        dev, shared = fn.endswith("_dev"), "_statement" in fn
        ins = (A, B, Gamma, xcoms, ycoms, pi, theta)
        if any(a is None for a in ins):
            raise GsError(3, "%s: every input array is required" % fn)
        self._u64(fn, stream=stream)
        if not dev:
            ins = tuple(_u8(a) for a in ins)
        in_names = ("A", "B", "Gamma", "xcoms", "ycoms", "pi", "theta")
        want = self._check(fn, ty, N, m, n, shared, **dict(zip(in_names, ins)))
        if dev:
            rst = (None,) * 3 if rst is None else tuple(rst)
            if outs is None or any(o is None for o in outs):
                raise GsError(3, "%s: every output array is required" % fn)
        else:
            rst = tuple(self._out(want[k]) if want_rand else None for k in ("R", "S", "T"))
            outs = tuple(self._out(want[k]) for k in ("xcoms", "ycoms", "pi", "theta"))
        self._check(fn, ty, N, m, n, shared, **dict(zip(("R", "S", "T", "xcoms_out", "ycoms_out", "pi_out", "theta_out"),
                                                        rst + tuple(outs))))
        self._chk(getattr(self.lib, fn)(self.ctx, ty, N, m, n, *[_p(a) for a in ins], stream,
                                        *[_p(a) for a in rst + tuple(outs)]))
        return dict(zip(("R", "S", "T", "xcoms", "ycoms", "pi", "theta"), rst + tuple(outs)))

    def rerandomize_batch_drawn(self, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream, want_rand=True):
        """gs_rerandomize_batch with R', S', T' drawn on the device from (the installed key, stream)."""
        return self._rerand_drawn("gs_rerandomize_batch_drawn", ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta,
                                  stream, want_rand=want_rand)

    def rerandomize_statement_drawn(self, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream, want_rand=True):
        return self._rerand_drawn("gs_rerandomize_statement_drawn", ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta,
                                  stream, want_rand=want_rand)

    def rerandomize_batch_drawn_dev(self, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream, R_out, S_out,
                                    T_out, xcoms_out, ycoms_out, pi_out, theta_out):
        self._rerand_drawn("gs_rerandomize_batch_drawn_dev", ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream,
                           (R_out, S_out, T_out), (xcoms_out, ycoms_out, pi_out, theta_out))

    def rerandomize_statement_drawn_dev(self, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, stream, R_out, S_out,
                                        T_out, xcoms_out, ycoms_out, pi_out, theta_out):
        self._rerand_drawn("gs_rerandomize_statement_drawn_dev", ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta,
                           stream, (R_out, S_out, T_out), (xcoms_out, ycoms_out, pi_out, theta_out))

    def set_extraction_key(self, key):
        """Install the binding key (a1, a2) of the installed CRS: two Montgomery Fr (gs_set_extraction_key); None
        forgets it.  A wrong key or a hiding CRS raises GsError code 3 and installs nothing."""
        if key is None:
            self._chk(self.lib.gs_set_extraction_key(self.ctx, _p(None)))
            return
        key = np.ascontiguousarray(key).view(np.uint8).reshape(-1)
        _need("gs_set_extraction_key", [("key", key, 2 * self.FR)])
        self._chk(self.lib.gs_set_extraction_key(self.ctx, _p(key)))

    def _check_extract(self, fn, group, coms, out=None):
        """Byte lengths of an extraction: whole commitments in, one point per commitment out.  Returns the count."""
        if group not in (1, 2):
            raise GsError(3, "%s: group must be 1 or 2" % fn)
        csz, gsz = (self.COM1, self.G1) if group == 1 else (self.COM2, self.G2)
        n = _nbytes(coms) // csz
        _need(fn, [("coms", coms, n * csz), ("out", out, n * gsz)])
        return n

    def extract(self, group, coms):
        """out[i] = coms[i].1 - a coms[i].0 with the installed binding key (gs_extract_g1 / gs_extract_g2): the
        committed G1 / G2 witness, or x * generator for a committed scalar x."""
        coms = np.ascontiguousarray(coms).view(np.uint8).reshape(-1)
        fn = "gs_extract_g1" if group == 1 else "gs_extract_g2"
        n = self._check_extract(fn, group, coms)
        gsz = self.G1 if group == 1 else self.G2
        out = self._out(n * gsz)
        self._chk(getattr(self.lib, fn)(self.ctx, ctypes.c_size_t(n), _p(coms), _p(out)))
        return out.reshape(n, gsz)

    def dlog_prepare(self, group, base, log2_table):
        """Build the baby-step table j * base, j = 1 .. 2^log2_table, for group 1 | 2 (gs_dlog_prepare): 2^(log2_table + 1)
        slots of 8 bytes on the device.  A second call for the group replaces the table."""
        if group not in (1, 2):
            raise GsError(3, "gs_dlog_prepare: group must be 1 or 2")
        base = _u8(base)
        _need("gs_dlog_prepare", [("base", base, self.G1 if group == 1 else self.G2)])
        tabs = self.__dict__.setdefault("_dlog_tables", {})
        tabs.pop(group, None)  # a refused call may already have dropped the old table
        self._chk(self.lib.gs_dlog_prepare(self.ctx, group, _p(base), int(log2_table)))
        tabs[group] = (base.tobytes(), int(log2_table))

    def dlog_table(self, group):
        """(base bytes, log2_table) of the table the last successful dlog_prepare built for the group, or None."""
        return self.__dict__.get("_dlog_tables", {}).get(group)

    def _check_dlog(self, fn, group, pts, out=None, found=None, coms=False):
        """Byte lengths of a bounded discrete logarithm: whole points (coms: whole commitments) in, one Fr and one
        found byte per element out.  Returns the count."""
        if group not in (1, 2):
            raise GsError(3, "%s: group must be 1 or 2" % fn)
        isz = (self.G1 if group == 1 else self.G2) * (2 if coms else 1)
        n = _nbytes(pts) // isz
        _need(fn, [("coms" if coms else "pts", pts, n * isz), ("out", out, n * self.FR), ("found", found, n)])
        return n

    def _dlog_host(self, fn, group, arr, bits, coms):
        arr = _u8(arr)
        n = self._check_dlog(fn, group, arr, coms=coms)
        out, found = self._out(n * self.FR), self._out(n)
        self._chk(getattr(self.lib, fn)(self.ctx, n, _p(arr), int(bits), _p(out), _p(found)))
        return out.reshape(n, self.FR), found

    def dlog(self, group, pts, bits):
        """(xs, found): found[i] = 1 and xs[i] = x (an Fr as commit("fr_b1") takes it) when 0 <= x < 2^bits with
        x * base == pts[i] exists, else 0 and all-zero bytes (gs_dlog_g1 / gs_dlog_g2; base: dlog_prepare)."""
        return self._dlog_host("gs_dlog_g1" if group == 1 else "gs_dlog_g2", group, pts, bits, False)

    def extract_scalar(self, group, coms, bits):
        """(xs, found) of scalar commitments opened with the installed binding key: extract, then dlog on the images
        (gs_extract_scalar_b1 / _b2).  The table must have been prepared with the CRS generator of the group."""
        return self._dlog_host("gs_extract_scalar_b1" if group == 1 else "gs_extract_scalar_b2", group, coms, bits, True)

    def verify_batch(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, ok=None):
        if ok is None:
            ok = np.zeros(N, dtype=np.uint8)
        _need("gs_verify_batch", [("ok", ok, N)])
        A, B, Gamma, target, xcoms, ycoms, pi, theta = map(_u8, (A, B, Gamma, target, xcoms, ycoms, pi, theta))
        self._check_verify("gs_verify_batch", ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta)
        self._chk(self.lib.gs_verify_batch(self.ctx, ty, ctypes.c_size_t(N), m, n, _p(A), _p(B), _p(Gamma), _p(target),
                                           _p(xcoms), _p(ycoms), _p(pi), _p(theta), _p(ok)))
        return ok

    def prove_statement(self, ty, E, m, n, X, Y, A, B, Gamma, R, S, T, want_coms=True):
        """E equations of one type over the SAME variables X[m], Y[n] (commit randomness R, S): commitments once,
        one proof per equation (gs_prove_statement)."""
        X, Y, A, B, Gamma, R, S, T = map(_u8, (X, Y, A, B, Gamma, R, S, T))
        want = self._check("gs_prove_statement", ty, E, m, n, True, X=X, Y=Y, A=A, B=B, Gamma=Gamma, R=R, S=S, T=T)
        xc = self._out(want["xcoms"]) if want_coms else None
        yc = self._out(want["ycoms"]) if want_coms else None
        pi, th = self._out(want["pi"]), self._out(want["theta"])
        self._chk(self.lib.gs_prove_statement(self.ctx, ty, ctypes.c_size_t(E), m, n, _p(X), _p(Y), _p(A), _p(B),
                                              _p(Gamma), _p(R), _p(S), _p(T), _p(xc), _p(yc), _p(pi), _p(th)))
        return dict(xcoms=xc, ycoms=yc, pi=pi, theta=th)

    def verify_statement(self, ty, E, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta):
        A, B, Gamma, target, xcoms, ycoms, pi, theta = map(_u8, (A, B, Gamma, target, xcoms, ycoms, pi, theta))
        self._check("gs_verify_statement", ty, E, m, n, True, A=A, B=B, Gamma=Gamma, target=target, xcoms=xcoms,
                    ycoms=ycoms, pi=pi, theta=theta)
        ok = np.zeros(E, dtype=np.uint8)
        self._chk(self.lib.gs_verify_statement(self.ctx, ty, ctypes.c_size_t(E), m, n, _p(A), _p(B), _p(Gamma),
                                               _p(target), _p(xcoms), _p(ycoms), _p(pi), _p(theta), _p(ok)))
        return ok

    # -- evaluation: an equation's value at a witness, and whether a witness satisfies it -------------------------
    def _eval(self, fn, ty, N, m, n, X, Y, A, B, Gamma, target=None, out=None):
        """gs_eval_* / gs_check_witness_*, host and _dev forms: byte lengths before the ABI is crossed, the output, the
        call.  A `_statement` entry takes ONE copy of X[m], Y[n].  out: target_out (gs_eval_*) or ok (gs_check_witness_*);
        a host form's missing output is allocated here, a _dev form's is refused.  Returns the output."""
        dev, shared, check = fn.endswith("_dev"), "_statement" in fn, fn.startswith("gs_check_witness")
        names = ("X", "Y", "A", "B", "Gamma") + (("target",) if check else ())
        arrays = (X, Y, A, B, Gamma) + ((target,) if check else ())
        if any(a is None for a in arrays):
            raise GsError(3, "%s: %s is required" % (fn, names[[a is None for a in arrays].index(True)]))
        if not dev:
            arrays = tuple(_u8(a) for a in arrays)
        want = self._check(fn, ty, N, m, n, shared, **dict(zip(names, arrays)))
        key = "ok" if check else "target_out"
        if out is None:
            if dev:
                raise GsError(3, "%s: %s is required" % (fn, key))
            out = self._out(want["ok" if check else "target"])
        self._check(fn, ty, N, m, n, shared, **{key: out})
        self._chk(getattr(self.lib, fn)(self.ctx, ty, N, m, n, *[_p(a) for a in arrays], _p(out)))
        return out

    def eval_batch(self, ty, N, m, n, X, Y, A, B, Gamma, target_out=None):
        """The targets of N equations at their witnesses (gs_eval_batch, host arrays): GT / G1 / G2 / Fr per type, in
        the form verify_batch takes them.  Returns target_out (N x target bytes)."""
        return self._eval("gs_eval_batch", ty, N, m, n, X, Y, A, B, Gamma, out=target_out).reshape(N, self.shape(ty)["st"])

    def eval_statement(self, ty, E, m, n, X, Y, A, B, Gamma, target_out=None):
        """The targets of a Statement's E equations over ONE copy of the variables X[m], Y[n] (gs_eval_statement)."""
        return self._eval("gs_eval_statement", ty, E, m, n, X, Y, A, B, Gamma, out=target_out).reshape(E, self.shape(ty)["st"])

    def check_witness_batch(self, ty, N, m, n, X, Y, A, B, Gamma, target, ok=None):
        """ok[e] = 1 iff the witness of equation e satisfies it: its value equals target[e] as an element
        (gs_check_witness_batch, host arrays).  A target with non-canonical limbs never matches."""
        return self._eval("gs_check_witness_batch", ty, N, m, n, X, Y, A, B, Gamma, target, ok)

    def check_witness_statement(self, ty, E, m, n, X, Y, A, B, Gamma, target, ok=None):
        """The same for a Statement's E equations over ONE copy of X[m], Y[n] (gs_check_witness_statement)."""
        return self._eval("gs_check_witness_statement", ty, E, m, n, X, Y, A, B, Gamma, target, ok)

    def eval_batch_dev(self, ty, N, m, n, X, Y, A, B, Gamma, target_out):
        """Device form (torch tensors): only enqueues on the context's stream."""
        self._eval("gs_eval_batch_dev", ty, N, m, n, X, Y, A, B, Gamma, out=target_out)

    def eval_statement_dev(self, ty, E, m, n, X, Y, A, B, Gamma, target_out):
        self._eval("gs_eval_statement_dev", ty, E, m, n, X, Y, A, B, Gamma, out=target_out)

    def check_witness_batch_dev(self, ty, N, m, n, X, Y, A, B, Gamma, target, ok):
        self._eval("gs_check_witness_batch_dev", ty, N, m, n, X, Y, A, B, Gamma, target, ok)

    def check_witness_statement_dev(self, ty, E, m, n, X, Y, A, B, Gamma, target, ok):
        self._eval("gs_check_witness_statement_dev", ty, E, m, n, X, Y, A, B, Gamma, target, ok)

    def _rlc(self, fn, ty, S, N, m, n, arrays, rho, **outs):
        """The batched (RLC) verifiers, host and _dev forms: byte lengths, missing outputs, the call.  arrays: A ..
        theta as verify_batch takes them; S: statements of N = E equations each over shared commitments (None: one
        unshared batch of N); outs: the entry's outputs in the order of its C signature.  A host form's missing output
        is allocated here, a _dev form's is refused.  Returns outs.  gs_verify_equation_rlc[_dev]: N proofs of ONE
        equation -- A, B, Gamma, target are sized as one copy (csrc/gs_layout.h, Layout::one_equation)."""
        dev, stmt = fn.endswith("_dev"), S is not None
        if not dev:
            rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(-1)
            arrays = [_u8(a) for a in arrays]
        if stmt and (S < 1 or N < 1):
            raise GsError(3, "%s: S and E must be >= 1" % fn)
        if not (0 <= ty <= 3) or m < 1 or n < 1:
            raise GsError(1, "%s: bad equation type or empty variable list" % fn)
        k = S if stmt else 1  # combined checks: copies of the layout, accumulator pairs
        one = self._sizes(ty, N, m, n, stmt)
        if fn.startswith("gs_verify_equation_rlc"):
            one.update({key: self._sizes(ty, 1, m, n)[key] for key in ("A", "B", "Gamma", "target")})
        want = dict(rho=32 * k * N, acc=k * 2 * self.GT, ok=S if stmt else N, ok_all=1, info=8)
        keys = ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta")
        _need(fn, [(key, a, k * one[key]) for key, a in zip(keys, arrays)] +
              [(key, a, want[key]) for key, a in [("rho", rho)] + list(outs.items())])
        for key, a in outs.items():
            if a is None and dev:
                raise GsError(3, "%s: %s is required" % (fn, key))
            if a is None:
                outs[key] = np.zeros(2, dtype=np.uint32) if key == "info" else self._out(want[key])
        count = [ctypes.c_size_t(S), ctypes.c_size_t(N)] if stmt else [ctypes.c_size_t(N)]
        self._chk(getattr(self.lib, fn)(self.ctx, ty, *count, m, n,
                                        *[_p(a) for a in list(arrays) + [rho] + list(outs.values())]))
        return outs

    def verify_batch_rlc(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """Batched verifier (host buffers).  rho: uint64[N*4].  Returns (ok_all, acc_pair_bytes)."""
        o = self._rlc("gs_verify_batch_rlc", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                      acc=None, ok_all=None)
        return int(o["ok_all"][0]), o["acc"]

    def verify_batch_rlc_locate(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """Batched verifier with fault localisation (host buffers; the arrays and rho of verify_batch_rlc).  Returns
        (ok[N], info, acc): ok[e] = 0 iff the descent of the kept product tree reached leaf e and it failed, info =
        [number of zeros in ok, number of node checks], acc = the accumulator pair of verify_batch_rlc."""
        o = self._rlc("gs_verify_batch_rlc_locate", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta),
                      rho, acc=None, ok=None, info=None)
        return o["ok"], o["info"], o["acc"]

    def verify_statements_rlc(self, ty, S, E, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """Batched verifier for S statements of E equations each over shared commitments (host buffers; the arrays
        of statement s are what verify_statement takes, at offset s).  rho: uint64[S*E*4], non-zero, from a CSPRNG
        (the rho contract of gs_amd.h).  Returns (ok[S], acc[S][2] GT bytes)."""
        o = self._rlc("gs_verify_statements_rlc", ty, S, E, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                      acc=None, ok=None)
        return o["ok"], o["acc"].reshape(S, 2, self.GT)

    def verify_equation_rlc(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """Batched verifier for N proofs of ONE equation (host buffers): A[n], B[m], Gamma[m][n], target[1] in one copy,
        xcoms[N][m], ycoms[N][n], pi[N][kx], theta[N][ky] per proof.  rho: uint64[N*4], non-zero, from a CSPRNG (the
        rho contract of gs_amd.h).  Returns (ok_all, acc_pair_bytes) in the convention of verify_batch_rlc."""
        o = self._rlc("gs_verify_equation_rlc", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                      acc=None, ok_all=None)
        return int(o["ok_all"][0]), o["acc"]

    def gt_finalize_dev(self, accs_dev, count):
        """the same with `count` pairs in device memory (torch tensor)."""
        _need("gs_gt_finalize_dev", [("accs", accs_dev, count * 2 * self.GT)])
        ok = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.gs_gt_finalize_dev(self.ctx, ctypes.c_size_t(count), _p(accs_dev), _p(ok)))
        return int(ok[0])

    def gt_finalize(self, accs):
        """accs: bytes of `count` accumulator pairs (host).  FE(prod acc[i][0]) == prod acc[i][1] ?"""
        a = np.ascontiguousarray(accs).view(np.uint8).reshape(-1)
        count = a.size // (2 * self.GT)
        ok = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.gs_gt_finalize(self.ctx, ctypes.c_size_t(count), _p(a), _p(ok)))
        return int(ok[0])

    def mat_left_mul(self, group, rows, k, lhs, col):
        fn = self.lib.gs_mat_left_mul_com1 if group == 1 else self.lib.gs_mat_left_mul_com2
        osz = self.COM1 if group == 1 else self.COM2
        out = self._out(rows * osz)
        lhs, col = _u8(lhs), _u8(col)
        _need("gs_mat_left_mul", [("lhs", lhs, rows * k * self.FR), ("col", col, k * osz)])
        self._chk(fn(self.ctx, rows, k, _p(lhs), _p(col), _p(out)))
        return out.reshape(rows, osz)

    def fr_matmul(self, lhs, rhs):
        """Matrix<Fr> product (lists of rows of 4 x u64 Montgomery scalars) on the prover's preparation kernels."""
        rows, inner, cols = len(lhs), len(lhs[0]), len(rhs[0])
        assert len(rhs) == inner and all(len(r) == inner for r in lhs) and all(len(r) == cols for r in rhs)
        pack = lambda mat: np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.uint64).reshape(-1) for r in mat
                                                        for v in r])).view(np.uint8).reshape(-1)
        out = self._out(rows * cols * self.FR)
        a, b = pack(lhs), pack(rhs)  # named: the buffers must outlive the call
        self._chk(self.lib.gs_fr_matmul(self.ctx, rows, inner, cols, _p(a), _p(b), _p(out)))
        o = out.view(np.uint64).reshape(rows, cols, self.FR // 8)
        return [[o[i, j].copy() for j in range(cols)] for i in range(rows)]

    def pairing_sum(self, k, x, y):
        out = self._out(4 * self.GT)
        x, y = _u8(x), _u8(y)
        _need("gs_pairing_sum", [("x", x, k * self.COM1), ("y", y, k * self.COM2)])
        self._chk(self.lib.gs_pairing_sum(self.ctx, k, _p(x), _p(y), _p(out)))
        return out.reshape(4, self.GT)

    def g_mul_batch(self, group, points, scalars, broadcast=False):
        fn = self.lib.gs_g1_mul_batch if group == 1 else self.lib.gs_g2_mul_batch
        gsz = self.G1 if group == 1 else self.G2
        k = _u8(scalars)
        n = k.size // self.FR
        out = self._out(n * gsz)
        points = _u8(points)
        _need("gs_g_mul_batch", [("points", points, (1 if broadcast else n) * gsz)])
        self._chk(fn(self.ctx, ctypes.c_size_t(n), _p(points), 1 if broadcast else 0, _p(k), _p(out)))
        return out.reshape(n, gsz)

    def multi_pairing_batch(self, n, k, P, Q):
        out = self._out(n * self.GT)
        P, Q = _u8(P), _u8(Q)
        _need("gs_multi_pairing_batch", [("P", P, n * k * self.G1), ("Q", Q, n * k * self.G2)])
        self._chk(self.lib.gs_multi_pairing_batch(self.ctx, ctypes.c_size_t(n), k, _p(P), _p(Q), _p(out)))
        return out.reshape(n, self.GT)

    # -- device entry points (torch CUDA uint8 tensors; asynchronous) --------------
    def prove_batch_dev(self, ty, N, m, n, X, Y, A, B, Gamma, R, S, T, xcoms, ycoms, pi, theta):
        self._check_prove("gs_prove_batch_dev", ty, N, m, n, X, Y, A, B, Gamma, R, S, T, xcoms, ycoms, pi, theta)
        self._chk(self.lib.gs_prove_batch_dev(self.ctx, ty, ctypes.c_size_t(N), m, n, _p(X), _p(Y), _p(A), _p(B),
                                              _p(Gamma), _p(R), _p(S), _p(T), _p(xcoms), _p(ycoms), _p(pi),
                                              _p(theta)))

    def _rerand_dev(self, fn, shared, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T, xcoms_out,
                    ycoms_out, pi_out, theta_out):
        outs = (xcoms_out, ycoms_out, pi_out, theta_out)
        self._check_rerand(fn, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T, outs, shared=shared)
        self._chk(getattr(self.lib, fn)(self.ctx, ty, ctypes.c_size_t(N), m, n,
                                        *[_p(a) for a in (A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T) + outs]))

    def rerandomize_batch_dev(self, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T, xcoms_out, ycoms_out,
                              pi_out, theta_out):
        self._rerand_dev("gs_rerandomize_batch_dev", False, ty, N, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T,
                         xcoms_out, ycoms_out, pi_out, theta_out)

    def rerandomize_statement_dev(self, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S, T, xcoms_out,
                                  ycoms_out, pi_out, theta_out):
        self._rerand_dev("gs_rerandomize_statement_dev", True, ty, E, m, n, A, B, Gamma, xcoms, ycoms, pi, theta, R, S,
                         T, xcoms_out, ycoms_out, pi_out, theta_out)

    def verify_batch_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, ok):
        self._check_verify("gs_verify_batch_dev", ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta)
        _need("gs_verify_batch_dev", [("ok", ok, N)])
        self._chk(self.lib.gs_verify_batch_dev(self.ctx, ty, ctypes.c_size_t(N), m, n, _p(A), _p(B), _p(Gamma),
                                               _p(target), _p(xcoms), _p(ycoms), _p(pi), _p(theta), _p(ok)))

    def verify_batch_rlc_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho, acc):
        self._rlc("gs_verify_batch_rlc_dev", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                  acc=acc)

    def verify_batch_rlc_locate_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho, acc, ok, info):
        """Device form: rho uint64[N*4], acc one accumulator pair, ok N bytes, info 2 x uint32, all on the device
        (asynchronous)."""
        self._rlc("gs_verify_batch_rlc_locate_dev", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta),
                  rho, acc=acc, ok=ok, info=info)

    def verify_equation_rlc_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho, acc):
        """Device form: the constants in one copy, rho uint64[N*4], acc one accumulator pair (asynchronous)."""
        self._rlc("gs_verify_equation_rlc_dev", ty, None, N, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                  acc=acc)

    def verify_statements_rlc_dev(self, ty, S, E, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho, acc, ok):
        """Device form: rho uint64[S*E*4], acc S accumulator pairs, ok S bytes, all on the device (asynchronous)."""
        self._rlc("gs_verify_statements_rlc_dev", ty, S, E, m, n, (A, B, Gamma, target, xcoms, ycoms, pi, theta), rho,
                  acc=acc, ok=ok)

    def g_mul_batch_dev(self, group, n, points, broadcast, scalars, out):
        fn = self.lib.gs_g1_mul_batch_dev if group == 1 else self.lib.gs_g2_mul_batch_dev
        self._chk(fn(self.ctx, ctypes.c_size_t(n), _p(points), 1 if broadcast else 0, _p(scalars), _p(out)))

    def extract_dev(self, group, coms, out):
        fn = "gs_extract_g1_dev" if group == 1 else "gs_extract_g2_dev"
        n = self._check_extract(fn, group, coms, out)
        self._chk(getattr(self.lib, fn)(self.ctx, ctypes.c_size_t(n), _p(coms), _p(out)))

    def dlog_dev(self, group, pts, bits, out, found):
        fn = "gs_dlog_g1_dev" if group == 1 else "gs_dlog_g2_dev"
        n = self._check_dlog(fn, group, pts, out, found)
        self._chk(getattr(self.lib, fn)(self.ctx, n, _p(pts), int(bits), _p(out), _p(found)))

    def extract_scalar_dev(self, group, coms, bits, out, found):
        fn = "gs_extract_scalar_b1_dev" if group == 1 else "gs_extract_scalar_b2_dev"
        n = self._check_dlog(fn, group, coms, out, found, coms=True)
        self._chk(getattr(self.lib, fn)(self.ctx, n, _p(coms), int(bits), _p(out), _p(found)))

    def multi_pairing_batch_dev(self, n, k, P, Q, out):
        self._chk(self.lib.gs_multi_pairing_batch_dev(self.ctx, ctypes.c_size_t(n), k, _p(P), _p(Q), _p(out)))

    def gt_pow_batch_dev(self, n, base, k, out):
        self._chk(self.lib.gs_gt_pow_batch_dev(self.ctx, ctypes.c_size_t(n), _p(base), _p(k), _p(out)))

    # -- mixed batches / mixed-type Statements (gs_prove_mixed, gs_verify_mixed) -----------
    def _parts(self, fn, parts, struct, in_keys, out_keys, dev):
        """parts: dicts with ty, N, m, n, the input arrays and (dev) the output arrays; host outputs are allocated
        here (xcoms / ycoms only when the part asks with want_coms, default True).  Every length is checked before a
        pointer crosses the ABI."""
        if len(parts) > GS_MIXED_MAX:
            raise GsError(3, "%s: at most %d parts" % (fn, GS_MIXED_MAX))
        arr = (struct * max(len(parts), 1))()
        keep, outs = [], []
        for i, p in enumerate(parts):
            ty, N, m, n, shared = p["ty"], p["N"], p["m"], p["n"], bool(p.get("shared", False))
            want = self._check(fn, ty, N, m, n, shared)
            a = arr[i]
            a.equ_type, a.N, a.m, a.n, a.shared_vars = ty, N, m, n, 1 if shared else 0
            o = {}
            for k in in_keys:
                v = p[k]
                if not dev:
                    v = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
                _need(fn, [(k, v, want[k])])
                keep.append(v)
                setattr(a, k, _p(v).value)
            for k in out_keys:
                if dev:
                    v = p.get(k)
                    if v is not None:
                        _need(fn, [(k, v, want[k])])
                elif k in ("xcoms", "ycoms") and not p.get("want_coms", True):
                    v = None
                else:
                    v = np.zeros(want[k], dtype=np.uint8)
                keep.append(v)
                o[k] = v
                setattr(a, k, _p(v).value)
            outs.append(o)
        return arr, keep, outs

    def prove_mixed(self, parts):
        """Several sub-batches (any types / shapes) in one call, host arrays.  -> list of dicts of outputs."""
        arr, keep, outs = self._parts("gs_prove_mixed", parts, ProvePart, ("X", "Y", "A", "B", "Gamma", "R", "S", "T"),
                                      ("xcoms", "ycoms", "pi", "theta"), False)
        self._chk(self.lib.gs_prove_mixed(self.ctx, len(parts), arr))
        return outs

    def verify_mixed(self, parts):
        arr, keep, outs = self._parts("gs_verify_mixed", parts, VerifyPart,
                                      ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta"), ("ok",), False)
        self._chk(self.lib.gs_verify_mixed(self.ctx, len(parts), arr))
        return [o["ok"] for o in outs]

    def prove_mixed_dev(self, parts):
        """Device tensors in the part dicts (outputs included); asynchronous on the context's stream."""
        arr, keep, _ = self._parts("gs_prove_mixed_dev", parts, ProvePart, ("X", "Y", "A", "B", "Gamma", "R", "S", "T"),
                                   ("xcoms", "ycoms", "pi", "theta"), True)
        self._chk(self.lib.gs_prove_mixed_dev(self.ctx, len(parts), arr))

    def verify_mixed_dev(self, parts):
        arr, keep, _ = self._parts("gs_verify_mixed_dev", parts, VerifyPart,
                                   ("A", "B", "Gamma", "target", "xcoms", "ycoms", "pi", "theta"), ("ok",), True)
        self._chk(self.lib.gs_verify_mixed_dev(self.ctx, len(parts), arr))

    # -- wire format (ark-serialize byte strings <-> boundary arrays) -------------------
    def wire_sizes(self):
        out = (ctypes.c_size_t * 6)()
        self._chk(self.lib.gs_wire_sizes(self.curve, out))
        return dict(zip(("g1c", "g1u", "g2c", "g2u", "fr", "gt"), [int(v) for v in out]))

    def wire_encode(self, kind, arr, compressed=True):
        """kind in g1|g2|fr|gt; arr: (n, element bytes) boundary values -> (n, wire bytes) uint8."""
        ws = self.wire_sizes()
        arr = np.ascontiguousarray(arr).view(np.uint8)
        esz = {"g1": self.G1, "g2": self.G2, "fr": self.FR, "gt": self.GT}[kind]
        n = arr.size // esz
        wsz = ws[kind + ("c" if compressed else "u")] if kind in ("g1", "g2") else ws[kind]
        out = np.zeros((n, wsz), dtype=np.uint8)
        if n == 0:
            return out
        if kind in ("g1", "g2"):
            fn = self.lib.gs_wire_encode_g1 if kind == "g1" else self.lib.gs_wire_encode_g2
            self._chk(fn(self.ctx, ctypes.c_size_t(n), 1 if compressed else 0, _p(arr), _p(out)))
        else:
            fn = self.lib.gs_wire_encode_fr if kind == "fr" else self.lib.gs_wire_encode_gt
            self._chk(fn(self.ctx, ctypes.c_size_t(n), _p(arr), _p(out)))
        return out

    def wire_decode(self, kind, buf, compressed=True, validate=True):
        """-> (values (n, element bytes) uint8, ok (n,) uint8)."""
        ws = self.wire_sizes()
        buf = np.ascontiguousarray(buf).view(np.uint8)
        esz = {"g1": self.G1, "g2": self.G2, "fr": self.FR, "gt": self.GT}[kind]
        wsz = ws[kind + ("c" if compressed else "u")] if kind in ("g1", "g2") else ws[kind]
        n = buf.size // wsz
        out = np.zeros((n, esz), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return out, ok
        if kind in ("g1", "g2"):
            fn = self.lib.gs_wire_decode_g1 if kind == "g1" else self.lib.gs_wire_decode_g2
            self._chk(fn(self.ctx, ctypes.c_size_t(n), 1 if compressed else 0, 1 if validate else 0, _p(buf), _p(out),
                         _p(ok)))
        elif kind == "fr":
            self._chk(self.lib.gs_wire_decode_fr(self.ctx, ctypes.c_size_t(n), _p(buf), _p(out), _p(ok)))
        else:
            self._chk(self.lib.gs_wire_decode_gt(self.ctx, ctypes.c_size_t(n), 1 if validate else 0, _p(buf), _p(out),
                                                 _p(ok)))
        return out, ok

    def validate_points(self, group, pts):
        """ok[i] = 1 iff point i (boundary limbs; group 1 = G1, 2 = G2) is canonical, on the curve (or the identity)
        and in the prime-order subgroup (gs_validate_points)."""
        pts = np.ascontiguousarray(pts).view(np.uint8).reshape(-1)
        per = self.G1 if group == 1 else self.G2
        assert group in (1, 2) and pts.size % per == 0
        n = pts.size // per
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.gs_validate_points(self.ctx, group, ctypes.c_size_t(n), _p(pts), _p(ok)))
        return ok

    # -- profiling hook ---------------------------------------------------------------
    def prof_enable(self, on=True):
        self.lib.gs_prof_enable(self.ctx, 1 if on else 0)

    def prof_reset(self):
        self.lib.gs_prof_reset(self.ctx)

    def prof_get(self):
        out = []
        i = 0
        while True:
            name = ctypes.create_string_buffer(128)
            ms = ctypes.c_double()
            n = ctypes.c_uint64()
            if self.lib.gs_prof_get(self.ctx, i, name, ctypes.c_size_t(128), ctypes.byref(ms), ctypes.byref(n)) != 0:
                break
            out.append((name.value.decode(), ms.value, n.value))
            i += 1
        return out

    def prof_get_work(self):
        """{kernel name: (lanes, work items)} for the kernels profiled since prof_reset()."""
        out = {}
        for i, (name, _, _) in enumerate(self.prof_get()):
            lanes, work = ctypes.c_uint64(), ctypes.c_uint64()
            self._chk(self.lib.gs_prof_get_work(self.ctx, i, ctypes.byref(lanes), ctypes.byref(work)))
            out[name] = (lanes.value, work.value)
        return out

    def prof_get_clock(self):
        """{kernel name: GHz} -- the clock the profiled launches ran at, stamped inside them (s_memtime /
        s_memrealtime per wave, gs_prof_get_clock); absent for kernels that are not segmented launches."""
        out = {}
        for i, (name, _, _) in enumerate(self.prof_get()):
            ghz = ctypes.c_double()
            self._chk(self.lib.gs_prof_get_clock(self.ctx, i, ctypes.byref(ghz)))
            if ghz.value > 0:
                out[name] = ghz.value
        return out


class MultiEngine:
    """gs_ctx_create_multi: the devices of one node behind one handle.  Host arrays in, host arrays out; the batch is
    cut into contiguous equation blocks, one per device (include/gs_amd.h, multi-GPU section)."""

    def __init__(self, curve=CURVE_BLS12_381, devices=(0,), shared_devices=False):
        """shared_devices=True (GS_MULTI_SHARED_DEVICES) lets several shards name the same ordinal: the ndev > 1 split
        on a one-GPU box."""
        self.lib = load_library()
        self.lib.gs_multi_last_error.restype = ctypes.c_char_p
        self.lib.gs_multi_exchange_note.restype = ctypes.c_char_p
        self.lib.gs_multi_ctx.restype = ctypes.c_void_p
        self.curve = curve
        self.devices = list(devices)
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self.h = ctypes.c_void_p()
        rc = self.lib.gs_ctx_create_multi_ex(curve, arr, len(self.devices),
                                             GS_MULTI_SHARED_DEVICES if shared_devices else 0, ctypes.byref(self.h))
        if rc != 0:
            raise GsError(rc, "gs_ctx_create_multi failed (no usable HIP device? there is no CPU fallback)")
        sz = (ctypes.c_size_t * 6)()
        self.lib.gs_sizes(curve, sz)
        self.FQ, self.FR, self.G1, self.G2, self.GT, self.CRS = [int(x) for x in sz]
        self.COM1, self.COM2 = 2 * self.G1, 2 * self.G2

    shape = Engine.shape
    _sizes = Engine._sizes
    _check = Engine._check
    _check_prove = Engine._check_prove
    _check_verify = Engine._check_verify

    def close(self):
        if self.h:
            self.lib.gs_multi_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise GsError(rc, (self.lib.gs_multi_last_error(self.h) or b"").decode())

    def set_option(self, key, value):
        if key.startswith("exchange_"):  # options of the multi-GPU layer itself (gs_multi_set_option)
            return self._chk(self.lib.gs_multi_set_option(self.h, key.encode(), int(value)))
        for i in range(len(self.devices)):
            ctx = ctypes.c_void_p(self.lib.gs_multi_ctx(self.h, i))
            if self.lib.gs_set_option(ctx, key.encode(), int(value)) != 0:
                raise GsError(3, "gs_set_option(%s)" % key)

    def shard(self, N, i):
        lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
        self._chk(self.lib.gs_multi_shard(self.h, ctypes.c_size_t(N), i, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def uses_rccl(self):
        return bool(self.lib.gs_multi_uses_rccl(self.h))

    def exchange_note(self):
        return (self.lib.gs_multi_exchange_note(self.h) or b"").decode()

    def sync(self):
        self._chk(self.lib.gs_multi_sync(self.h))

    # -- device-resident shards: lists of ndev torch tensors (entry i on devices[i], shard i's block) -----------------
    def _pp(self, lst):
        if lst is None:
            return None
        assert len(lst) == len(self.devices)
        return (ctypes.c_void_p * len(lst))(*[_p(t).value for t in lst])

    def prove_batch_dev(self, ty, N, m, n, X, Y, A, B, Gamma, R, S, T, xcoms, ycoms, pi, theta):
        for i in range(len(self.devices)):
            lo, hi = self.shard(N, i)
            pick = lambda l: None if l is None else l[i]
            if hi > lo:
                self._check_prove("gs_multi_prove_batch_dev", ty, hi - lo, m, n, X[i], Y[i], A[i], B[i], Gamma[i], R[i],
                                  S[i], T[i], pick(xcoms), pick(ycoms), pi[i], theta[i])
        args = [self._pp(a) for a in (X, Y, A, B, Gamma, R, S, T, xcoms, ycoms, pi, theta)]
        self._chk(self.lib.gs_multi_prove_batch_dev(self.h, ty, ctypes.c_size_t(N), m, n, *args))

    def verify_batch_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, ok):
        for i in range(len(self.devices)):
            lo, hi = self.shard(N, i)
            if hi > lo:
                self._check_verify("gs_multi_verify_batch_dev", ty, hi - lo, m, n, A[i], B[i], Gamma[i], target[i],
                                   xcoms[i], ycoms[i], pi[i], theta[i])
                _need("gs_multi_verify_batch_dev", [("ok", ok[i], hi - lo)])
        args = [self._pp(a) for a in (A, B, Gamma, target, xcoms, ycoms, pi, theta, ok)]
        self._chk(self.lib.gs_multi_verify_batch_dev(self.h, ty, ctypes.c_size_t(N), m, n, *args))

    def verify_batch_rlc_dev(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """rho: list of per-shard uint64 device tensors (4 per equation of the shard's block).  -> (ok_all, pairs)"""
        for i in range(len(self.devices)):
            lo, hi = self.shard(N, i)
            if hi > lo:
                self._check_verify("gs_multi_verify_batch_rlc_dev", ty, hi - lo, m, n, A[i], B[i], Gamma[i], target[i],
                                   xcoms[i], ycoms[i], pi[i], theta[i])
                _need("gs_multi_verify_batch_rlc_dev", [("rho", rho[i], 32 * (hi - lo))])
        args = [self._pp(a) for a in (A, B, Gamma, target, xcoms, ycoms, pi, theta, rho)]
        acc = np.zeros(len(self.devices) * 2 * self.GT, dtype=np.uint8)
        okb = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.gs_multi_verify_batch_rlc_dev(self.h, ty, ctypes.c_size_t(N), m, n, *args, _p(acc), _p(okb)))
        return int(okb[0]), acc

    def set_crs(self, crs):
        crs = np.ascontiguousarray(crs).view(np.uint8).reshape(-1)
        assert crs.size == self.CRS
        self._chk(self.lib.gs_multi_set_crs(self.h, _p(crs)))

    def prove_batch(self, ty, N, m, n, X, Y, A, B, Gamma, R, S, T, want_coms=True):
        X, Y, A, B, Gamma, R, S, T = map(_u8, (X, Y, A, B, Gamma, R, S, T))
        want = self._check_prove("gs_multi_prove_batch", ty, N, m, n, X, Y, A, B, Gamma, R, S, T)
        z = lambda k: np.zeros(want[k], dtype=np.uint8)
        xc = z("xcoms") if want_coms else None
        yc = z("ycoms") if want_coms else None
        pi, th = z("pi"), z("theta")
        self._chk(self.lib.gs_multi_prove_batch(self.h, ty, ctypes.c_size_t(N), m, n, _p(X), _p(Y), _p(A), _p(B),
                                                _p(Gamma), _p(R), _p(S), _p(T), _p(xc), _p(yc), _p(pi), _p(th)))
        return dict(xcoms=xc, ycoms=yc, pi=pi, theta=th)

    def verify_batch(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta):
        A, B, Gamma, target, xcoms, ycoms, pi, theta = map(_u8, (A, B, Gamma, target, xcoms, ycoms, pi, theta))
        self._check_verify("gs_multi_verify_batch", ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta)
        ok = np.zeros(N, dtype=np.uint8)
        self._chk(self.lib.gs_multi_verify_batch(self.h, ty, ctypes.c_size_t(N), m, n, _p(A), _p(B), _p(Gamma),
                                                 _p(target), _p(xcoms), _p(ycoms), _p(pi), _p(theta), _p(ok)))
        return ok

    def verify_batch_rlc(self, ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta, rho):
        """-> (ok_all, the ndev gathered accumulator pairs as bytes)"""
        A, B, Gamma, target, xcoms, ycoms, pi, theta = map(_u8, (A, B, Gamma, target, xcoms, ycoms, pi, theta))
        self._check_verify("gs_multi_verify_batch_rlc", ty, N, m, n, A, B, Gamma, target, xcoms, ycoms, pi, theta)
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(-1)
        _need("gs_multi_verify_batch_rlc", [("rho", rho, 32 * N)])
        acc = np.zeros(len(self.devices) * 2 * self.GT, dtype=np.uint8)
        ok = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.gs_multi_verify_batch_rlc(self.h, ty, ctypes.c_size_t(N), m, n, _p(A), _p(B), _p(Gamma),
                                                     _p(target), _p(xcoms), _p(ycoms), _p(pi), _p(theta), _p(rho),
                                                     _p(acc), _p(ok)))
        return int(ok[0]), acc

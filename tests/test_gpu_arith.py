"""The lazy radix-2^28 arithmetic ON THE DEVICE, at its contract limits (tests/arithvec.py has the operands and the checks).

Every number the engine produces goes through csrc/gs_fq28.cuh, whose multipliers are generated instruction streams with
64-bit column accumulators sized to the last bit.  A wrapped accumulator does not fault, it yields a wrong field element;
the prove / verify tests only ever feed it random witnesses, whose column sums sit near half of the worst case, and the CPU
twin replaces the streams by C++.  Here a test-only translation unit over the product's headers (tests/hip/arith_probe.hip,
the operation table of tests/hip/arith_ops.inc, compiled with the engine's own flags) runs each operation lane by lane on
chosen RAW limb vectors and returns the raw result limbs:

  base field   mul sqr norm norm_full vreduce is_zero is_zero_slow eq inv fq_from_boundary fq_to_boundary
  Fp2          mul / mul_l2, sqr / sqr_l2, dot3, mul_xi, mul_fp, inv
  tower        f6_mul f6_mul_by_01 f12_mul f12_sqr f12_mul_by_014 f12_mul_by_034 f12_inv f12_frob f12_eq, and nine
               f12_cyclo_sqr with f12_vreduce after every third (the x-power loop) on pairing values
  curve        the G1 / G2 dbl / madd entry points of the scalar-multiplication loops (the generated subroutines) and
               jac_add, on Jacobian inputs with extreme-limb coordinates, P + P, P + (-P), P + O, O + P, Z a lazy 1

each compared EXACTLY with Python big integers: the value mod p, and the representation the headers promise (unique /
N limbs, value intervals).  No tolerance exists in this project.  The base-field and Fp2 families run a second time on a
build with -DGS_NO_ASM_CALL (the inline multiplier forms of the fallback build; only those two families are compiled into
it).  The probe is built when missing or older than its sources (about 85 s of hipcc for the first build, 12 s for the
second), 64-thread blocks, one launch per (operation, curve), in a child process per (build, curve); a launch that
fails is not repeated and nothing further is launched.  Operands outside a contract are never sent to the device: the
over-contract controls live in tests/test_mul28_gen.py, on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import arithvec as av
from gsutil import HERE, REPO

pytestmark = pytest.mark.gpu

CSRC = os.path.join(REPO, "groth_sahai_rs_amd", "csrc")
SRC = os.path.join(HERE, "hip", "arith_probe.hip")
HIPCC = "/opt/rocm/bin/hipcc"
BUILDS = {"asmcall": [], "noasmcall": ["-DGS_NO_ASM_CALL", "-DARITH_BASE_FP2_ONLY"]}
_failed = []  # a launch that failed: nothing more goes to the device from this module


def probe_path(build):
    return os.path.join(HERE, "hip", "libarith_probe_%s.so" % build)


def build_probe(build, include_dir=CSRC, out=None):
    """compile the probe with the engine's own flags (csrc/Makefile print-flags, as tools/build_variant.sh does)"""
    out = out or probe_path(build)
    srcs = [SRC, os.path.join(HERE, "hip", "arith_ops.inc")] + [
        os.path.join(include_dir, f) for f in os.listdir(include_dir) if f.endswith((".cuh", ".h"))]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        flags = subprocess.check_output(["make", "-s", "-C", CSRC, "print-flags"], text=True).split()
        subprocess.check_call([HIPCC] + flags + BUILDS[build] + ["-shared", "-I" + include_dir, SRC, "-o", out])
    return out


_results = {}


def device_results(build, cname, tmp_path_factory):
    """{op: int32 result limbs} of every operation the build holds, for one curve.  The probe runs in a CHILD process
    (tests/arithvec.py as a script): it is linked against the system's HIP runtime, and a process that has loaded that
    runtime can no longer initialise the one PyTorch ships -- in-process, every GPU test after this module would find no
    device.  One child per (build, curve); it stops at its first failing launch, and after a child that failed or was
    killed at its time limit (or a probe that did not compile) nothing more is started from this module."""
    key = (build, cname)
    if key not in _results:
        if _failed:
            pytest.fail("not launched: %s failed earlier" % (_failed[0],))
        # anything that goes wrong from here on -- a compile error, a child that fails, a child that hangs and is killed at
        # its time limit -- latches: every later test of this module fails at once, nothing is compiled or launched again
        try:
            lib = build_probe(build)
            ops = list(av.OPS) if build == "asmcall" else av.BASE_FP2_OPS
            out = str(tmp_path_factory.mktemp("arith") / ("%s_%s.npz" % key))
            r = subprocess.run([sys.executable, os.path.join(HERE, "arithvec.py"), lib, "probe_run", cname, out,
                                ",".join(ops), "0" if cname == "bls12_381" else "1"], capture_output=True, text=True,
                               cwd=HERE, timeout=300)
        except BaseException as e:
            _failed.append(key + (type(e).__name__,))
            raise
        if r.returncode != 0:
            _failed.append(key + (r.returncode,))
            pytest.fail("the probe's child process ended with status %d:\n%s" % (r.returncode, r.stderr[-2000:]))
        _results[key] = dict(np.load(out))
    return _results[key]


@pytest.mark.parametrize("op", list(av.OPS))
@pytest.mark.parametrize("cname", ["bls12_381", "bn254"])
def test_device_arithmetic_at_contract_limits(tmp_path_factory, cname, op):
    res = device_results("asmcall", cname, tmp_path_factory)
    av.check_all(cname, op, av.op_cases(cname, op), res[op])


@pytest.mark.parametrize("op", av.BASE_FP2_OPS)
@pytest.mark.parametrize("cname", ["bls12_381", "bn254"])
def test_device_arithmetic_inline_multiplier_build(tmp_path_factory, cname, op):
    """the same on the -DGS_NO_ASM_CALL build: gen(L) / gen_sqr(L) inlined, the Fp2 kernels as the compiler's own code"""
    res = device_results("noasmcall", cname, tmp_path_factory)
    av.check_all(cname, op, av.op_cases(cname, op), res[op])

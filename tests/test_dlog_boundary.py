"""CPU checks of the discrete-logarithm boundary: include/gs_amd.h declares, libgs_amd.so exports and the ctypes binding
lists the gs_dlog_* / gs_extract_scalar_* entry points; Engine._check_dlog refuses arrays of the wrong length before a
pointer reaches the C ABI; the C++ host layer's CRS::dlog_prepare / CRS::extract_scalars compile."""
import os
import re
import subprocess

import numpy as np
import pytest

from gsutil import REPO

NAMES = ["gs_dlog_prepare", "gs_dlog_g1_dev", "gs_dlog_g2_dev", "gs_dlog_g1", "gs_dlog_g2", "gs_extract_scalar_b1_dev",
         "gs_extract_scalar_b2_dev", "gs_extract_scalar_b1", "gs_extract_scalar_b2"]


def test_dlog_symbols_declared_and_exported():
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import SYMBOLS

    src = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = gs.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n
        assert n in SYMBOLS


def test_check_dlog_rejects_wrong_lengths_before_the_c_abi():
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import Engine

    e = object.__new__(Engine)  # sizes only: no context (there is no GPU here)
    e.FQ, e.FR, e.G1, e.G2, e.GT, e.CRS = 48, 32, 96, 192, 576, 2016
    e.COM1, e.COM2 = 192, 384
    z = lambda n: np.zeros(n, dtype=np.uint8)
    n = 3
    try:
        for group, pt in ((1, 96), (2, 192)):
            for coms in (False, True):
                isz = pt * (2 if coms else 1)
                inname = "coms" if coms else "pts"
                assert e._check_dlog("t", group, z(n * isz), z(n * 32), z(n), coms=coms) == n
                assert e._check_dlog("t", group, z(n * isz), coms=coms) == n  # the host forms make their own outputs
                assert e._check_dlog("t", group, z(0), z(0), z(0), coms=coms) == 0
                for name, args in ((inname, (z(n * isz - 1), z(n * 32), z(n))), (inname, (z(n * isz + 1), z(n * 32), z(n))),
                                   ("out", (z(n * isz), z(n * 32 - 32), z(n))), ("out", (z(n * isz), z(n * 32 + 1), z(n))),
                                   ("found", (z(n * isz), z(n * 32), z(n - 1))), ("found", (z(n * isz), z(n * 32), z(n + 1)))):
                    with pytest.raises(gs.GsError) as ei:
                        e._check_dlog("t", group, *args, coms=coms)
                    assert ei.value.code == 1 and name in str(ei.value), (name, str(ei.value))
        with pytest.raises(gs.GsError) as ei:
            e._check_dlog("t", 3, z(96), z(32), z(1))
        assert ei.value.code == 3
        with pytest.raises(gs.GsError) as ei:
            e.dlog_prepare(1, z(95), 8)  # a short base never reaches the C ABI
        assert ei.value.code == 1 and "base" in str(ei.value)
        assert e.dlog_table(1) is None and e.dlog_table(2) is None  # nothing was prepared
    finally:
        e.ctx = None  # nothing to destroy


TU = r"""
#include "gs_amd.hpp"
using namespace gs_amd;
std::vector<std::optional<Fr>> open(const CRS& crs, const std::vector<Com1>& a, const std::vector<Com2>& b) {
  crs.dlog_prepare(1, 8);
  crs.dlog_prepare(2, 8);
  std::vector<std::optional<Fr>> r = crs.extract_scalars(a, 16), s = crs.extract_scalars(b, 16);
  r.insert(r.end(), s.begin(), s.end());
  return r;
}
"""


def test_cpp_extract_scalars_compiles(tmp_path):
    src = tmp_path / "dlog_tu.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

"""CPU checks of the rerandomization boundary: include/gs_amd.h declares, libgs_amd.so exports and the ctypes binding
lists the four gs_rerandomize_* entry points, and the C++ host layer's Equation::rerandomize compiles."""
import os
import re
import subprocess

from gsutil import REPO

NAMES = ["gs_rerandomize_batch_dev", "gs_rerandomize_batch", "gs_rerandomize_statement_dev", "gs_rerandomize_statement"]


def test_rerandomize_symbols_declared_and_exported():
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd.capi import SYMBOLS

    src = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = gs.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n
        assert n in SYMBOLS


TU = r"""
#include "gs_amd.hpp"
using namespace gs_amd;
struct Rng { Fr fr() { return Fr{Bytes(32)}; } };
template <class E> CProof again(const E& e, const CProof& p, const CRS& crs, Rng& r) { return e.rerandomize(p, crs, r); }
CProof all(const PPE& a, const MSMEG1& b, const MSMEG2& c, const QuadEqu& d, const CProof& p, const CRS& crs) {
  Rng r;
  again(b, p, crs, r);
  again(c, p, crs, r);
  again(d, p, crs, r);
  return a.rerandomize(p, crs, r);
}
"""


def test_cpp_equation_rerandomize_compiles(tmp_path):
    src = tmp_path / "rerand_tu.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

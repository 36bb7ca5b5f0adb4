"""The C++ host layer's combined check of N showings of one equation (include/gs_amd.hpp: Equation::verify_rlc_many)
driven by tests/cpp/test_eq_rlc.cpp: built with g++ -Werror against the in-tree libgs_amd.so and run on the GPU on the
first equation of each of the four types of the statement blob of test_gpu_stmt_rlc_cpp.py."""
import os
import subprocess

import pytest

from gsutil import HERE, REPO

pytestmark = pytest.mark.gpu


def build_program():
    from test_gpu_cpp_host import BUILD, LIBDIR

    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_eq_rlc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(HERE, "cpp", "test_eq_rlc.cpp"), "-o", exe, "-L" + LIBDIR, "-lgs_amd",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])
def test_cpp_equation_verify_rlc_many(cid, tmp_path):
    import groth_sahai_rs_amd as gs
    from test_gpu_stmt_rlc_cpp import write_statement

    exe = build_program()
    p = str(tmp_path / "statement.bin")
    eng = gs.Engine(cid, 0)
    try:
        write_statement(eng, p)
    finally:
        eng.close()
    r = subprocess.run([exe, p], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)

"""The C++ host layer's combined statement check (include/gs_amd.hpp: Statement::verify_rlc) driven by
tests/cpp/test_stmt_rlc.cpp: built with g++ -Werror against the in-tree libgs_amd.so and run on the GPU on a mixed-type
statement -- two satisfied equations of each of the four types over one list of variables (tests/stmtutil.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gsutil import HERE, REPO

pytestmark = pytest.mark.gpu


def build_program():
    from test_gpu_cpp_host import BUILD, LIBDIR

    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_stmt_rlc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(HERE, "cpp", "test_stmt_rlc.cpp"), "-o", exe, "-L" + LIBDIR, "-lgs_amd",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def write_statement(eng, path, mg=2, ng=3, ms=2, ns=1):
    from stmtutil import StatementInputs

    st = StatementInputs(eng, mg=mg, ng=ng, ms=ms, ns=ns, seed=8200)
    b = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1).tobytes()
    crs = b(st.crs)
    c1, c2 = eng.COM1, eng.COM2
    o = 2 * c1 + 2 * c2
    secs = [crs[:c1], crs[c1:2 * c1], crs[2 * c1:2 * c1 + c2], crs[2 * c1 + c2:o], crs[o:o + eng.G1],
            crs[o + eng.G1:o + eng.G1 + eng.G2], crs[o + eng.G1 + eng.G2:]]
    secs += [b(st.vars[k]) for k in ("xg", "yg", "xs", "ys")]
    for ty in range(4):
        p = st.part(ty, 2)
        secs += [b(p[k]) for k in ("A", "B", "Gamma", "target")]
    with open(path, "wb") as f:
        f.write(struct.pack("<5I", eng.curve, mg, ng, ms, ns))
        for s in secs:
            f.write(struct.pack("<Q", len(s)))
            f.write(s)


@pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])
def test_cpp_statement_verify_rlc(cid, tmp_path):
    import groth_sahai_rs_amd as gs

    exe = build_program()
    p = str(tmp_path / "statement.bin")
    eng = gs.Engine(cid, 0)
    try:
        write_statement(eng, p)
    finally:
        eng.close()
    r = subprocess.run([exe, p], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)

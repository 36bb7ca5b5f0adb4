"""The byte sizes of a batch's arrays are written down twice: csrc/gs_layout.h (what the C ABI stages, shards and
checks with) and Engine._sizes in capi.py (what the binding checks before a pointer crosses the ABI).  This compiles
the header by itself into a small program (host compiler, address + undefined-behaviour sanitizers), lets it print its
table over a grid of curves, types and shapes, and holds every line against the Python table and a few literal
values.  No GPU."""
import os
import subprocess

import pytest

from gsutil import HERE, REPO

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "cpp", "layout_dump.cpp")
CSRC = os.path.join(REPO, "groth_sahai_rs_amd", "csrc")
SHAPES = [(1, 1, 1), (3, 2, 1), (5, 1, 3), (1 << 20, 4096, 1024)]  # the last one overflows a 32-bit product


def engine(fq):
    from groth_sahai_rs_amd.capi import Engine

    e = object.__new__(Engine)  # sizes only: no context
    e.FQ, e.FR, e.G1, e.G2, e.GT = fq, 32, 2 * fq, 4 * fq, 12 * fq
    e.COM1, e.COM2 = 2 * e.G1, 2 * e.G2
    e.ctx = None  # nothing to destroy
    return e


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ for the layout program")
    exe = str(tmp_path_factory.mktemp("layout") / "layout_dump")
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stderr == "", r.stderr  # a sanitizer report
    sizes, shapes = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[2] == "shape":
            shapes[(int(f[0]), int(f[1]))] = [int(v) for v in f[3:]]
        else:
            sizes[tuple(int(v) for v in f[:6]) + (f[6],)] = int(f[7])
    return sizes, shapes


def test_header_and_binding_agree(dump):
    sizes, shapes = dump
    seen = 0
    for fq in (48, 32):  # BLS12-381, BN254
        e = engine(fq)
        assert (e.G1, e.G2, e.GT, e.COM1, e.COM2) == \
            {48: (96, 192, 576, 192, 384), 32: (64, 128, 384, 128, 256)}[fq]
        for ty in range(4):
            sh = e.shape(ty)
            assert shapes[(fq, ty)] == [int(sh["xg"]), int(sh["yg"]), sh["kx"], sh["ky"], sh["sx"], sh["sy"], sh["st"]]
            for shared in (0, 1):
                for N, m, n in SHAPES:
                    want = e._sizes(ty, N, m, n, shared=bool(shared))
                    assert len(want) == 14
                    for name, nbytes in want.items():
                        assert sizes[(fq, ty, shared, N, m, n, name)] == nbytes, (fq, ty, shared, N, m, n, name)
                        seen += 1
    assert seen == len(sizes) == 2 * 4 * 2 * len(SHAPES) * 14


def test_known_values(dump):
    """The literal sizes test_capi_rejects_short_buffers_before_the_c_abi uses (PPE, N = 1, m = 2, n = 1, BLS12-381),
    against both tables; and one product that does not fit 32 bits."""
    sizes, _ = dump
    anchors = dict(A=96, B=384, Gamma=64, target=576, xcoms=384, ycoms=384, pi=768, theta=384)
    got = engine(48)._sizes(0, 1, 2, 1)
    assert {k: got[k] for k in anchors} == anchors
    # the program's grid has m = 2, n = 1 at N = 3: three times the N = 1 sizes, every array here being per equation
    for name, nbytes in anchors.items():
        assert sizes[(48, 0, 0, 3, 2, 1, name)] == 3 * nbytes, name
    # a Statement's variables and commitments do not grow with N
    assert sizes[(48, 0, 1, 3, 2, 1, "xcoms")] == 384 and sizes[(48, 0, 1, 3, 2, 1, "X")] == 2 * 96
    assert sizes[(48, 0, 0, 1 << 20, 4096, 1024, "Gamma")] == (1 << 20) * 4096 * 1024 * 32 > 1 << 32

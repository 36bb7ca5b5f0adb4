"""The C++ host layer's DeviceRng on the GPU (tests/cpp/test_rand.cpp): commit_and_prove -> verify -> rerandomize ->
verify with the randomness drawn on the device, the carried randomness held against the model of tests/randvec.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import randvec as rv
from gsutil import HERE, REPO, curve

pytestmark = pytest.mark.gpu


def write_model(c, ty, m, n, path):
    R, S, T = rv.drawn_rst(rv.KEY_TEST, c.r, ty, 1, m, n, 0)
    R1, S1, _ = rv.drawn_rst(rv.KEY_TEST, c.r, ty, 1, m, n, 1, rerand=True)
    sR, sS, sT = rv.drawn_rst(rv.KEY_TEST, c.r, ty, 2, m, n, 2, shared=True)
    with open(path, "wb") as f:
        for sec in (rv.KEY_TEST, R, S, T, R1, S1, sR, sS, sT):
            b = sec if isinstance(sec, bytes) else np.ascontiguousarray(sec).view(np.uint8).tobytes()
            f.write(struct.pack("<Q", len(b)))
            f.write(b)


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_cpp_device_rng(name, tmp_path):
    from test_gpu_cpp_host import BUILD, LIBDIR, write_case

    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_rand")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(HERE, "cpp", "test_rand.cpp"), "-o", exe, "-L" + LIBDIR, "-lgs_amd",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    c = curve(name)
    for case in c.golden["cases"][4:8]:  # dense 2x2, all four types
        p, q = str(tmp_path / (case["name"] + ".bin")), str(tmp_path / (case["name"] + ".model"))
        write_case(c, case, p)
        write_model(c, case["type"], case["m"], case["n"], q)
        r = subprocess.run([exe, p, q], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (case["name"], r.stdout, r.stderr)

"""The C++ host layer's simulation calls (include/gs_amd.hpp: CRS::generate_hiding_with_trapdoor, set_simulation_key,
Equation::simulate, Statement::simulate) driven by tests/cpp/test_simulate.cpp: built with g++ -Werror against the
in-tree libgs_amd.so and run on the GPU, over the generators of a golden case of each curve."""
import os
import subprocess

import pytest

from gsutil import HERE, REPO, curve

pytestmark = pytest.mark.gpu


def build_program():
    from test_gpu_cpp_host import BUILD, LIBDIR

    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_simulate")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(HERE, "cpp", "test_simulate.cpp"), "-o", exe, "-L" + LIBDIR, "-lgs_amd",
           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_cpp_simulate(name, tmp_path):
    from test_gpu_cpp_host import write_case

    exe = build_program()
    c = curve(name)
    case = next(k for k in c.golden["cases"] if k["type"] == 0)
    p = str(tmp_path / (case["name"] + ".bin"))
    write_case(c, case, p)
    r = subprocess.run([exe, p], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (case["name"], r.stdout, r.stderr)

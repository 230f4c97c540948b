"""dense::compute_backward, compute_backward_multi, solution_jacobians and qp_solve_backward_in_parallel of the C++17 facade
on QPs with box constraints (include/proxsuite/proxqp/dense/compute_ECJ.hpp, parallel/qp_solve.hpp), compiled with g++
-Werror and run as a program (tests/cpp/backward_box_facade_test.cpp) on the QPs and against the oracle numbers of
tests/backward_box_cases.py::case_vs_oracle, which this test writes into a temporary file.  CPU: linked against the
SIMT-emulator build of the device code (test-only).  GPU (`-m gpu`): linked against libproxqp_hip.so."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import backward_box_cases as bx

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "backward_box_facade_test.cpp"
CSRC = ROOT / "proxsuite_amd" / "csrc"


def _compile(out, libdir, libname, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(SRC), "-o",
           str(out), "-L", str(libdir), "-l" + libname, "-L", str(CSRC), "-lpqp_randqp",
           "-Wl,-rpath," + str(libdir), "-Wl,-rpath," + str(CSRC), "-pthread"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def values(oracle, randqp, tmp_path_factory):
    """three QPs of the (20, 7, 9) case, one loss derivative each with x, y, z_in and z_box parts, and the nine jacobians
    of the oracle on the row-stated QPs"""
    B, n, ne, ni = 3, 20, 7, 9
    case = bx.make_case(oracle, randqp, B, n, ne, ni)
    ld = bx.random_rows(B, 1, n, ne, case.nc, dual_rows=1)
    ref, _ = bx.oracle_rows_reference(oracle, case, ld)
    path = tmp_path_factory.mktemp("bwbox") / "values.txt"
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (B, n, ne, ni))
        for i in range(B):
            r = ref[i][0]
            for a in (case.H[i], case.g[i], case.A[i], case.b[i], case.C[i], case.l[i], case.u[i], case.l_box[i], case.u_box[i],
                      ld[i, 0], r["dL_dH"], r["dL_dg"], r["dL_dA"], r["dL_db"], r["dL_dC"], r["dL_du"], r["dL_dl"],
                      r["dL_dl_box"], r["dL_du_box"]):
                f.write(" ".join("%.17g" % v for v in np.asarray(a).ravel()) + "\n")
    return path


def _run(exe, values):
    r = subprocess.run([str(exe), str(values)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout


def test_backward_box_facade_on_emulator(values, tmp_path):
    sys.path.insert(0, str(ROOT / "tests" / "emu"))
    import build as emu_build
    lib = Path(emu_build.build())
    _run(_compile(tmp_path / "backward_box_facade_emu", lib.parent, "pqp_emu"), values)


@pytest.mark.gpu
def test_backward_box_facade_on_gpu(values, tmp_path):
    assert (CSRC / "libproxqp_hip.so").exists(), "build libproxqp_hip.so first (__graft_entry__.build())"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    _run(_compile(tmp_path / "backward_box_facade_hip", CSRC, "proxqp_hip",
                  extra=["-L", rocm + "/lib", "-Wl,-rpath-link," + rocm + "/lib", "-Wl,-rpath," + rocm + "/lib"]), values)

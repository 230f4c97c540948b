"""`-m gpu`: the factors the engine leaves in HBM on a real MI355X, stage by stage and kernel by kernel, against
long-double references of the same operations on the stage's own inputs (tests/factor_cases.py: gates, what each
buffer holds).  On the GPU the matrix-core forms run (ldlt_factor_mfma, diag_block_inverses_mfma, tri_inverse_mfma,
tri_inverse_mfma_rows, both forms of build_ZG, the one-wavefront kernel's factor_schur_reg), which the CPU emulator
replaces by scalar loops: this file is their only direct coverage.

Every case prints its worst ratio per stage; PQP_FACTOR_REPORT=<file> collects the lines (profiles/factor_accuracy.txt
is such a run)."""
import os

import pytest

import factor_cases as fc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import HessianType

pytestmark = pytest.mark.gpu

DENSE, DIAG, ZERO = int(HessianType.Dense), int(HessianType.Diagonal), int(HessianType.Zero)
# primal block: around the 16-column tiles, and 112 / 113 where ldlt_factor_reg hands over to ldlt_factor_mfma
PRIMAL_N = [2, 15, 16, 17, 33, 64, 100, 112, 113, 127, 128]
# dual Schur block of exactly r = n_eq rows (n_in = 0: never edited): 1 .. 8 register tiles of the one-wavefront
# kernel, 112 / 113 where ldlt_inverse_reg hands over to the blocked path of the workgroup kernel
SCHUR_R = [1, 15, 16, 17, 31, 32, 33, 48, 64, 85, 96, 97, 112, 113, 127, 128]
EDITED = [(100, 50, 100), (33, 8, 40), (128, 60, 128)]
REPORT = []


@pytest.fixture(scope="module")
def lib():
    return N.load()  # raises loudly when the HIP library or the device is missing


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    path = os.environ.get("PQP_FACTOR_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(REPORT) + "\n")


def primal_shape(n):
    return n, n // 4, max(1, n // 2)


def test_library_exports_the_accessor(lib):
    assert hasattr(lib.L, "pqp_batch_get_primal_factor")


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("n", PRIMAL_N)
def test_primal_block(lib, randqp, monkeypatch, kernel, n):
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    n, ne, ni = primal_shape(n)
    fc.case_primal_block(lib, randqp, n, ne, ni, B=8, pair=(kernel == "wave"), threads=None if kernel == "wave" else 256,
                         label="%s primal (%d,%d,%d)" % (kernel, n, ne, ni), report=REPORT)


@pytest.mark.parametrize("shape", [(1, 0, 1), (129, 32, 64), (200, 50, 100), (256, 64, 128)])
def test_primal_block_workgroup_sizes(lib, randqp, monkeypatch, shape):
    """one variable; primal blocks beyond the one-wavefront kernel's 128 columns (tri_inverse_mfma_rows)"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", "workgroup")
    fc.case_primal_block(lib, randqp, *shape, B=8, pair=False, threads=256, label="workgroup primal %s" % (shape,), report=REPORT)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("r", SCHUR_R)
def test_schur_block_of_r_rows(lib, randqp, monkeypatch, kernel, r):
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_primal_block(lib, randqp, 128, r, 0, B=8, pair=(kernel == "wave"), threads=None if kernel == "wave" else 256,
                         forward=False, label="%s schur r=%d" % (kernel, r), report=REPORT)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
def test_schur_block_beyond_128_rows(lib, randqp, monkeypatch, kernel):
    """(128, 128, 128): early in a solve the block has n_eq + n_slots > 128 rows (the one-wavefront kernel's blocked path)"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_primal_block(lib, randqp, 128, 128, 128, B=8, pair=(kernel == "wave"), need_r_above=128, early_stops=(1, 2, 3),
                         label="%s schur r>128 (128,128,128)" % kernel, report=REPORT)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("shape", EDITED)
def test_schur_edited(lib, randqp, monkeypatch, kernel, shape):
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_schur_edited(lib, randqp, *shape, B=8, pair=(kernel == "wave"), label="%s edited %s" % (kernel, shape), report=REPORT)


@pytest.mark.parametrize("shape", [(100, 50, 100), (33, 8, 11), (128, 128, 0), (113, 28, 56)])
def test_kernel_agreement(lib, randqp, monkeypatch, shape):
    fc.case_kernel_agreement(lib, randqp, monkeypatch, *shape, B=8)


@pytest.mark.parametrize("shape", [(40, 10, 30), (100, 20, 50)])
def test_box_constraints(lib, randqp, monkeypatch, shape):
    """Z rows of diag(i_scaled), nd = n_eq + n_in + n"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", "workgroup")
    fc.case_primal_block(lib, randqp, *shape, B=8, box=True, pair=False, threads=256, label="workgroup box %s" % (shape,), report=REPORT)


@pytest.mark.parametrize("hessian", [DIAG, ZERO])
@pytest.mark.parametrize("box", [False, True])
def test_identity_factor_general_constraints(lib, randqp, monkeypatch, hessian, box):
    """diagonal / zero Hessian with general C: L = I, Z = B, dF = diag(H_s) + rho -- exact copies -- and G with its gate.
    The Schur factors these solves leave are judged when unedited (the float64 comparator scales the gate).  Edited ones
    are recorded only: with a zero Hessian G = B B^T / rho has entries of 1e6 and the block a condition number of 1e9 -
    1e13, where even a FRESH float64 factorisation of the same S gives 2e-11 - 4e-11 in the metric the project gates at
    1e-11 for strongly convex QPs; an edited factor of that family measured 2.85e-11 (MI355X and emulator alike)."""
    monkeypatch.setenv("PQP_DIAG_KERNEL", "workgroup")
    fc.case_primal_block(lib, randqp, 40, 10, 30, B=8, box=box, hessian=hessian, gate_edited=False, threads=256, pair=False,
                         label="L=I hessian %d box %d" % (hessian, box), report=REPORT)


@pytest.mark.parametrize("hessian", [DIAG, ZERO])
@pytest.mark.parametrize("form", ["C", "box"])
def test_diagonal_structure_mode(lib, randqp, monkeypatch, hessian, form):
    """elementwise Zr, G against their one-line formulas (the 256-thread form of the solver keeps them in HBM)"""
    monkeypatch.setenv("PQP_DIAG_KERNEL", "workgroup")
    n = 70
    fc.case_primal_block(lib, randqp, n, 0, n if form == "C" else 0, B=8, box=(form == "box"), hessian=hessian, diag_c=True,
                         threads=256, label="diagonal structure hessian %d %s" % (hessian, form), report=REPORT)


@pytest.mark.parametrize("shape", [(300, 40, 120, 512), (257, 0, 300, 512), (512, 200, 400, 1024), (600, 100, 50, 1024)])
def test_wide_workgroups(lib, randqp, shape):
    """512- / 1024-thread kernels: LDS-tiled build_ZG, tri_inverse_mfma_rows"""
    n, ne, ni, nt = shape
    fc.case_primal_block(lib, randqp, n, ne, ni, B=4, threads=nt, label="%d threads (%d,%d,%d)" % (nt, n, ne, ni), report=REPORT)


@pytest.mark.parametrize("shape", [(100, 50, 100), (300, 40, 120)])
def test_vectors_in_hbm_instance(lib, randqp, monkeypatch, shape):
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    fc.case_primal_block(lib, randqp, *shape, B=4, threads=1024, label="vectors in HBM %s" % (shape,), report=REPORT)


@pytest.mark.parametrize("dim", [20, 100])
def test_primal_ldlt(lib, randqp, dim):
    fc.case_primal_ldlt_factor(lib, randqp, dim, B=8, threads=256 if dim == 20 else 512,  # (n_eq + n_in + dim rows)
                               label="PrimalLDLT dim %d (2 dim, 2 dim, box)" % dim, report=REPORT)


@pytest.mark.parametrize("shape", [(30, 7, 9, False), (20, 0, 40, False), (100, 50, 100, False)])
def test_primal_ldlt_edited(lib, randqp, shape):
    """the engine forced on generator QPs whose active sets move: factors of P_J edited by pm_rank1"""
    dim, ne, ni, box = shape
    fc.case_primal_ldlt_factor(lib, randqp, dim, B=8, shape=(ne, ni, box), need_edited=True, threads=256,
                               label="PrimalLDLT forced %s" % (shape[:3],), report=REPORT)


@pytest.mark.parametrize("shape", [(160, 40, 80, 256), (300, 40, 120, 512)])
def test_primal_ldlt_blocked(lib, randqp, shape):
    """P_J beyond 112 columns, and in a 512-thread kernel: factor_pm's other branch (ldlt_factor_mfma, then
    tri_inverse_mfma_rows writing W in place) instead of ldlt_inverse_reg"""
    dim, ne, ni, nt = shape
    fc.case_primal_ldlt_factor(lib, randqp, dim, B=4, shape=(ne, ni, False), threads=nt,
                               label="PrimalLDLT forced %s" % (shape[:3],), report=REPORT)


@pytest.mark.parametrize("case", [("wave", 100, 50, 100), ("workgroup", 100, 50, 100), ("workgroup", 113, 28, 56),
                                  ("workgroup", 200, 50, 100), (None, 300, 40, 120)])
def test_ill_conditioned_hessian(lib, randqp, monkeypatch, case):
    """cond(H_s + rho I) ~ 1e8 (strong convexity 1e-6, no preconditioner): where a missing pivot guard or a short Neumann
    product shows first.  The componentwise gates do not depend on the conditioning; the forward leg scales itself."""
    kernel, n, ne, ni = case
    if kernel:
        monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_primal_block(lib, randqp, n, ne, ni, B=8 if n < 300 else 4, cond=True, pair=(kernel == "wave"),
                         threads=512 if kernel is None else (256 if kernel == "workgroup" else None),
                         label="cond 1e8 %s (%d,%d,%d)" % (kernel or "512 threads", n, ne, ni), report=REPORT)

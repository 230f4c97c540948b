"""`-m "not gpu"`: the direct factor checks of tests/factor_cases.py on the CPU SIMT emulator (tests/emu).  The emulator
compiles the PQP_EMULATED_MFMA forms of the matrix-core stages, so this leg proves the test logic, the accessor
pqp_batch_get_primal_factor and the routines without matrix-core instructions (ldlt_factor_reg, ldlt_inverse_reg, the
rank-1 row appends / deletions, the one-wavefront kernel's control flow); tests/test_gpu_factors.py runs every named
shape on the device.

The emulator runs one fiber per GPU thread, and this file is held to two minutes serial.  Against the GPU file that
cost, with two QPs per shape (six / eight for the small edited-factor shapes):
  * Schur blocks of r rows: r = 64, 85, 127 left out (same tile counts as 48, 96, 128 in the register paths), n = 40
    instead of 128 up to r = 40;
  * primal block in the workgroup kernel: n = 1, 2, 17, 112, 113, 128 only (the one-wavefront pair takes the full list
    but 127 through the same 256-thread routine; test_kernel_agreement asserts equal bits);
  * edited factors: (33, 8, 40) and (30, 7, 30) instead of (100, 50, 100) and (128, 60, 128);
  * the Schur block beyond 128 rows in the one-wavefront kernel only (the workgroup kernel's blocked path starts at
    113 rows and is taken by r = 113, 128);
  * box constraints at (40, 10, 30) only; vectors-in-HBM instance at (30, 7, 9); one 512-thread shape, no 1024-thread
    one; PrimalLDLT at dim 12 / 20 instead of 20 / 100; kernel agreement and cond 1e8 at n <= 113."""
import os
import sys

import pytest

import factor_cases as fc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import HessianType

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

DENSE, DIAG, ZERO = int(HessianType.Dense), int(HessianType.Diagonal), int(HessianType.Zero)


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


def primal_shape(n):
    return n, n // 4, max(1, n // 2)


def test_library_exports_the_accessor(lib):
    assert "pqp_batch_get_primal_factor" in N.NativeLib.SYMBOLS
    assert hasattr(lib.L, "pqp_batch_get_primal_factor")


def test_accessor_arguments(lib, randqp):
    """every output is optional; one QP per call; the index is checked"""
    b = fc.solve_batch(lib, randqp, 2, 10, 2, 3)
    assert lib.L.pqp_batch_get_primal_factor(b._h, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.L.pqp_batch_get_primal_factor(b._h, -1, None, None, None, None, None, None, None, None, None) != 0
    assert lib.L.pqp_batch_get_primal_factor(b._h, 2, None, None, None, None, None, None, None, None, None) != 0
    pf = b.primal_factor(1)
    assert pf["meta"] == dict(factor_valid=1, diag_mode=0, backend=1, hessian=DENSE) and pf["rho"] == 1e-6
    assert (pf["i_scaled"] == 1.0).all()  # (no box constraints)
    b.close()


# (both kernels run the primal block through the same 256-thread routine -- test_kernel_agreement asserts equal bits --
# so the workgroup kernel takes the sizes around the tile and hand-over edges only)
@pytest.mark.parametrize("case", [("wave", n) for n in (2, 15, 16, 17, 33, 64, 100, 112, 113, 128)] +
                         [("workgroup", n) for n in (1, 2, 17, 112, 113, 128)])
def test_primal_block(lib, randqp, monkeypatch, case):
    kernel, n = case
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    n, ne, ni = primal_shape(n)
    fc.case_primal_block(lib, randqp, n, ne, ni, B=2, pair=(kernel == "wave"), threads=None if kernel == "wave" else 256)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
@pytest.mark.parametrize("r", [1, 15, 16, 17, 31, 32, 33, 48, 96, 97, 112, 113, 128])
def test_schur_block_of_r_rows(lib, randqp, monkeypatch, kernel, r):
    """n_in = 0: the dual Schur block has exactly r = n_eq rows and is never edited.  (n = 128 as on the GPU once r > 40:
    with n close to r the block's condition number reaches 1e7 and plain float64 factorisations already differ from one
    another by more than the gate's factor 8)"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_primal_block(lib, randqp, 40 if r <= 40 else 128, r, 0, B=2, pair=(kernel == "wave"),
                         threads=None if kernel == "wave" else 256, forward=False)


def test_schur_block_beyond_128_rows(lib, randqp, monkeypatch):
    """(128, 128, 128) in the one-wavefront kernel, whose blocked path starts there (the workgroup kernel's starts at 113
    rows: test_schur_block_of_r_rows)"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", "wave")
    fc.case_primal_block(lib, randqp, 128, 128, 128, B=2, pair=True, need_r_above=128, early_stops=(1,), forward=False)


@pytest.mark.parametrize("case", [("wave", 33, 8, 40, 6), ("workgroup", 33, 8, 40, 6), ("workgroup", 30, 7, 30, 8)])
def test_schur_edited(lib, randqp, monkeypatch, case):
    """(more QPs at the small shapes: a deletion whose trailing rows survive to the end of a solve is seen on a few QPs
    of a batch only)"""
    kernel, n, ne, ni, B = case
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_schur_edited(lib, randqp, n, ne, ni, B=B, pair=(kernel == "wave"))


@pytest.mark.parametrize("shape", [(33, 8, 11), (64, 20, 30)])
def test_kernel_agreement(lib, randqp, monkeypatch, shape):
    fc.case_kernel_agreement(lib, randqp, monkeypatch, *shape, B=2)


def test_box_constraints(lib, randqp, monkeypatch):
    monkeypatch.setenv("PQP_DENSE_KERNEL", "workgroup")
    fc.case_primal_block(lib, randqp, 40, 10, 30, B=2, box=True, pair=False, threads=256)


@pytest.mark.parametrize("hessian", [DIAG, ZERO])
@pytest.mark.parametrize("box", [False, True])
def test_identity_factor_general_constraints(lib, randqp, monkeypatch, hessian, box):
    monkeypatch.setenv("PQP_DIAG_KERNEL", "workgroup")
    fc.case_primal_block(lib, randqp, 40, 10, 30, B=2, box=box, hessian=hessian, gate_edited=False, threads=256, pair=False)


@pytest.mark.parametrize("hessian", [DIAG, ZERO])
@pytest.mark.parametrize("form", ["C", "box"])
def test_diagonal_structure_mode(lib, randqp, monkeypatch, hessian, form):
    monkeypatch.setenv("PQP_DIAG_KERNEL", "workgroup")
    n = 24
    fc.case_primal_block(lib, randqp, n, 0, n if form == "C" else 0, B=2, box=(form == "box"), hessian=hessian, diag_c=True,
                         threads=256)


def test_wide_workgroup(lib, randqp):
    fc.case_primal_block(lib, randqp, 300, 40, 120, B=2, threads=512)


def test_vectors_in_hbm_instance(lib, randqp, monkeypatch):
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    fc.case_primal_block(lib, randqp, 30, 7, 9, B=2, threads=1024)


@pytest.mark.parametrize("dim", [12, 20])
def test_primal_ldlt(lib, randqp, dim):
    fc.case_primal_ldlt_factor(lib, randqp, dim, B=2, threads=256)


@pytest.mark.parametrize("shape", [(30, 7, 9, False), (20, 0, 40, False)])
def test_primal_ldlt_edited(lib, randqp, shape):
    dim, ne, ni, box = shape
    fc.case_primal_ldlt_factor(lib, randqp, dim, B=2, shape=(ne, ni, box), need_edited=True, threads=256)


@pytest.mark.parametrize("case", [("wave", 64, 20, 30), ("workgroup", 64, 20, 30), ("workgroup", 113, 28, 56)])
def test_ill_conditioned_hessian(lib, randqp, monkeypatch, case):
    kernel, n, ne, ni = case
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    fc.case_primal_block(lib, randqp, n, ne, ni, B=2, cond=True, pair=(kernel == "wave"))

"""`-m "not gpu"`: the dispatch cases of tests/dispatch_cases.py on the CPU SIMT emulator (tests/emu), whose device has
ONE compute unit: every threshold of the rule is a handful of QPs there, so every rung is reached, none dropped."""
import os
import sys

import pytest

import dispatch_cases as dc
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

N_CU = 1  # tests/emu/hip_emu.hpp: hipDeviceAttributeMultiprocessorCount


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


def test_no_kernel_before_the_first_solve(lib):
    b = N.Batch(1, *dc.SHAPE, lib=lib)
    assert b.last_kernel == ""
    b.close()


def test_dense_ladder(lib, randqp, monkeypatch):
    assert dc.case_dense_ladder(lib, randqp, monkeypatch, N_CU) == 0


def test_dense_switches(lib, randqp, monkeypatch):
    dc.case_dense_switches(lib, randqp, monkeypatch, N_CU)


def test_lds_bound(lib, randqp, monkeypatch):
    assert dc.case_lds_bound(lib, randqp, monkeypatch, N_CU, dc.LDS_BOUND_SHAPE) == 0


@pytest.mark.parametrize("how", ["box", "primal_ldlt"])
def test_general_kernel(lib, randqp, monkeypatch, how):
    assert dc.case_general(lib, randqp, monkeypatch, N_CU, how) == 0


@pytest.mark.parametrize("n,label", dc.DIAG_ROWS)
def test_diagonal_structure(lib, randqp, monkeypatch, n, label):
    dc.case_diag(lib, randqp, monkeypatch, n, label)


def test_diagonal_structure_of_the_launch(lib, randqp, monkeypatch):
    dc.case_diag_of_the_launch(lib, randqp, monkeypatch, N_CU)


@pytest.mark.parametrize("rows", [257, 513])
def test_wide_classes(lib, randqp, monkeypatch, rows):
    assert dc.case_wide(lib, randqp, monkeypatch, N_CU, rows) == 0


def test_hbm_vectors(lib, randqp, monkeypatch):
    assert dc.case_hbm(lib, randqp, monkeypatch) == 0

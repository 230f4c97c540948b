"""`-m "not gpu"`: the cases of tests/backward_multi_cases.py on the CPU SIMT emulator (tests/emu): the backward pass for K
loss derivatives per QP (pqp_batch_backward_multi), its HBM-vector form, and pqp_batch_backward on a handle whose per-QP
vectors live in HBM."""
import os
import sys

import pytest

import backward_multi_cases as bc
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


@pytest.mark.parametrize("mirror", [False, True])
def test_rows_equal_single_calls(lib, randqp, mirror):
    bc.case_rows_equal_single(lib, randqp, mirror)


def test_full_jacobian(lib, oracle, randqp, monkeypatch):
    bc.case_full_jacobian(lib, oracle, randqp, monkeypatch)


@pytest.mark.slow
@pytest.mark.parametrize("n,ne,ni,B,K,threads", bc.WIDTHS)
def test_every_workgroup_width(lib, randqp, n, ne, ni, B, K, threads):
    bc.case_width(lib, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm(lib, oracle, randqp, monkeypatch):
    bc.case_hbm_forced(lib, oracle, randqp, monkeypatch)


def test_diagonal_structure(lib, randqp):
    bc.case_diag_structure(lib, randqp)


def test_addressing(lib, randqp):
    bc.case_addressing(lib, randqp)


def test_state_left_behind(lib, randqp):
    bc.case_state(lib, randqp)


def test_errors(lib, randqp):
    bc.case_errors(lib, randqp)

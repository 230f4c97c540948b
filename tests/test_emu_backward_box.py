"""`-m "not gpu"`: the cases of tests/backward_box_cases.py on the CPU SIMT emulator (tests/emu): the backward pass of QPs
with box constraints (pqp_batch_backward_box) against the oracle on the row-stated QP, with Ruiz on against an independent
KKT solve, by finite differences, in every form the engine has for box QPs, and its addressing, state and errors."""
import os
import sys

import pytest

import backward_box_cases as bx
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


def test_against_the_oracle_on_the_row_stated_qp(lib, oracle, randqp):
    bx.case_vs_oracle(lib, oracle, randqp)


def test_with_ruiz_on_no_further_from_the_truth_than_the_row_path(lib, oracle, randqp):
    bx.case_ruiz(lib, oracle, randqp)


def test_finite_differences(lib, oracle, randqp):
    bx.case_finite_differences(lib, oracle, randqp)


@pytest.mark.parametrize("name", sorted(bx.FORMS))
def test_forms(lib, oracle, randqp, name):
    bx.case_form(lib, oracle, randqp, name)


@pytest.mark.slow
@pytest.mark.parametrize("n,ne,ni,B,K,threads", bx.WIDTHS)
def test_every_workgroup_width(lib, oracle, randqp, n, ne, ni, B, K, threads):
    bx.case_width(lib, oracle, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm(lib, oracle, randqp, monkeypatch):
    bx.case_hbm_forced(lib, oracle, randqp, monkeypatch)


def test_addressing(lib, oracle, randqp):
    bx.case_addressing(lib, oracle, randqp)


def test_state_left_behind(lib, oracle, randqp):
    bx.case_state(lib, oracle, randqp)


def test_errors(lib, oracle, randqp):
    bx.case_errors(lib, oracle, randqp)


def test_proxqp_dense_api_on_box_qps(lib, oracle, randqp, monkeypatch):
    bx.case_dense_api(lib, oracle, randqp, monkeypatch)

"""`-m gpu`: the cases of tests/backward_multi_cases.py on the MI355X: the backward pass for K loss derivatives per QP
(pqp_batch_backward_multi) in its LDS and HBM-vector forms, pqp_batch_backward on a shape whose per-QP vectors exceed the
LDS of a CU, ROCm tensors in and out, and qplayer.solution_jacobians."""
import pytest

import backward_multi_cases as bc
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.mark.parametrize("mirror", [False, True])
def test_rows_equal_single_calls(lib, randqp, mirror):
    bc.case_rows_equal_single(lib, randqp, mirror)


def test_full_jacobian(lib, oracle, randqp, monkeypatch):
    bc.case_full_jacobian(lib, oracle, randqp, monkeypatch)


@pytest.mark.parametrize("n,ne,ni,B,K,threads", bc.WIDTHS)
def test_every_workgroup_width(lib, randqp, n, ne, ni, B, K, threads):
    bc.case_width(lib, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm_forced(lib, oracle, randqp, monkeypatch):
    bc.case_hbm_forced(lib, oracle, randqp, monkeypatch)


def test_vectors_in_hbm_at_a_shape_that_needs_it(lib, oracle, randqp):
    bc.case_hbm_real_shape(lib, oracle, randqp)


def test_diagonal_structure(lib, randqp):
    bc.case_diag_structure(lib, randqp)


def test_addressing(lib, randqp):
    bc.case_addressing(lib, randqp)


def test_state_left_behind(lib, randqp):
    bc.case_state(lib, randqp)


def test_errors(lib, randqp):
    bc.case_errors(lib, randqp)


def test_rocm_tensors_give_the_same_bits(lib, randqp):
    bc.case_rocm_tensors(lib, randqp)


def test_torch_solution_jacobians(randqp):
    bc.case_torch_helper(randqp)

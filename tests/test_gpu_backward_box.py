"""`-m gpu`: the cases of tests/backward_box_cases.py on the MI355X: the backward pass of QPs with box constraints
(pqp_batch_backward_box) in its LDS and HBM-vector forms and every workgroup width, ROCm tensors in and out, and the
QPFunctionBox layer."""
import pytest

import backward_box_cases as bx
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_against_the_oracle_on_the_row_stated_qp(lib, oracle, randqp):
    bx.case_vs_oracle(lib, oracle, randqp)


def test_with_ruiz_on_no_further_from_the_truth_than_the_row_path(lib, oracle, randqp):
    bx.case_ruiz(lib, oracle, randqp)


def test_finite_differences(lib, oracle, randqp):
    bx.case_finite_differences(lib, oracle, randqp)


@pytest.mark.parametrize("name", sorted(bx.FORMS))
def test_forms(lib, oracle, randqp, name):
    bx.case_form(lib, oracle, randqp, name)


@pytest.mark.parametrize("n,ne,ni,B,K,threads", bx.WIDTHS)
def test_every_workgroup_width(lib, oracle, randqp, n, ne, ni, B, K, threads):
    bx.case_width(lib, oracle, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm_forced(lib, oracle, randqp, monkeypatch):
    bx.case_hbm_forced(lib, oracle, randqp, monkeypatch)


def test_vectors_in_hbm_at_a_shape_that_needs_it(lib, oracle, randqp):
    bx.case_hbm_real_shape(lib, oracle, randqp)


def test_addressing(lib, oracle, randqp):
    bx.case_addressing(lib, oracle, randqp)


def test_state_left_behind(lib, oracle, randqp):
    bx.case_state(lib, oracle, randqp)


def test_errors(lib, oracle, randqp):
    bx.case_errors(lib, oracle, randqp)


def test_proxqp_dense_api_on_box_qps(lib, oracle, randqp, monkeypatch):
    bx.case_dense_api(lib, oracle, randqp, monkeypatch)


def test_rocm_tensors_give_the_same_bits(lib, oracle, randqp):
    bx.case_rocm_tensors(lib, oracle, randqp)


def test_torch_qpfunction_box(oracle, randqp):
    bx.case_torch_layer(oracle, randqp)


def test_torch_qpfunction_box_without_general_inequalities(oracle, randqp):
    bx.case_torch_no_G(oracle, randqp)

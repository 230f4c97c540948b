"""`-m gpu`: the cases of tests/shared_model_cases.py on the MI355X: batches that share a model, with host arrays and
with ROCm tensors as sources and destinations, and the three torch layers on "cuda" tensors."""
import pytest

import shared_model_cases as sm
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    N.load()
    return N


@pytest.mark.parametrize("device", [None, "cuda"], ids=["host", "rocm"])
@pytest.mark.parametrize("shape,mask", sm.ADDRESSING)
def test_broadcast_addressing(native, randqp, shape, mask, device):
    sm.case_addressing(native, randqp, shape, mask, device)


@pytest.mark.parametrize("device", [None, "cuda"], ids=["host", "rocm"])
def test_update_shared(native, randqp, device):
    sm.case_update(native, randqp, device)


def test_update_shared_initialises_a_fresh_qp(native, randqp):
    sm.case_update_of_a_fresh_qp(native, randqp)


def test_errors_and_edge_cases(native, randqp):
    sm.case_errors(native, randqp)


@pytest.mark.parametrize("which", sorted(sm.SUMS))
def test_sum_after_backward(native, randqp, which):
    sm.case_sum(native, randqp, which, "cuda")


def test_sum_after_backward_box(native, randqp):
    sm.case_sum_box(native, randqp, "cuda")


def test_sum_after_backward_closest_feasible(native, randqp):
    sm.case_sum_closest_feasible(native, randqp, "cuda")


def test_multi_init_shared(native, randqp):
    sm.case_multi(native, randqp)


def test_batchqp_init_shared(native, randqp):
    sm.case_batchqp(native, randqp)


@pytest.mark.parametrize("which", sm.LAYERS)
def test_layer_with_shared_matrices(native, randqp, which):
    sm.case_layer(which, randqp, "cuda")


@pytest.mark.parametrize("which", sm.LAYERS)
def test_layer_with_every_parameter_shared(native, randqp, which):
    sm.case_layer_everything_shared(which, randqp, "cuda")


def test_layer_allocates_no_expanded_copy_of_a_shared_matrix(native, randqp):
    sm.case_layer_allocates_no_expanded_copy(randqp)

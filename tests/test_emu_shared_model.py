"""`-m "not gpu"`: the cases of tests/shared_model_cases.py on the CPU SIMT emulator (tests/emu) -- TEST ONLY: the emulator
library is injected in place of libproxqp_hip.so, which the product never does.  Batches that share a model: the broadcast
of pqp_batch_init_shared / pqp_batch_update_shared, the ordered sum of pqp_batch_get_backward_sum, the shards, BatchQP and
the three torch layers on "cpu" tensors."""
import os
import sys

import pytest

import shared_model_cases as sm
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def native():
    import build as emu_build
    saved = N._lib
    N._lib = N.NativeLib(emu_build.build())
    yield N
    N._lib = saved


@pytest.mark.parametrize("shape,mask", sm.ADDRESSING)
def test_broadcast_addressing(native, randqp, shape, mask):
    sm.case_addressing(native, randqp, shape, mask)


def test_update_shared(native, randqp):
    sm.case_update(native, randqp)


def test_update_shared_initialises_a_fresh_qp(native, randqp):
    sm.case_update_of_a_fresh_qp(native, randqp)


def test_errors_and_edge_cases(native, randqp):
    sm.case_errors(native, randqp)


@pytest.mark.parametrize("which", sorted(sm.SUMS))
def test_sum_after_backward(native, randqp, which):
    sm.case_sum(native, randqp, which)


def test_sum_after_backward_box(native, randqp):
    sm.case_sum_box(native, randqp)


def test_sum_after_backward_closest_feasible(native, randqp):
    sm.case_sum_closest_feasible(native, randqp)


def test_multi_init_shared(native, randqp):
    sm.case_multi(native, randqp)


def test_batchqp_init_shared(native, randqp):
    sm.case_batchqp(native, randqp)


@pytest.mark.parametrize("which", sm.LAYERS)
def test_layer_with_shared_matrices(native, randqp, which):
    sm.case_layer(which, randqp)


@pytest.mark.parametrize("which", sm.LAYERS)
def test_layer_with_every_parameter_shared(native, randqp, which):
    sm.case_layer_everything_shared(which, randqp)

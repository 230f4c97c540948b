"""`-m "not gpu"`: the backward pass of the closest-feasible QPLayer (csrc/pqp_infeas.hpp,
pqp_batch_backward_closest_feasible, QPFunction(structural_feasibility=False)) through the CPU SIMT emulator build of the
device code (tests/emu) -- TEST ONLY: the emulator library is injected in place of libproxqp_hip.so, which the product
never does -- and the yardstick of these tests against finite differences (oracle only)."""
import os
import sys

import pytest

import infeas_backward_cases as ic
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def native():
    import build as emu_build
    saved = N._lib
    N._lib = N.NativeLib(emu_build.build())
    yield N
    N._lib = saved


@pytest.mark.parametrize("shape", ic.SHAPES)
def test_layer_backward_matches_the_restatement(native, oracle, shape):
    from proxsuite_amd.torch import QPFunction
    ic.case_layer(QPFunction, oracle, shape)


@pytest.mark.slow
def test_layer_backward_wide_inner_qp(native, oracle):
    from proxsuite_amd.torch import QPFunction
    ic.case_layer(QPFunction, oracle, ic.WIDE_SHAPE, B=2)


@pytest.mark.parametrize("shape", ic.SHAPES)
def test_capi_against_the_restatement(native, oracle, shape):
    ic.case_capi(native, oracle, shape)


@pytest.mark.slow
def test_capi_wide_inner_qp(native, oracle):
    ic.case_capi(native, oracle, ic.WIDE_SHAPE, B=2)


def test_capi_errors(native):
    ic.case_capi_errors(native)


def test_passes_are_bit_identical(native):
    ic.case_passes(native)


def test_range_leaves_the_other_slots_alone(native):
    ic.case_range(native)


def test_shared_parameters_receive_the_batch_sum(native):
    from proxsuite_amd.torch import QPFunction
    ic.case_shared(QPFunction)


def test_object_api(native, oracle):
    """proxqp.dense.compute_backward_closest_feasible fills qp.model.backward_data"""
    import numpy as np
    from proxsuite_amd.proxqp import dense
    n, ne, ns = 10, 3, 6
    q = ic.make_qp(n, ne, ns, 3, infeasible=True)
    G1, h = ic.single_sided(q)
    qp = dense.QP(n, ne, 2 * ns)
    qp.settings.primal_infeasibility_solving = True
    qp.settings.eps_abs = ic.EPS_FORWARD
    qp.init(q["H"], q["g"], q["A"], q["b"], G1, np.full(2 * ns, -1.0e20), h)
    qp.solve()
    ld = ic.random_rows(1, n, ne, 2 * ns)[0]
    sol, flags = dense.compute_backward_closest_feasible(qp, ld, eps=1e-9)
    r = qp.results
    ref = ic.restated_backward(oracle, q["H"], q["A"], G1, h, np.array(r.x), np.array(r.y), np.array(r.z), np.array(r.se),
                               -ld, flags, 1e-9)
    ic.close(sol, ref["solution"], "solution")
    for k in ic.JACOBIANS:
        ic.close(getattr(qp.model.backward_data, k), ref[k], k)


@pytest.mark.parametrize("infeasible", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_yardstick_against_finite_differences(oracle, seed, infeasible):
    ic.case_yardstick_fd(oracle, seed, infeasible)

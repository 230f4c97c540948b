"""`-m gpu`: the backward pass of the closest-feasible QPLayer on the real MI355X library, the cases of
tests/test_emu_infeas_backward.py on ROCm tensors, plus a batch of more than one pass and more than one wave of
workgroups."""
import pytest

import infeas_backward_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from proxsuite_amd import _native as N
    N.load()  # fails loudly if libproxqp_hip.so or the GPU is missing
    return N


@pytest.mark.parametrize("shape", ic.SHAPES + [ic.WIDE_SHAPE])
def test_layer_backward_matches_the_restatement(native, oracle, shape):
    from proxsuite_amd.torch import QPFunction
    ic.case_layer(QPFunction, oracle, shape, device="cuda", B=2 if shape == ic.WIDE_SHAPE else 4)


@pytest.mark.parametrize("shape", ic.SHAPES + [ic.WIDE_SHAPE])
def test_capi_against_the_restatement(native, oracle, shape):
    ic.case_capi(native, oracle, shape, B=2 if shape == ic.WIDE_SHAPE else 4, device="cuda")


def test_capi_host_rows(native, oracle):
    ic.case_capi(native, oracle, (10, 3, 6))


def test_capi_errors(native):
    ic.case_capi_errors(native)


def test_passes_are_bit_identical(native):
    ic.case_passes(native, device="cuda")


def test_range_leaves_the_other_slots_alone(native):
    ic.case_range(native, device="cuda")


def test_shared_parameters_receive_the_batch_sum(native):
    from proxsuite_amd.torch import QPFunction
    ic.case_shared(QPFunction, device="cuda")


def test_many_qps_in_several_passes(native, oracle):
    """B = 64 at (10, 3, 6): more than one wave of workgroups in the assembly kernel, and four passes of 16 whose
    results are those of one pass"""
    import numpy as np
    import torch
    B, shape = 64, (10, 3, 6)
    n, ne, ns = shape
    qps = ic.make_batch(shape, B)
    batch, G1, h = ic.solved_handle(native, qps)
    ld = ic.random_rows(B, n, ne, 2 * ns)
    sol, flags = batch.backward_closest_feasible(torch.as_tensor(ld, device="cuda"), 1e-9)
    one = batch.backward_results(-1)
    sol16, flags16 = batch.backward_closest_feasible(torch.as_tensor(ld, device="cuda"), 1e-9, qps_per_pass=16)
    four = batch.backward_results(-1)
    assert torch.equal(sol, sol16) and torch.equal(flags, flags16)
    for k in ic.JACOBIANS:
        assert np.array_equal(one[k], four[k]), k
    x, y, z, se, _, _ = batch.results()
    sol, flags = sol.cpu().numpy(), flags.cpu().numpy()
    for i in (0, 31, 32, 63):
        q = qps[i]
        ic.check_flags(flags[i], G1[i], h[i], x[i], z[i], n, ne)
        ref = ic.restated_backward(oracle, q["H"], q["A"], G1[i], h[i], x[i], y[i], z[i], se[i], -ld[i], flags[i], 1e-9)
        ic.close(sol[i], ref["solution"], "qp %d solution" % i)
        for k in ic.JACOBIANS:
            ic.close(one[k][i], ref[k], "qp %d %s" % (i, k))
    batch.close()

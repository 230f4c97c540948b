"""`-m gpu`: the cases of tests/eig_cases.py on a real MI355X: the batched minimal-eigenvalue estimate
(pqp_estimate_min_eigenvalues, csrc/pqp_eig.hpp) from host arrays and from ROCm tensors, and the per-QP
manual_minimal_H_eigenvalue of a bulk init / update."""
import numpy as np
import pytest

import eig_cases as ec
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()  # raises loudly when the HIP library or the device is missing


def _rocm(mats):
    import torch
    return torch.as_tensor(np.stack(mats), device="cuda")


@pytest.mark.parametrize("n", ec.EXACT_ORDERS + (ec.EXACT_ORDER_GPU_ONLY,))
def test_exact_every_kind(lib, n):
    ec.case_exact_order(lib, n)


def test_exact_single_matrix(lib):
    ec.case_exact_single(lib)


def test_exact_70_mixed_matrices(lib):
    ec.case_exact_mixed(lib)


def test_exact_70_mixed_matrices_from_a_rocm_tensor(lib):
    import torch
    got, _ = ec.case_exact_mixed(lib, _rocm)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    host, _ = ec.case_exact_mixed(lib)
    assert np.array_equal(got.cpu().numpy(), host)  # the same kernel on the same numbers, staged or read in place


@pytest.mark.parametrize("resident", ["0", "1"])
def test_exact_both_homes_of_the_working_copy(lib, monkeypatch, resident):
    """PQP_EIG_RESIDENT forces the HBM / the LDS working copy at an order where both exist"""
    monkeypatch.setenv("PQP_EIG_RESIDENT", resident)
    ec.case_exact_order(lib, 65)


@pytest.mark.parametrize("accuracy,nb", ec.POWER_SETTINGS)
@pytest.mark.parametrize("n", ec.POWER_ORDERS)
def test_power_iteration_converged(lib, n, accuracy, nb):
    ec.case_power_converged(lib, n, accuracy, nb)


def test_power_iteration_streamed(lib, monkeypatch):
    monkeypatch.setenv("PQP_EIG_RESIDENT", "0")
    ec.case_power_converged(lib, 65, 1e-8, 1000)


def test_power_iteration_cut_short(lib):
    ec.case_power_cut_short(lib)


def test_power_iteration_without_iterations(lib):
    ec.case_power_nb_zero(lib)


def test_power_iteration_degenerate_starts(lib):
    ec.case_power_degenerate(lib)


def test_errors(lib):
    ec.case_errors(lib)


def test_dense_helper_takes_a_batch(lib, monkeypatch):
    ec.case_dense_3d(lib, monkeypatch)
    ec.case_dense_3d(lib, monkeypatch, _rocm)


def test_end_to_end(lib):
    ec.case_end_to_end(lib)

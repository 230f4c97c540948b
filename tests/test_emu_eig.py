"""`-m "not gpu"`: the cases of tests/eig_cases.py on the CPU SIMT emulator (tests/emu): the batched minimal-eigenvalue
estimate (pqp_estimate_min_eigenvalues), the per-QP manual_minimal_H_eigenvalue of a bulk init / update, and the same
through a MultiBatch on two emulated devices."""
import os
import sys

import pytest

import eig_cases as ec
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    os.environ["HIPEMU_DEVICES"] = "4"  # (as tests/test_emu_multi.py: several emulated devices, all of them the host)
    return N.NativeLib(emu_build.build())


@pytest.mark.parametrize("n", ec.EXACT_ORDERS)
def test_exact_every_kind(lib, n):
    ec.case_exact_order(lib, n)


def test_exact_single_matrix(lib):
    ec.case_exact_single(lib)


def test_exact_70_mixed_matrices(lib):
    ec.case_exact_mixed(lib)


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


def test_2d_call_unchanged():
    ec.case_2d_unchanged()


def test_dense_helper_takes_a_batch(lib, monkeypatch):
    ec.case_dense_3d(lib, monkeypatch)


def test_end_to_end(lib):
    ec.case_end_to_end(lib)


def test_end_to_end_multibatch(lib):
    """the bulk handle is a MultiBatch on two emulated devices: the array is sliced along the shards"""
    ec.case_end_to_end(lib, lambda: N.MultiBatch(6, 12, 0, 12, devices=[0, 1], lib=lib))

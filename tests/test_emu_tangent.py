"""`-m "not gpu"`: the cases of tests/tangent_cases.py on the CPU SIMT emulator (tests/emu): forward-mode sensitivities of
solved QPs (pqp_batch_tangent_multi) -- the assembly of the right-hand sides, the K-tangent solve in its LDS and HBM-vector
forms, addressing, state and errors, and dense.compute_forward_sensitivity."""
import os
import sys

import pytest

import tangent_cases as tc
import backward_multi_cases as bc
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


def test_assembly_against_numpy(lib, randqp):
    tc.case_assembly(lib, randqp)


@pytest.mark.parametrize("mirror", [False, True])
def test_solve_against_backward_multi_identity_equilibration(lib, randqp, mirror):
    tc.case_solve_identity(lib, randqp, mirror)


@pytest.mark.parametrize("mirror", [False, True])
def test_equilibrated(lib, randqp, mirror):
    tc.case_equilibrated(lib, randqp, mirror)


@pytest.mark.slow
@pytest.mark.parametrize("n,ne,ni,B,K,threads", bc.WIDTHS)
def test_every_workgroup_width(lib, randqp, n, ne, ni, B, K, threads):
    tc.case_width(lib, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm(lib, randqp, monkeypatch):
    tc.case_hbm_forced(lib, randqp, monkeypatch)


def test_diagonal_structure(lib, randqp):
    tc.case_diag_structure(lib, randqp)


def test_addressing(lib, randqp):
    tc.case_addressing(lib, randqp)


def test_state_left_behind(lib, randqp):
    tc.case_state(lib, randqp)


def test_errors(lib, randqp):
    tc.case_errors(lib, randqp)


def test_dense_compute_forward_sensitivity(lib, randqp, monkeypatch):
    tc.case_dense_facade(lib, randqp, monkeypatch)


def test_torch_solution_tangents_on_host_tensors(lib, randqp, monkeypatch):
    monkeypatch.setattr(N, "_lib", lib)  # (the library `load()` hands out)
    tc.case_torch_helper(lib, randqp, device="cpu")


@pytest.mark.parametrize("shared_matrices", [False, True])
def test_forward_ad_through_qpfunction_on_host_tensors(lib, randqp, monkeypatch, shared_matrices):
    monkeypatch.setattr(N, "_lib", lib)
    tc.case_forward_ad(randqp, shared_matrices, device="cpu")

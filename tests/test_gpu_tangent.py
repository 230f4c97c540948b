"""`-m gpu`: the cases of tests/tangent_cases.py on the MI355X: forward-mode sensitivities of solved QPs
(pqp_batch_tangent_multi) in every kernel instance, ROCm tensors in and out, qplayer.solution_tangents and
torch.autograd.forward_ad through QPFunction."""
import pytest

import tangent_cases as tc
import backward_multi_cases as bc
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_assembly_against_numpy(lib, randqp):
    tc.case_assembly(lib, randqp)


@pytest.mark.parametrize("mirror", [False, True])
def test_solve_against_backward_multi_identity_equilibration(lib, randqp, mirror):
    tc.case_solve_identity(lib, randqp, mirror)


@pytest.mark.parametrize("mirror", [False, True])
def test_equilibrated(lib, randqp, mirror):
    tc.case_equilibrated(lib, randqp, mirror)


@pytest.mark.parametrize("n,ne,ni,B,K,threads", bc.WIDTHS)
def test_every_workgroup_width(lib, randqp, n, ne, ni, B, K, threads):
    tc.case_width(lib, randqp, n, ne, ni, B, K, threads)


def test_vectors_in_hbm_forced(lib, randqp, monkeypatch):
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


def test_rocm_tensors_give_the_same_bits(lib, randqp):
    tc.case_rocm_tensors(lib, randqp)


def test_torch_solution_tangents(lib, randqp):
    tc.case_torch_helper(lib, randqp)


@pytest.mark.parametrize("shared_matrices", [False, True])
def test_forward_ad_through_qpfunction(randqp, shared_matrices):
    tc.case_forward_ad(randqp, shared_matrices)

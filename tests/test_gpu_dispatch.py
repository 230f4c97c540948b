"""`-m gpu`: the dispatch cases of tests/dispatch_cases.py on a real MI355X, the thresholds scaled by the device's CU
count (read from box_calibration).  A row of more than dispatch_cases.MAX_QPS QPs is dropped; the cases print how many
(the emulator file runs every rung, none dropped)."""
import pytest

import dispatch_cases as dc
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()  # raises loudly when the HIP library or the device is missing


@pytest.fixture(scope="module")
def n_cu(lib):
    return N.box_calibration(lib=lib)["n_cu"]


def test_no_kernel_before_the_first_solve(lib):
    b = N.Batch(1, *dc.SHAPE, lib=lib)
    assert b.last_kernel == ""
    b.close()


def test_dense_ladder(lib, randqp, monkeypatch, n_cu):
    print("rows dropped:", dc.case_dense_ladder(lib, randqp, monkeypatch, n_cu))


def test_dense_switches(lib, randqp, monkeypatch, n_cu):
    dc.case_dense_switches(lib, randqp, monkeypatch, n_cu)


def test_lds_bound(lib, randqp, monkeypatch, n_cu):
    print("rows dropped:", dc.case_lds_bound(lib, randqp, monkeypatch, n_cu, dc.LDS_BOUND_SHAPE))


@pytest.mark.parametrize("how", ["box", "primal_ldlt"])
def test_general_kernel(lib, randqp, monkeypatch, n_cu, how):
    print("rows dropped:", dc.case_general(lib, randqp, monkeypatch, n_cu, how))


@pytest.mark.parametrize("n,label", dc.DIAG_ROWS)
def test_diagonal_structure(lib, randqp, monkeypatch, n, label):
    dc.case_diag(lib, randqp, monkeypatch, n, label)


def test_diagonal_structure_of_the_launch(lib, randqp, monkeypatch, n_cu):
    dc.case_diag_of_the_launch(lib, randqp, monkeypatch, n_cu)


@pytest.mark.parametrize("rows", [257, 513])
def test_wide_classes(lib, randqp, monkeypatch, n_cu, rows):
    print("rows dropped:", dc.case_wide(lib, randqp, monkeypatch, n_cu, rows))


def test_hbm_vectors(lib, randqp, monkeypatch):
    print("rows dropped:", dc.case_hbm(lib, randqp, monkeypatch))

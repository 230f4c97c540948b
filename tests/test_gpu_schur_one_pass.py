"""`-m gpu`: the one-pass dual Schur solve / row append of the one-wavefront dense kernel against its two-pass twin on a
real MI355X, equal bits (tests/schur_one_pass_cases.py).  The twin is variants/libproxqp_hip_schur2pass.so: the product's
objects with the kernel's translation unit recompiled under PQP_DW_SCHUR_ONE_PASS=0 (proxsuite_amd/_build.py).  On the
device the sixteen-row reduction runs on the matrix core and the rows travel through buffer loads, which the emulator
replaces: this file is the direct coverage of the form that ships."""
import pytest

import schur_one_pass_cases as sc
from proxsuite_amd import _build
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    path = _build.VARIANT_DIR / "libproxqp_hip_schur2pass.so"
    assert path.exists(), "build the variants first (__graft_entry__.build())"
    return N.load(), N.NativeLib(path)


@pytest.fixture(scope="module")
def stats_lib():
    """the product with the event counters compiled in (n_append, n_delete)"""
    assert _build.HIP_STATS_LIB.exists(), "build the instrumented library first (__graft_entry__.build())"
    return N.NativeLib(_build.HIP_STATS_LIB)


@pytest.mark.parametrize("r", sc.NEVER_EDITED_R)
def test_never_edited_block_of_r_rows(libs, randqp, monkeypatch, r):
    sc.case_equal_bits(*libs, randqp, monkeypatch, 40 if r <= 40 else 128, r, 0, B=2)


@pytest.mark.parametrize("shape", [(33, 8, 40, 6), (100, 50, 100, 8), (128, 60, 128, 4)])
def test_edited_blocks(libs, stats_lib, randqp, monkeypatch, shape):
    """appends, deletions and solves on edited factors; the instrumented build counts them and must agree bit for bit too"""
    n, ne, ni, B = shape
    sc.case_equal_bits(*libs, randqp, monkeypatch, n, ne, ni, B=B, need_edits=True, counters=stats_lib)


def test_block_beyond_128_rows(libs, randqp, monkeypatch):
    """(128, 128, 128): beyond 128 rows both libraries take two passes (NCB = 2); a solve stopped after one outer iteration
    ends there, the whole solve crosses the threshold on its way down"""
    sc.case_equal_bits(*libs, randqp, monkeypatch, 128, 128, 128, B=2, need_r_above=128, max_iter=1)
    sc.case_equal_bits(*libs, randqp, monkeypatch, 128, 128, 128, B=2)

"""`-m gpu`: the primal-block reuse cases of tests/primal_reuse_cases.py on a real MI355X, every kernel family at its
smallest shape.  The cases run on the instrumented twin of the product library (libproxqp_hip_stats.so: the same sources
with the per-phase counters compiled in), whose cyc_factor_h says whether a solve factorised; the re-solve, hand-over
and mixed-launch cases run on the product library as well, where the bit-equality with the PQP_PRIMAL_REUSE=0 twin and
the direct factor gates carry the check alone."""
import pytest

import primal_reuse_cases as pr
from proxsuite_amd import _build
from proxsuite_amd import _native as N

pytestmark = pytest.mark.gpu

RESOLVE_FAMILIES = ["pair", "workgroup", "pair_n17", "workgroup_n17", "workgroup_box", "threads512", "threads1024",
                    "hbm_vectors", "identity_L"]


@pytest.fixture(scope="module")
def lib():
    return N.load()  # raises loudly when the HIP library or the device is missing


@pytest.fixture(scope="module")
def statlib(lib):
    assert _build.HIP_STATS_LIB.exists(), "the instrumented library is missing: __graft_entry__.build() makes it"
    return N.NativeLib(_build.HIP_STATS_LIB)


@pytest.mark.parametrize("family", RESOLVE_FAMILIES)
def test_resolve(statlib, randqp, monkeypatch, family):
    pr.case_resolve(statlib, randqp, monkeypatch, family)


@pytest.mark.parametrize("family", RESOLVE_FAMILIES)
def test_resolve_product_library(lib, randqp, monkeypatch, family):
    pr.case_resolve(lib, randqp, monkeypatch, family, counters=False)


@pytest.mark.parametrize("family", ["pair", "workgroup"])
@pytest.mark.parametrize("guess", pr.ALL_GUESSES)
def test_vector_update(statlib, randqp, monkeypatch, family, guess):
    pr.case_vector_update(statlib, randqp, monkeypatch, family, guess)


@pytest.mark.parametrize("family", ["pair", "workgroup"])
@pytest.mark.parametrize("how", pr.INVALIDATIONS)
def test_invalidation(statlib, randqp, monkeypatch, family, how):
    pr.case_invalidation(statlib, randqp, monkeypatch, family, how)


@pytest.mark.parametrize("family", ["pair", "workgroup"])
def test_settings_that_do_not_invalidate(statlib, randqp, monkeypatch, family):
    pr.case_settings_keep(statlib, randqp, monkeypatch, family)


@pytest.mark.parametrize("first", ["workgroup", "wave"])
def test_hand_over(statlib, lib, randqp, monkeypatch, first):
    pr.case_hand_over(statlib, randqp, monkeypatch, first)
    pr.case_hand_over(lib, randqp, monkeypatch, first, counters=False)


@pytest.mark.parametrize("family", ["pair", "workgroup"])
def test_mixed_launch(statlib, lib, randqp, monkeypatch, family):
    pr.case_mixed_launch(statlib, randqp, monkeypatch, family)
    pr.case_mixed_launch(lib, randqp, monkeypatch, family, counters=False)


def test_primal_ldlt_never_skips(statlib, randqp, monkeypatch):
    pr.case_primal_ldlt_never_skips(statlib, randqp, monkeypatch)

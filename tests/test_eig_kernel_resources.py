"""The kernels of the eigenvalue-estimate family (csrc/pqp_eig.hpp, translation unit 19) against their own frozen record
(tests/golden/eig_kernel_resources_expected.json, written by `python -m proxsuite_amd._build --freeze`), with the rules of
tests/test_kernel_resources.py: no drift beyond compiler noise, no private array in scratch memory.  The solver's record
(tests/golden/kernel_resources_expected.json) names the solver's kernels only."""
import json
import os

import pytest

from proxsuite_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "eig_kernel_resources_expected.json")
TOL = {"VGPRs": 4, "AGPRs": 8, "VGPRs_Spill": 0, "ScratchSize": 0, "SGPRs_Spill": 40, "Occupancy": 0}


def _record():
    _build.build_hip()  # no-op when the library is newer than its sources; the record is that build's
    if not _build.kernel_resources():
        pytest.skip("no kernel-resource record of the product build in build/obj/default (library prebuilt elsewhere)")
    return _build.kernel_resources(auxiliary=True)


def test_both_methods_are_built_and_match_their_frozen_resources():
    rec, exp = _record(), json.load(open(EXPECTED))
    assert sorted(rec) == sorted(exp) == ["pqp_eig_kernel<256,0>", "pqp_eig_kernel<256,1>"]
    drift = ["%s %s: %s -> %s" % (k, f, e[f], rec[k].get(f)) for k, e in exp.items() for f, ab in TOL.items()
             if abs(rec[k].get(f, 0) - e[f]) > ab]
    assert not drift, "register allocation drifted from the frozen record:\n  " + "\n  ".join(drift)


def test_no_spill_and_no_register_array_in_scratch_memory():
    for k, v in _record().items():
        assert v["VGPRs_Spill"] == 0 and v["ScratchSize"] == 0, (k, v)


def test_the_solver_record_holds_no_kernel_of_this_family():
    assert not [k for k in _build.kernel_resources() if "eig" in k]

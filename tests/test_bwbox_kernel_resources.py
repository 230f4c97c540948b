"""The kernels of the box backward family (Solver::backward_box: translation units 23 and 24 of csrc/pqp_kernels.hip) against
their own frozen record (tests/golden/bwbox_kernel_resources_expected.json, written by
`python -m proxsuite_amd._build --freeze`), with the rules of tests/test_kernel_resources.py: no drift beyond compiler
noise, no private array in scratch memory.  The other records name no kernel of this family."""
import json
import os

import pytest

from proxsuite_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "bwbox_kernel_resources_expected.json")
# (as tests/test_kernel_resources.py: absolute, relative)
TOL = {"VGPRs": (4, 0.0), "AGPRs": (8, 0.0), "VGPRs_Spill": (12, 0.05), "ScratchSize": (48, 0.05), "SGPRs_Spill": (40, 0.05),
       "Occupancy": (0, 0.0)}
KERNELS = ["pqp_bwbox_hbm_kernel<1024>", "pqp_bwbox_kernel<1024>", "pqp_bwbox_kernel<256>", "pqp_bwbox_kernel<512>",
           "pqp_bwbox_outer_kernel<256>"]


def _record():
    _build.build_hip()  # no-op when the library is newer than its sources; the record is that build's
    if not _build.kernel_resources():
        pytest.skip("no kernel-resource record of the product build in build/obj/default (library prebuilt elsewhere)")
    return _build.kernel_resources(auxiliary="backward_box")


def test_the_family_is_built_and_matches_its_frozen_resources():
    rec, exp = _record(), json.load(open(EXPECTED))
    assert sorted(rec) == sorted(exp) == KERNELS
    drift = ["%s %s: %s -> %s" % (k, f, e[f], rec[k].get(f)) for k, e in exp.items() for f, (ab, rel) in TOL.items()
             if f in e and abs(rec[k].get(f, 0) - e[f]) > max(ab, rel * abs(e[f]))]
    assert not drift, "register allocation drifted from the frozen record:\n  " + "\n  ".join(drift)


def test_the_outer_product_kernel_neither_spills_nor_uses_scratch():
    v = _record()["pqp_bwbox_outer_kernel<256>"]
    assert v["VGPRs_Spill"] == 0 and v["SGPRs_Spill"] == 0 and v["ScratchSize"] == 0, v


def test_no_register_array_lives_in_scratch_memory():
    bad = {k: (v["ScratchSize"], v["VGPRs_Spill"]) for k, v in _record().items()
           if v.get("ScratchSize", 0) > 4 * v.get("VGPRs_Spill", 0) + 16}
    assert not bad, bad


def test_the_other_records_hold_no_kernel_of_this_family():
    assert not [k for k in _build.kernel_resources() if "bwbox" in k]
    assert not [k for k in _build.kernel_resources(auxiliary=True) if "bwbox" in k]
    for name in _build.NAMED_TUS:
        if name != "backward_box":
            assert not [k for k in _build.kernel_resources(auxiliary=name) if "bwbox" in k], name

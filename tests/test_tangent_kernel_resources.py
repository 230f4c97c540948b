"""The kernels of the forward-mode sensitivities (csrc/pqp_tangent.hpp: translation units 26 and 27 of csrc/pqp_kernels.hip)
against their own frozen record (tests/golden/tangent_kernel_resources_expected.json, written by
`python -m proxsuite_amd._build --freeze`), with the rules of tests/test_kernel_resources.py: no drift beyond compiler
noise.  The assembly kernel is a stream of loads with wavefront reductions: it neither spills nor uses scratch memory.  The
other records name no kernel of this family."""
import json
import os

import pytest

from proxsuite_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "tangent_kernel_resources_expected.json")
# (as tests/test_kernel_resources.py: absolute, relative)
TOL = {"VGPRs": (4, 0.0), "AGPRs": (8, 0.0), "VGPRs_Spill": (12, 0.05), "ScratchSize": (48, 0.05), "SGPRs_Spill": (40, 0.05),
       "Occupancy": (0, 0.0)}
KERNELS = ["pqp_tangent_multi_hbm_kernel<1024>", "pqp_tangent_multi_kernel<1024>", "pqp_tangent_multi_kernel<256>",
           "pqp_tangent_multi_kernel<512>", "pqp_tangent_rhs_kernel<256>"]


def _record():
    _build.build_hip()  # no-op when the library is newer than its sources; the record is that build's
    if not _build.kernel_resources():
        pytest.skip("no kernel-resource record of the product build in build/obj/default (library prebuilt elsewhere)")
    return _build.kernel_resources(auxiliary="tangent")


def test_the_family_is_built_and_matches_its_frozen_resources():
    assert _build.NAMED_TUS["tangent"] == (26, 27)
    rec, exp = _record(), json.load(open(EXPECTED))
    assert sorted(rec) == sorted(exp) == KERNELS
    drift = ["%s %s: %s -> %s" % (k, f, e[f], rec[k].get(f)) for k, e in exp.items() for f, (ab, rel) in TOL.items()
             if f in e and abs(rec[k].get(f, 0) - e[f]) > max(ab, rel * abs(e[f]))]
    assert not drift, "register allocation drifted from the frozen record:\n  " + "\n  ".join(drift)


def test_the_assembly_kernel_neither_spills_nor_uses_scratch():
    v = _record()["pqp_tangent_rhs_kernel<256>"]
    assert v["VGPRs_Spill"] == 0 and v["SGPRs_Spill"] == 0 and v["ScratchSize"] == 0, v


def test_the_other_records_hold_no_kernel_of_this_family():
    mine = lambda rec: [k for k in rec if "tangent" in k]
    assert "tangent" in _build.NAMED_TUS and sorted(mine(json.load(open(EXPECTED)))) == KERNELS  # (the family exists, in its own record)
    assert not mine(_build.kernel_resources())
    assert not mine(_build.kernel_resources(auxiliary=True))
    for name in _build.NAMED_TUS:
        if name != "tangent":
            assert not mine(_build.kernel_resources(auxiliary=name)), name
    golden = os.path.join(ROOT, "tests", "golden")
    for f in os.listdir(golden):
        if f.endswith("kernel_resources_expected.json") and not f.startswith("tangent_"):
            assert not mine(json.load(open(os.path.join(golden, f)))), f

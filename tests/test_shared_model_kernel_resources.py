"""The kernels of the batches that share a model (csrc/pqp_shared.hpp: translation unit 25 of csrc/pqp_kernels.hip) against
their own frozen record (tests/golden/shared_model_kernel_resources_expected.json, written by
`python -m proxsuite_amd._build --freeze`), with the rules of tests/test_kernel_resources.py: no drift beyond compiler
noise.  Both kernels are streams of loads and stores: neither spills nor uses scratch memory.  The other records name no
kernel of this family."""
import json
import os

import pytest

from proxsuite_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "shared_model_kernel_resources_expected.json")
# (as tests/test_kernel_resources.py: absolute, relative)
TOL = {"VGPRs": (4, 0.0), "AGPRs": (8, 0.0), "VGPRs_Spill": (12, 0.05), "ScratchSize": (48, 0.05), "SGPRs_Spill": (40, 0.05),
       "Occupancy": (0, 0.0)}
KERNELS = ["pqp_broadcast_kernel<256>", "pqp_sum_kernel<256>"]


def _record():
    _build.build_hip()  # no-op when the library is newer than its sources; the record is that build's
    if not _build.kernel_resources():
        pytest.skip("no kernel-resource record of the product build in build/obj/default (library prebuilt elsewhere)")
    return _build.kernel_resources(auxiliary="shared_model")


def test_the_family_is_built_and_matches_its_frozen_resources():
    rec, exp = _record(), json.load(open(EXPECTED))
    assert sorted(rec) == sorted(exp) == KERNELS
    drift = ["%s %s: %s -> %s" % (k, f, e[f], rec[k].get(f)) for k, e in exp.items() for f, (ab, rel) in TOL.items()
             if f in e and abs(rec[k].get(f, 0) - e[f]) > max(ab, rel * abs(e[f]))]
    assert not drift, "register allocation drifted from the frozen record:\n  " + "\n  ".join(drift)


@pytest.mark.parametrize("kernel", KERNELS)
def test_neither_kernel_spills_or_uses_scratch(kernel):
    v = _record()[kernel]
    assert v["VGPRs_Spill"] == 0 and v["SGPRs_Spill"] == 0 and v["ScratchSize"] == 0, v


def test_the_other_records_hold_no_kernel_of_this_family():
    mine = lambda rec: [k for k in rec if "broadcast" in k or "pqp_sum" in k]
    assert not mine(_build.kernel_resources())
    assert not mine(_build.kernel_resources(auxiliary=True))
    for name in _build.NAMED_TUS:
        if name != "shared_model":
            assert not mine(_build.kernel_resources(auxiliary=name)), name

"""`-m "not gpu"`: the one-pass dual Schur solve / row append of the one-wavefront dense kernel against its two-pass twin
on the CPU SIMT emulator (tests/emu), equal bits (tests/schur_one_pass_cases.py).  The emulator compiles the same
mat_pass_block with its primitives replaced (PQP_EMULATED_MFMA) and runs one fiber per GPU thread, with barriers that
are real: a row sum read before its reduction has written it is a wrong result here.

Held to well under the two minutes serial of tests/test_emu_factors.py: two QPs per never-edited shape, six for the edited
one; (100, 50, 100), (128, 60, 128) and the block beyond 128 rows run on the device only
(tests/test_gpu_schur_one_pass.py)."""
import os
import sys

import pytest

import schur_one_pass_cases as sc
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


@pytest.fixture(scope="module")
def libs():
    import build as emu_build
    return N.NativeLib(emu_build.build()), N.NativeLib(emu_build.build_variant("schur2pass", ["PQP_DW_SCHUR_ONE_PASS=0"]))


@pytest.mark.parametrize("r", sc.NEVER_EDITED_R)
def test_never_edited_block_of_r_rows(libs, randqp, monkeypatch, r):
    sc.case_equal_bits(*libs, randqp, monkeypatch, 40 if r <= 40 else 128, r, 0, B=2)


def test_edited_blocks(libs, randqp, monkeypatch):
    """appends, deletions and solves on edited factors (the emulator library counts them)"""
    sc.case_equal_bits(*libs, randqp, monkeypatch, 33, 8, 40, B=6, need_edits=True, counters=libs[0])

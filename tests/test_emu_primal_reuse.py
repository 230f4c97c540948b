"""`-m "not gpu"`: the primal-block reuse cases of tests/primal_reuse_cases.py on the CPU SIMT emulator (tests/emu), whose
library compiles the per-phase counters in: every case reads whether the factorisation ran.  The emulator proves the state
machine -- who sets, keeps and clears State::primal_valid, what a skipping solve restores into LDS, the bit-equality with
the twin -- on the same sources; tests/test_gpu_primal_reuse.py runs the cases on the device, the 1024-thread kernel
included (no 1024-thread shape fits the emulator's time budget, as in tests/test_emu_factors.py)."""
import os
import sys

import pytest

import primal_reuse_cases as pr
from proxsuite_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


def emu_B(family):
    """the emulator runs one fiber per GPU thread: the one-wavefront pair, forced by PQP_DENSE_KERNEL=wave, gets 4 QPs here
    (its kernels do not depend on the launch size; the device file gives it the 64 its dispatch asks for)"""
    return 4 if family.startswith("pair") else (1 if family == "threads512" else None)


@pytest.fixture(scope="module")
def lib():
    import build as emu_build
    return N.NativeLib(emu_build.build())


@pytest.mark.parametrize("family", ["pair", "workgroup", "pair_n17", "workgroup_n17", "workgroup_box", "threads512",
                                    "hbm_vectors", "identity_L"])
def test_resolve(lib, randqp, monkeypatch, family):
    pr.case_resolve(lib, randqp, monkeypatch, family, B=emu_B(family))


@pytest.mark.parametrize("family", ["pair", "workgroup"])
@pytest.mark.parametrize("guess", pr.ALL_GUESSES)
def test_vector_update(lib, randqp, monkeypatch, family, guess):
    pr.case_vector_update(lib, randqp, monkeypatch, family, guess, B=emu_B(family))


@pytest.mark.parametrize("family", ["pair", "workgroup"])
@pytest.mark.parametrize("how", pr.INVALIDATIONS)
def test_invalidation(lib, randqp, monkeypatch, family, how):
    pr.case_invalidation(lib, randqp, monkeypatch, family, how, B=emu_B(family))


@pytest.mark.parametrize("family", ["pair", "workgroup"])
def test_settings_that_do_not_invalidate(lib, randqp, monkeypatch, family):
    pr.case_settings_keep(lib, randqp, monkeypatch, family, B=emu_B(family))


@pytest.mark.parametrize("first", ["workgroup", "wave"])
def test_hand_over(lib, randqp, monkeypatch, first):
    pr.case_hand_over(lib, randqp, monkeypatch, first, B=4)


@pytest.mark.parametrize("family", ["pair", "workgroup"])
def test_mixed_launch(lib, randqp, monkeypatch, family):
    pr.case_mixed_launch(lib, randqp, monkeypatch, family, B=emu_B(family))


def test_primal_ldlt_never_skips(lib, randqp, monkeypatch):
    pr.case_primal_ldlt_never_skips(lib, randqp, monkeypatch)

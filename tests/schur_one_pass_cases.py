"""One read of W_S per dual Schur solve and per row append in the one-wavefront dense kernel (mat_pass_block's SELF mode,
proxsuite_amd/csrc/pqp_dwave.hpp) -- shared by tests/test_emu_schur_one_pass.py and tests/test_gpu_schur_one_pass.py, as
factor_cases.py is shared by the factor tests.

The comparator is the TWO-PASS TWIN: the same sources compiled with PQP_DW_SCHUR_ONE_PASS=0, where the row sums, the
division by D_S and the column sums are three steps with W_S read twice, as before the switch existed.  The one-pass
form takes the same row sums through the same reduction, divides by the same expression in the same lanes and feeds
every column the same FMA chain (items ascending, even items in one accumulator, odd items in the other): the two
libraries must leave EQUAL BITS in x, y, z, se, si, in every Info field but the three timers, and in the Schur factor
(W_S, D_S, the slot list and its metadata, mu).  No tolerance anywhere.

Shapes: blocks that are never edited (n_in = 0, r = n_eq) at the edges of the sixteen-row groups, and QPs whose active
sets move, so that appends, deletions and solves on edited factors are all in the comparison -- a case of that kind
asserts that an append and a deletion did happen."""
import numpy as np

import factor_cases as fc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import DenseBackend, pqp_info

TIMERS = ("setup_time", "solve_time", "run_time")
INFO_FIELDS = tuple(n for n, _ in pqp_info._fields_ if n not in TIMERS and n != "_pad")
N_APPEND, N_DELETE = N.STAT_NAMES.index("n_append"), N.STAT_NAMES.index("n_delete")

# never-edited blocks of r rows: one row; around the sixteen-row group (a partial group, one whole group, one row into
# the next); three groups with a partial last one; the full register block.  (n = 40 up to r = 40, 128 above: see
# tests/test_emu_factors.py::test_schur_block_of_r_rows)
NEVER_EDITED_R = (1, 15, 16, 17, 33, 128)


def bits(a):
    """a float array as the integers its bits spell: NaNs compare by payload, -0.0 differs from 0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def snapshot(b, B, ne):
    """everything the comparison covers, copied off the batch"""
    x, y, z, se, si, info = b.results()
    snap = dict(x=x, y=y, z=z, se=se, si=si)
    snap["info"] = [tuple(getattr(info[q], f) for f in INFO_FIELDS) for q in range(B)]
    snap["schur"] = []
    for q in range(B):
        WS, dS, G, slots, meta, mus = b.schur_factor(q)
        r = ne + meta["n_slots"]  # (rows of the block: what lies beyond them in W_S and D_S is scratch)
        snap["schur"].append(dict(WS=WS[:r, :r].copy(), dS=dS[:r].copy(), slots=slots.copy(), meta=meta, mus=mus.copy()))
    return snap


def assert_equal_bits(a, t, what):
    for name in ("x", "y", "z", "se", "si"):
        assert np.array_equal(bits(a[name]), bits(t[name])), (what, name, float(np.max(np.abs(a[name] - t[name]))))
    for q, (ia, it) in enumerate(zip(a["info"], t["info"])):
        for f, u, v in zip(INFO_FIELDS, ia, it):
            same = np.array_equal(bits([u]), bits([v])) if isinstance(u, float) else u == v
            assert same, (what, "Info.%s" % f, q, u, v)
    for q, (sa, st) in enumerate(zip(a["schur"], t["schur"])):
        assert sa["meta"] == st["meta"], (what, "Schur meta", q, sa["meta"], st["meta"])
        assert np.array_equal(sa["slots"], st["slots"]), (what, "slots", q)
        for name in ("WS", "dS", "mus"):
            assert np.array_equal(bits(sa[name]), bits(st[name])), (what, name, q)


def solve(lib, randqp, monkeypatch, n, ne, ni, B, seed0, max_iter=None):
    monkeypatch.setenv("PQP_DENSE_KERNEL", "wave")
    b = fc.solve_batch(lib, randqp, B, n, ne, ni, backend=int(DenseBackend.PrimalDualLDLT), seed0=seed0, max_iter=max_iter)
    fc.assert_kernel(b, pair=True)
    return b


def case_equal_bits(lib, twin, randqp, monkeypatch, n, ne, ni, B, need_edits=False, need_r_above=None, counters=None,
                    seed0=0, max_iter=None):
    """the same seeded batch through the product library and through the two-pass twin, PQP_DENSE_KERNEL=wave.
    `need_edits`: some QP's factor has been edited when the solve ends (ls_edited), and -- `counters`: a library with the
    event counters compiled in, given the same batch -- rows were appended and rows were deleted.
    `need_r_above`: some QP ends on a block of more rows than that (the two-pass code in both libraries); `max_iter`
    stops the solve after so many outer iterations (the active set is largest early in a solve)."""
    what = "(%d,%d,%d) B=%d%s" % (n, ne, ni, B, "" if max_iter is None else " max_iter=%d" % max_iter)
    snaps, st = [], None
    for l in (lib, twin) + (() if counters in (None, lib) else (counters,)):
        b = solve(l, randqp, monkeypatch, n, ne, ni, B, seed0, max_iter)
        snaps.append(snapshot(b, B, ne))
        if l is counters:
            st = b.stats()
        b.close()
    a, t = snaps[:2]
    assert all(np.all(np.isfinite(a[k])) for k in ("x", "y", "z")), (what, "non-finite result")
    assert_equal_bits(a, t, what)
    if len(snaps) == 3:  # (the instrumented build runs the same arithmetic)
        assert_equal_bits(a, snaps[2], what + " instrumented")
    metas = [s["meta"] for s in a["schur"]]
    if ni == 0:
        assert all(m["n_slots"] == 0 and not m["ls_edited"] for m in metas), (what, metas)
    if need_edits:
        assert any(m["ls_edited"] for m in metas), (what, "no QP ended on an edited factor", metas)
        if st is not None:
            print("%s: appends per QP %s, deletions per QP %s" % (what, st[:, N_APPEND].tolist(), st[:, N_DELETE].tolist()))
            assert np.any(st[:, N_APPEND] > 0), (what, "no row was appended", st[:, N_APPEND])
            assert np.any(st[:, N_DELETE] > 0), (what, "no row was deleted", st[:, N_DELETE])
    if need_r_above is not None:
        r_max = max(ne + m["n_slots"] for m in metas)
        assert r_max > need_r_above, (what, r_max, "no QP ended on a Schur block beyond %d rows" % need_r_above)

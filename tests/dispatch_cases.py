"""Which kernel a solve launch runs on -- pqp_plan_solve (csrc/pqp_kernels.hip), read back through Batch.last_kernel --
shared by tests/test_emu_dispatch.py and tests/test_gpu_dispatch.py, as factor_cases.py is shared by the factor tests.

Every case pins the label of one rung of the rule: the 256-thread budget ladder (one, two, three, four workgroups per
CU), the round arithmetic of the one-wavefront dense pair, the two environment switches, the LDS condition of the
four-per-CU build, the general kernel, the diagonal-structure kernels (by dimension, and by the QPs OF THE LAUNCH), the
512- and 1024-thread classes and the HBM-vector kernel.  The thresholds are multiples of the device's CU count `n_cu`:
1 on the emulated device, where the counts below are a handful of QPs; the device runner scales them.

The expected labels are the rule as it stood BEFORE it was gathered into pqp_plan_solve (confirmed then on a build that
printed the instantiation from every launcher).  Results are only checked for status == 0: accuracy is the other
suites' job."""
import numpy as np

import factor_cases as fc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import DenseBackend, HessianType, InitialGuess

DENSE, DIAG = int(HessianType.Dense), int(HessianType.Diagonal)
SHAPE = (6, 2, 3)  # (n, n_eq, n_in) unless a case says otherwise
MODELS = 8         # distinct generator QPs per batch (tiled: the dispatch does not look at the data)
MAX_QPS = 4096     # a device case of more QPs than this is dropped (and counted)

LDS_BOUND_SHAPE = (6, 2, 250)  # 256 threads, 43032 bytes of LDS: four of them exceed the 160 KiB of a CU
DIAG_ROWS = [(6, "pqp_diag_kernel<1,2>"), (100, "pqp_diag_kernel<2,2>"), (200, "pqp_diag_kernel<4,2>")]

S1 = "pqp_solve_kernel<256,%d,1>"
PAIR = "pqp_dwave_kernel<2>"


def dense_ladder(n_cu):
    """(count, label) of solve_range(0, count) on dense QPs without box, PrimalDualLDLT.  The one-wavefront pair keeps
    8 QPs per CU resident (a round); it takes launches of at least 64 QPs from 0.6 of a round, and beyond a round those
    whose last round is empty or at least 0.4 full."""
    if n_cu == 1:
        return [(1, S1 % 1), (2, S1 % 2), (3, S1 % 3), (4, S1 % 4), (63, S1 % 4), (64, PAIR), (65, S1 % 4), (67, S1 % 4),
                (68, PAIR)]
    assert n_cu >= 16, n_cu  # (below, 0.6 of a round falls under the 64 QPs or into the ladder)
    rnd = 8 * n_cu
    first, last = -(-3 * rnd // 5), -(-2 * rnd // 5)  # smallest counts with 5 c >= 3 round, 5 c >= 2 round
    return [(n_cu, S1 % 1), (n_cu + 1, S1 % 2), (2 * n_cu, S1 % 2), (2 * n_cu + 1, S1 % 3), (3 * n_cu, S1 % 3),
            (3 * n_cu + 1, S1 % 4), (first - 1, S1 % 4), (first, PAIR), (rnd, PAIR), (rnd + 1, S1 % 4),
            (rnd + last - 1, S1 % 4), (rnd + last, PAIR)]


def make_batch(lib, randqp, B, n, ne, ni, box=False, hessian=DENSE, backend=int(DenseBackend.PrimalDualLDLT), C=None):
    """B generator QPs (MODELS distinct ones, tiled), `box`: inside a box that leaves them feasible.  A diagonal Hessian comes with n_eq = 0 and C = a positive diagonal
    (`C`: another one), bounds -1 .. 1: the diagonal-structure signature, strongly convex and bounded."""
    G = min(B, MODELS)
    tile = lambda a: None if a is None else np.ascontiguousarray(np.concatenate([a] * (-(-B // G)))[:B])
    kw = {}
    if hessian == DIAG:
        assert ne == 0 and ni == n and not box
        k = np.arange(n)
        H = np.stack([np.diag(1.0 + 0.1 * ((k + s) % 7)) for s in range(G)])
        g = np.stack([np.cos(k + s) for s in range(G)])
        Cm = np.stack([np.diag(1.0 + 0.05 * (k % 5))] * G) if C is None else C
        mats = (H, g, None, None, Cm, -np.ones((G, n)), np.ones((G, n)))
    else:
        m, H, _ = fc.make_models(randqp, G, n, ne, ni, False, hessian, False)
        if box:  # (wide: the generator's feasible point lies inside)
            kw = dict(l_box=np.full((G, n), -100.0), u_box=np.full((G, n), 100.0))
        mats = (H, m.g, m.A if ne else None, m.b if ne else None, m.C if ni else None, m.l if ni else None,
                m.u if ni else None)
    b = N.Batch(B, n, ne, ni, box_constraints=box, hessian_type=hessian, dense_backend=backend, lib=lib)
    b.set_all_settings(eps_abs=1e-9, eps_rel=0, initial_guess=int(InitialGuess.NO_INITIAL_GUESS))
    b.init(-1, *map(tile, mats), **{k: tile(v) for k, v in kw.items()})
    return b


def check_launch(b, label, solved, what=""):
    """the launch that just ran: its label, its two times, the status of the QPs it solved"""
    k, ms, pro = b.last_kernel, b.last_solve_ms, b.last_prologue_ms
    print("%-40s %-32s %8.3f ms  prologue %.3f ms" % (what, k, ms, pro))
    assert k == label, (what, k, label)
    assert ms > 0, (what, ms)
    if k.startswith("pqp_dwave_kernel<"):
        assert 0 < pro < ms, (what, pro, ms)
    else:
        assert pro == 0, (what, pro)
    info = b.infos()
    bad = [(q, info[q].status) for q in solved if info[q].status != 0]
    assert not bad, (what, bad[:8])


def check_whole_batch(b, what="", solve=True):
    """launch_config() is the plan of a whole-batch launch: solve() (`solve=False`: the launch that just ran, which
    covered the batch) runs on a kernel of that many threads, and the forecast is the same before and after"""
    cfg = b.launch_config()
    if solve:
        b.solve()
    k = b.last_kernel
    assert fc.kernel_threads(k) == cfg[0] and cfg[1] > 0 and b.launch_config() == cfg, (what, k, cfg, b.launch_config())
    assert (b.last_prologue_ms > 0) == k.startswith("pqp_dwave_kernel<"), (what, k, b.last_prologue_ms)
    return k


def case_ranges(lib, randqp, rows, n=SHAPE[0], ne=SHAPE[1], ni=SHAPE[2], what="", **kw):
    """solve_range(0, count) for every (count, label) of `rows`, in ascending order, on ONE batch of as many QPs as the
    last row -- which is therefore a launch of the whole batch, what launch_config() forecasts.  Returns how many rows
    were dropped for size."""
    keep = [(c, k) for c, k in rows if c <= MAX_QPS]
    assert keep == sorted(keep), keep
    b = make_batch(lib, randqp, keep[-1][0], n, ne, ni, **kw)
    for count, label in keep:
        b.solve(0, count)
        check_launch(b, label, range(count), "%s solve_range(0, %d)" % (what, count))
    check_whole_batch(b, what, solve=False)
    b.close()
    if len(keep) < len(rows):
        print("%s: %d of %d rows dropped (more than %d QPs)" % (what, len(rows) - len(keep), len(rows), MAX_QPS))
    return len(rows) - len(keep)


def case_dense_ladder(lib, randqp, monkeypatch, n_cu):
    monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False)
    return case_ranges(lib, randqp, dense_ladder(n_cu), what="dense")


def case_dense_switches(lib, randqp, monkeypatch, n_cu):
    """PQP_DENSE_KERNEL, read per launch: the smallest launch the pair takes by itself sent to the workgroup kernel, one
    QP sent to the pair"""
    count = next(c for c, k in dense_ladder(n_cu) if k == PAIR)
    b = make_batch(lib, randqp, count, *SHAPE)
    for env, cnt, label in (("workgroup", count, S1 % 4), ("wave", 1, PAIR), (None, count, PAIR)):
        monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False) if env is None else monkeypatch.setenv("PQP_DENSE_KERNEL", env)
        b.solve(0, cnt)
        check_launch(b, label, range(cnt), "PQP_DENSE_KERNEL=%s solve_range(0, %d)" % (env, cnt))
    b.close()


def case_lds_bound(lib, randqp, monkeypatch, n_cu, shape):
    """four workgroups of `shape` do not fit the 160 KiB of a CU: the launch that would take the four-per-CU build runs
    the three-per-CU one"""
    monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False)
    probe = N.Batch(1, *shape, lib=lib)
    cfg = probe.launch_config()
    probe.close()
    assert cfg[0] == 256 and cfg[1] > 40960, (shape, cfg)
    return case_ranges(lib, randqp, [(3 * n_cu + 1, S1 % 3)], *shape, what="LDS %d B" % cfg[1])


def case_general(lib, randqp, monkeypatch, n_cu, how):
    """box constraints or PrimalLDLT: the general kernel, one workgroup per CU or three"""
    kw = dict(box=True) if how == "box" else dict(backend=int(DenseBackend.PrimalLDLT))
    rows = [(n_cu, "pqp_solve_kernel<256,1,0>"), (n_cu + 1, "pqp_solve_kernel<256,3,0>")]
    return case_ranges(lib, randqp, rows, what=how, **kw)


def case_diag(lib, randqp, monkeypatch, n, label):
    """diagonal Hessian, n_eq = 0, C diagonal, n_in = n: the one-wavefront kernel with 1, 2 or 4 register slots per vector
    by dimension; PQP_DIAG_KERNEL=workgroup: the 256-thread form"""
    monkeypatch.delenv("PQP_DIAG_KERNEL", raising=False)
    b = make_batch(lib, randqp, 2, n, 0, n, hessian=DIAG)
    b.solve()
    check_launch(b, label, range(2), "diagonal n=%d" % n)
    assert b.launch_config()[0] == 64
    assert check_whole_batch(b) == label
    monkeypatch.setenv("PQP_DIAG_KERNEL", "workgroup")
    b.solve()
    check_launch(b, "pqp_solve_kernel<256,2,2>", range(2), "diagonal n=%d, PQP_DIAG_KERNEL=workgroup" % n)
    assert b.launch_config()[0] == 256
    b.close()


def case_diag_of_the_launch(lib, randqp, monkeypatch, n_cu):
    """four QPs of the diagonal signature, QP 0 with a full C: a launch of the structured three runs the one-wavefront
    kernel, a launch of all four the general one -- and launch_config() forecasts the whole batch both times"""
    monkeypatch.delenv("PQP_DIAG_KERNEL", raising=False)
    n = SHAPE[0]
    Cm = np.stack([np.diag(1.0 + 0.05 * np.arange(n))] * 4)
    Cm[0] += 0.1 * np.cos(np.arange(n * n)).reshape(n, n)
    b = make_batch(lib, randqp, 4, n, 0, n, hessian=DIAG, C=Cm)
    general = "pqp_solve_kernel<256,%d,0>" % (1 if 4 <= n_cu else 3)
    b.solve_subset([1, 2, 3])
    check_launch(b, "pqp_diag_kernel<1,2>", [1, 2, 3], "solve_subset([1, 2, 3])")
    cfg = b.launch_config()
    assert cfg[0] == 256, cfg
    b.solve(1, 3)
    check_launch(b, "pqp_diag_kernel<1,2>", [1, 2, 3], "solve_range(1, 3)")
    b.solve()
    check_launch(b, general, range(4), "solve()")
    assert b.launch_config() == cfg, (b.launch_config(), cfg)
    b.close()


def case_wide(lib, randqp, monkeypatch, n_cu, rows_of_constraints):
    """the smallest shapes of the 512- and 1024-thread classes (257 / 513 constraint rows)"""
    n, ne = SHAPE[0], SHAPE[1]
    ni = rows_of_constraints - ne
    probe = N.Batch(1, n, ne, ni, lib=lib)
    threads, lds = probe.launch_config()
    probe.close()
    if rows_of_constraints <= 512:
        assert threads == 512
        # (the 128-VGPR build only when it buys a second resident workgroup: more QPs than CUs, two LDS layouts per CU)
        second = "pqp_solve_kernel<512,4,1>" if 2 * lds <= 160 * 1024 else "pqp_solve_kernel<512,2,1>"
        rows = [(n_cu, "pqp_solve_kernel<512,2,1>"), (n_cu + 1, second)]
    else:
        assert threads == 1024
        rows = [(1, "pqp_solve_kernel<1024,4,1>")]
    return case_ranges(lib, randqp, rows, n, ne, ni, what="%d rows" % rows_of_constraints)


def case_hbm(lib, randqp, monkeypatch):
    """PQP_FORCE_HBM_VECTORS=1 (read when the batch is created): a small shape through the kernel of the shapes whose
    vectors outgrow the LDS"""
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    return case_ranges(lib, randqp, [(2, "pqp_solve_hbm_kernel<1024,4,1>")], what="HBM vectors")

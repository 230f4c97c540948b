"""`-m gpu`: parity of the HIP path on a real MI355X, through the C-ABI of
include/proxqp_hip.h (proxsuite_amd/csrc/libproxqp_hip.so), against the CPU oracle on the same
seeded inputs, the committed golden fixtures, and -- at BASELINE.json's full sizes -- through
size-independent properties (KKT residuals on the unscaled model, run-to-run determinism)."""
import os
import sys

import numpy as np
import pytest

import parity_cases as pc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import HessianType, InitialGuess

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return N.load()  # raises loudly when the HIP library or the device is missing


def test_library_exports_every_declared_symbol(lib):
    for name in N.NativeLib.SYMBOLS:
        assert hasattr(lib.L, name), name
    assert lib.path.endswith("libproxqp_hip.so")


def test_known_answers(lib):
    pc.case_known_answers(lib)


def test_ruiz(lib, oracle, randqp):
    pc.case_ruiz(lib, oracle, randqp)
    pc.case_ruiz(lib, oracle, randqp, 100, 50, 100)


@pytest.mark.parametrize("shape", [(10, 2, 3, 32), (30, 7, 9, 32), (50, 25, 50, 128), (100, 50, 100, 64),
                                   (60, 0, 20, 16), (60, 20, 0, 16), (200, 30, 56, 8),
                                   (33, 8, 11, 16), (101, 49, 99, 16), (1, 0, 1, 4)])  # odd n: 8-byte-load path of gemv_dual
def test_random_batch(lib, oracle, randqp, shape):
    n, ne, ni, B = shape
    pc.case_random_batch(lib, oracle, randqp, n, ne, ni, B=B)


@pytest.mark.parametrize("shape", [(120, 100, 100, 8), (40, 5, 300, 8), (130, 10, 20, 8), (300, 40, 120, 4)])
def test_matrix_core_fallback_paths(lib, oracle, randqp, shape):
    """shapes beyond the register-resident factorisations (ldlt_factor_mfma, tri_inverse_mfma_rows):
    Schur block > 112 rows, 512- and 1024-thread workgroups, primal block > 112 columns."""
    n, ne, ni, B = shape
    pc.case_random_batch(lib, oracle, randqp, n, ne, ni, B=B)


@pytest.mark.parametrize("shape", [(10, 4, 7, 16), (12, 0, 9, 8), (9, 5, 0, 8), (100, 50, 100, 32)])
def test_backward(lib, oracle, randqp, shape):
    n, ne, ni, B = shape
    pc.case_backward(lib, oracle, randqp, n, ne, ni, B=B)


def test_equality_constrained_initial_guess_batch(lib, oracle, randqp):
    pc.case_random_batch(lib, oracle, randqp, 100, 50, 100, B=32,
                         guess=InitialGuess.EQUALITY_CONSTRAINED_INITIAL_GUESS)


@pytest.mark.parametrize("guess", list(InitialGuess))
def test_state_machine(lib, oracle, randqp, guess):
    pc.case_state_machine(lib, oracle, randqp, guess)


@pytest.mark.parametrize("hessian", [HessianType.Dense, HessianType.Diagonal])
def test_box_constraints(lib, oracle, randqp, hessian):
    pc.case_box_constraints(lib, oracle, randqp, seeds=100, hessian=hessian)


@pytest.mark.parametrize("dim", [10, 60, 110])
def test_families(lib, oracle, randqp, dim):
    pc.case_families(lib, oracle, randqp, dim)


def test_maros_meszaros_small(lib):
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maros_meszaros_small.npz")
    d = np.load(gold)
    for name in [str(s) for s in d["names"]]:
        pc.case_maros_meszaros(lib, *(d["%s/%s" % (name, k)] for k in "PqAlu"))


def test_maros_meszaros_small_path(lib, oracle):
    """the same 33 problems, iteration by iteration against the oracle (settings.verbose trace): 27 walk the oracle's
    path line for line; QADLITTL, QAFIRO, QISRAEL, QPCBOEI2, QSCAGR7, QSHARE2B (ill-conditioned LP-like problems, see
    the case) leave it and end SOLVED within a few iterations of it"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maros_meszaros_small.npz"))
    probs = {str(name): tuple(d["%s/%s" % (name, k)] for k in "PqAlu") for name in d["names"]}
    same, forks = pc.case_maros_meszaros_path(lib, oracle, probs)
    print("same path:", len(same), "forks:", forks)
    assert len(same) + len(forks) == len(probs) and len(same) >= 24, (len(same), forks)


def _medium_names():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maros_meszaros_medium.npz"))
    return [str(s) for s in d["names"]]


@pytest.mark.parametrize("name", _medium_names())
def test_maros_meszaros_medium(lib, name):
    """the other 29 problems of reference test/src/dense_maros_meszaros.cpp:97 (n up to 760, up to 856
    constraint rows): the 512- and 1024-thread kernels on ill-conditioned real-world data"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_maros_meszaros_fixtures as mm
    pc.case_maros_meszaros(lib, *mm.load_medium(only=name)[name])


def test_errors(lib):
    pc.case_errors(lib)


def test_determinism(lib, randqp):
    pc.case_determinism(lib, randqp, 100, 50, 100, B=64)


@pytest.mark.parametrize("shape", [(100, 50, 100, 1024, 256, False), (100, 50, 100, 1024, 512, False),
                                   (100, 50, 100, 1024, 768, False),
                                   (40, 5, 300, 320, 64, False), (100, 200, 200, 320, 64, True)])
def test_launch_size_invariance(lib, randqp, shape, monkeypatch):
    """(The dense shapes on the 256-thread WORKGROUP kernels, PQP_DENSE_KERNEL=workgroup: by default a device-filling launch
    of this signature goes to the one-wavefront kernel, which sums in another order -- test_launch_size_wave_vs_workgroup.)
    1024 QPs in one launch (four workgroups per CU, pqp_solve_kernel<256,4,1>) against the same QPs in
    launches of 256 (a CU per QP: <256,1,1>, the whole register file), of 512 (two per CU: <256,2,1>) and of 768
    (<256,3,1>); 320 QPs of two
    512-thread shapes in one launch (<512,4,.>) against launches of 64 (<512,2,.>), the boxed one on the PrimalLDLT
    engine: bit-identical."""
    n, ne, ni, B, chunk, box = shape
    monkeypatch.setenv("PQP_DENSE_KERNEL", "workgroup")
    pc.case_launch_size_invariance(lib, randqp, n, ne, ni, B, chunk, box=box)


@pytest.mark.parametrize("chunk", [256, 768])
def test_launch_size_wave_vs_workgroup(lib, randqp, chunk, monkeypatch):
    """The default dispatch: 2048 C2-shaped QPs in one launch take the one-wavefront kernel (csrc/pqp_dwave.hpp behind the
    factorisation prologue), the same QPs in launches of 256 / 768 a 256-thread workgroup kernel.  Same algorithm and
    decisions, sums in another order: every Info counter equal, (x, y, z) equal to 1e-10 (1 + |.|)."""
    monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False)
    pc.case_launch_size_invariance(lib, randqp, 100, 50, 100, 2048, chunk, exact=False)


@pytest.mark.parametrize("shape", [(1500, 300, 600), (60, 10, 1500), (40, 0, 2100)])
def test_rows_above_1024(lib, oracle, randqp, shape):
    """More rows than the widest workgroup has threads (reference dense/model.hpp:65-68 has no size limit): 1500
    variables with 900 constraint rows; 1510 and 2100 constraint rows on a few variables (3000 / 4200 line-search
    breakpoints on 1024 threads).  The 1024-thread kernel walks its one-thread-per-row stages in chunks; every QP
    against the oracle (1e-10, equal Info counters) like any other shape."""
    n, ne, ni = shape
    pc.case_random_batch(lib, oracle, randqp, n, ne, ni, B=2, compare="all", info_residuals=False)


@pytest.mark.parametrize("name", ["GOULDQP2", "CVXQP2_M"])
def test_maros_meszaros_above_1024_rows(lib, name):
    """Maros-Meszaros problems with 1048 and 1250 constraint rows (beyond the reference test's own 1000-row cut),
    to the reference test's acceptance lines"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_maros_meszaros_fixtures as mm
    pc.case_maros_meszaros(lib, *mm.load_medium(mm.OUT_LARGE, only=name)[name])


@pytest.mark.parametrize("shape", [(6, 0, 4500), (5, 1, 7000)])
def test_rows_above_4096(lib, oracle, randqp, shape):
    """4500 and 7000 constraint rows on a few variables (9000 / 14 000 line-search breakpoints on 1024 threads, per-QP vectors in
    HBM): round 4 stopped at 4096 rows, the reference has no limit (dense/model.hpp:65-68).  Against the oracle like any shape."""
    n, ne, ni = shape
    pc.case_random_batch(lib, oracle, randqp, n, ne, ni, B=2, compare="all", info_residuals=False)


def test_size_limit_is_reported(lib):
    """beyond 8192 rows the library says so instead of computing garbage"""
    with pytest.raises(N.NativeError):
        N.Batch(1, 10, 0, 9000, lib=lib)


def test_full_size_c2_all_against_oracle(lib, oracle, randqp):
    """BASELINE.json configs[1]: 2048 random dense QPs, n=100 n_eq=50 n_in=100.  Every QP must
    reach SOLVED with unscaled KKT residuals <= 1e-9 (numpy), and EVERY solution is compared with
    the oracle's (x, y, z) and status."""
    pc.case_random_batch(lib, oracle, randqp, 100, 50, 100, B=2048, compare="all")


def test_full_size_c3_on_one_gpu_all_against_oracle(lib, oracle, randqp):
    """BASELINE.json configs[2] (16 384 QPs, n=100 n_eq=50 n_in=100) at N = 1: one launch of one handle, every QP
    SOLVED, KKT <= 1e-9 (numpy), every solution and Info record against the oracle"""
    rec = pc.case_c3_one_launch(lib, oracle, randqp)
    assert rec["qps"] == 16384 and rec["max_kkt"] <= 1e-9


def test_full_size_c4_all_against_oracle(lib, oracle, randqp):
    """BASELINE.json configs[3] at its real size: ALL 512 QPs of shape (512, 200, 400), 1024-thread workgroups, every
    one against the oracle (solutions to 1e-10, Info counters equal, KKT <= 1e-9 in numpy)."""
    pc.case_c4_shape(lib, oracle, randqp, B=512)


@pytest.mark.parametrize("box", [False, True])
def test_full_shape_c5_against_oracle(lib, oracle, randqp, box):
    """BASELINE.json configs[4] at its real size: ALL 4096 QPs (n = 200, diagonal Hessian, 200 bound pairs), both forms,
    through the one-wavefront kernel; every QP against the oracle (1e-10, equal Info) and KKT-gated in numpy."""
    pc.case_c5(lib, oracle, randqp, B=4096, sample=4096, box=box)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
def test_dense_wave_kernel_flows(lib, oracle, randqp, monkeypatch, kernel):
    """the one-wavefront dense kernel (csrc/pqp_dwave.hpp) and its 256-thread A/B partner on the same cases, each against
    the oracle: random batches over the shapes the register layout distinguishes (odd n, no equalities, no inequalities,
    n = n_eq = n_in = 128, a Schur block beyond the 96 slots factorised in registers), the state machine under every
    initial guess, the infeasibility statuses, the verbose trace"""
    monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
    for (n, ne, ni, B) in [(10, 2, 3, 6), (33, 8, 11, 6), (12, 0, 9, 4), (9, 5, 0, 4), (100, 50, 100, 24), (64, 60, 70, 6),
                           (128, 128, 128, 4), (2, 1, 1, 4)]:
        pc.case_random_batch(lib, oracle, randqp, n, ne, ni, B)
    for guess in pc.InitialGuess:
        pc.case_state_machine(lib, oracle, randqp, guess)
    pc.case_infeasibility_statuses(lib, oracle)
    pc.case_verbose_round_trip(lib, oracle, randqp)
    # QPLayer backward on the state the forward kernel left in HBM (slot list, W_S, D_S, active-set flags)
    pc.case_backward(lib, oracle, randqp)
    pc.case_backward(lib, oracle, randqp, with_dual_terms=False)


def test_diag_mixed_handle(lib, oracle, randqp):
    """range / subset launches of structured QPs out of a handle that also holds a general one (parity_cases.case_diag_mixed_handle)"""
    pc.case_diag_mixed_handle(lib, oracle, randqp)


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
def test_diag_wave_kernel_flows(lib, oracle, randqp, monkeypatch, kernel):
    """the one-wavefront, register-resident diagonal-structure kernel (csrc/pqp_diag.hpp) and its 256-thread A/B partner
    through the whole solve state machine against the oracle, at the sizes of BASELINE.json configs[4] and at the edges of
    the kernel's range (dim 256 = four register slots per lane, dim 1)"""
    monkeypatch.setenv("PQP_DIAG_KERNEL", kernel)
    for dim, box in ((200, False), (200, True), (256, True), (256, False), (65, False), (1, True)):
        pc.case_diag_wave_flows(lib, oracle, randqp, dim, box=box, B=6 if dim > 1 else 2)
    pc.case_diag_wave_flows(lib, oracle, randqp, 200, box=True, hessian=pc.HessianType.Zero)
    pc.case_diag_wave_flows(lib, oracle, randqp, 120, box=False, constrained=False)
    forked = pc.case_diag_wave_flows(lib, oracle, randqp, 150, box=True, merit=1, B=8) + pc.case_diag_wave_flows(lib, oracle, randqp, 150, box=False, merit=1, B=8)
    import warnings
    warnings.warn(UserWarning("PDAL flows on the diagonal kernel (%s): %d forked results of %d" % (kernel, forked, 2 * 8 * 8)))
    assert forked <= 13, forked
    assert pc.case_diag_wave_infeasible(lib, oracle) != int(pc.QPSolverOutput.PROXQP_SOLVED)
    pc.case_diag_wave_backward(lib, oracle, randqp, dim=200, B=4)


def test_infeasibility_statuses(lib, oracle):
    pc.case_infeasibility_statuses(lib, oracle)


def test_seed14_mechanism_on_the_device(lib, randqp):
    """the one reference-held line the oracle misses (seed 14 of dense_qp_wrapper.cpp:7153-7215): on the MI355X the
    cycle, its fixed point and the phase-decided exit are asserted from the kernel's own Info records.  Sweeping the
    safe guard over 15 consecutive values (one period of the cycle in the oracle's iteration count), BOTH outcomes
    occur and each is the one mu at the exit implies: 14 runs end SOLVED within the reference test's lines and one ends
    MAX_ITER_REACHED on the MI355X, 11 and 4 for the oracle -- the stagnated outer iterations take one or two inner
    iterations by the last bits of |alpha dw| (solver.hpp:969), so the two count the phases differently; neither
    implementation, nor the reference binary, can be "right" about seed 14 beyond this."""
    n_ok, n = pc.case_seed14_mechanism(lib, randqp)
    assert n == 15 and 1 <= n_ok < n, (n_ok, n)


def test_verbose_round_trip(lib, oracle, randqp, capfd):
    pc.case_verbose_round_trip(lib, oracle, randqp)
    capfd.readouterr()  # (the host-side report of the verbose QPs)


def test_verbose_trace(lib, oracle, randqp, capfd):
    """per-iteration lines of settings.verbose: recorded by the kernel, equal to the oracle's line by line, printed"""
    assert pc.case_verbose_trace(lib, oracle, randqp, capfd) > 20
    # C2-sized QPs, and box constraints through the 512-thread kernel
    assert pc.case_verbose_trace(lib, oracle, randqp, capfd, n=100, ne=50, ni=100, B=16) > 400
    assert pc.case_verbose_trace(lib, oracle, randqp, capfd, n=60, ne=10, ni=40, B=4, box=True) > 20


def test_closest_feasible(lib, oracle, randqp):
    """reference test/src/dense_qp_wrapper.cpp:7153-7215, all 20 seeds, with and without
    primal_infeasibility_solving"""
    seen = pc.case_closest_feasible(lib, oracle, randqp, seeds=range(20))
    assert {0, 2} <= seen and (3 in seen or 0 in seen), seen  # SOLVED, PRIMAL_INFEASIBLE (+ closest-feasible runs)


@pytest.mark.parametrize("wps", [3, 4])
def test_register_budget_sweep_512_threads(oracle, randqp, wps):
    """512-thread workgroups at 170 and 128 VGPRs per lane (the product runs them at 256): round 1
    recorded NaNs at (512, 4) and simply did not instantiate it.  The kernel has been rewritten since
    (inverse-factor Schur block, no substitution chains) and the variants are correct; this keeps it so."""
    from proxsuite_amd import _build
    path = _build.VARIANT_DIR / ("libproxqp_hip_wps512_%d.so" % wps)
    assert path.exists(), "build the variants first (__graft_entry__.build())"
    vlib = N.NativeLib(path)
    for n, ne, ni, B in ((300, 40, 120, 8), (40, 5, 300, 8), (200, 100, 200, 8)):
        pc.case_random_batch(vlib, oracle, randqp, n, ne, ni, B=B)


@pytest.mark.parametrize("dim,B", [(20, 16), (100, 8)])
def test_primal_ldlt_engine(lib, oracle, randqp, dim, B):
    """DenseBackend::PrimalLDLT at benchmark/timings-dense-backend.cpp's shape (n_eq = n_in = 2 dim, box):
    256-thread (dim 20) and 512-thread (dim 100: 500 constraints) workgroups"""
    pc.case_primal_ldlt(lib, oracle, randqp, dim=dim, B=B)


def test_refinement_fallback(lib, oracle):
    """row a14 on the real device (the event counter needs the instrumented twin of the library)"""
    from proxsuite_amd import _build
    pc.case_refinement_fallback(lib, oracle, need_stats=False)
    pc.case_refinement_fallback(N.NativeLib(_build.HIP_STATS_LIB), oracle, need_stats=True)


def test_schur_factor_identity(lib, randqp):
    """rows a10-a13: accuracy of the rank-1 edited inverse Schur factor as the MI355X leaves it, C2 shape"""
    worst, edited = pc.case_schur_factor_identity(lib, randqp, 100, 50, 100, B=256)
    print("max |W S W^T - D| / max|D| = %.2e over %d edited factors" % (worst, edited))


def test_vectors_in_hbm_path(lib, oracle, randqp, monkeypatch):
    """the large-shape kernel (per-QP vectors in HBM) on ordinary shapes, against the oracle"""
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    pc.case_random_batch(lib, oracle, randqp, 100, 50, 100, B=64)
    pc.case_random_batch(lib, oracle, randqp, 300, 40, 120, B=8)
    pc.case_box_constraints(lib, oracle, randqp, seeds=8)


def test_diag_kernel_settings_sweep():
    """tests/test_emu_parity.py::test_diag_kernel_settings_sweep on the MI355X, dimensions up to 200"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "LIB"}
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "diag_kernel_sweep.py"), "2", "60"], capture_output=True, text=True,
                       env=env, timeout=1200)
    assert "60 shapes, 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_dense_wave_launch_forms(lib, randqp, monkeypatch):
    """Every launch form of the one-wavefront dense pair at a size its default dispatch takes (2048 C2-shaped QPs: the
    factorisation prologue and the iteration kernel both walk the same order array): a whole-batch solve, two ranges,
    a shuffled subset, and the opt-in learned order of a repeated whole-batch solve -- each QP's result must be the
    whole-batch solve's bit for bit (same kernel, same arithmetic, whatever the order or the slice)."""
    monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False)
    B, n, ne, ni = 2048, 100, 50, 100
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)

    def fresh():
        b = N.Batch(B, n, ne, ni, lib=lib)
        pc.settings_all(b, eps_abs=pc.EPS, eps_rel=0)
        b.init(-1, m.H, m.g, m.A, m.b, m.C, m.l, m.u)
        return b

    def snap(b):
        x, y, z, se, si, info = b.results()
        return x.copy(), y.copy(), z.copy(), np.array([(i.status, i.iter, i.iter_ext, i.mu_updates) for i in info])

    b = fresh()
    b.solve()
    assert b.last_kernel.startswith("pqp_dwave_kernel<") and b.launch_config()[0] == 64 and b.last_prologue_ms > 0  # the pair ran
    ref = snap(b)
    assert all(s == 0 for s in ref[3][:, 0])
    b.close()
    # two ranges of 1280 + 768 (the second one is below the dispatch's 0.6 of a round: force the pair for both)
    monkeypatch.setenv("PQP_DENSE_KERNEL", "wave")
    b = fresh()
    b.solve(0, 1280)
    b.solve(1280, 768)
    got = snap(b)
    for a, c in zip(ref, got):
        assert np.array_equal(a, c)
    b.close()
    # a shuffled subset of 1500 QPs, then the rest
    b = fresh()
    rng = np.random.default_rng(5)
    perm = rng.permutation(B)
    b.solve_subset(perm[:1500])
    b.solve_subset(perm[1500:])
    got = snap(b)
    for a, c in zip(ref, got):
        assert np.array_equal(a, c)
    b.close()
    monkeypatch.delenv("PQP_DENSE_KERNEL", raising=False)
    # the learned longest-first order: the second whole-batch solve is dispatched through the order array
    b = fresh()
    b.set_schedule(True)
    b.solve()
    b.solve()
    got = snap(b)
    for a, c in zip(ref, got):
        assert np.array_equal(a, c)
    b.close()

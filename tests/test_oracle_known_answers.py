"""Pins the CPU oracle on every literal known answer the reference's dense tests hold
(SURVEY.md 8(c), Appendix B)."""
import numpy as np
import pytest

from proxsuite_amd._ctypes_defs import InitialGuess, QPSolverOutput, HessianType


def test_cvxpy_1d(oracle):
    # reference test/src/cvxpy.cpp:61-102 : H=20, g=-10, 0<=x<=1 -> x*=0.5
    qp = oracle.QP(1, 0, 1)
    qp.settings.eps_abs = 1e-8
    qp.init(np.array([[20.0]]), np.array([-10.0]), None, None, np.array([[1.0]]), np.array([0.0]),
            np.array([1.0]))
    qp.solve()
    assert qp.results.info.status == QPSolverOutput.PROXQP_SOLVED
    assert abs(qp.results.x[0] - 0.5) <= 1e-8


def test_cvxpy_1d_start_from_solution(oracle):
    # reference test/src/cvxpy.cpp:104-160 : warm start at the solution -> iter <= 0
    qp = oracle.QP(1, 0, 1)
    qp.settings.eps_abs = 1e-8
    qp.init(np.array([[20.0]]), np.array([-10.0]), None, None, np.array([[1.0]]), np.array([0.0]),
            np.array([1.0]))
    qp.solve(np.array([0.5]), None, np.array([0.0]))
    assert qp.results.info.iter <= 0
    assert abs(qp.results.x[0] - 0.5) <= 1e-8


def test_cvxpy_3d_box(oracle):
    # reference test/src/cvxpy.cpp:22-59
    H = np.array([[13.0, 12.0, -2.0], [12.0, 17.0, 6.0], [-2.0, 6.0, 12.0]])
    g = np.array([-22.0, -14.5, 13.0])
    C = np.eye(3)
    l, u = -np.ones(3), np.ones(3)
    qp = oracle.QP(3, 0, 3)
    qp.settings.eps_abs = 1e-9
    qp.init(H, g, None, None, C, l, u)
    qp.solve()
    pri, dua = oracle.kkt_residuals(H, g, None, None, C, l, u, qp.results.x, qp.results.y, qp.results.z)
    assert pri <= 1e-9 and dua <= 1e-9


def test_lower_bounded_tridiagonal(oracle):
    # reference test/src/dense_qp_solve.py:302-333 : x* = [2]*149 + [3]
    n = 150
    M = np.eye(n)
    for i in range(1, n - 1):
        M[i, i + 1] = -1
        M[i, i - 1] = 1
    H = M @ M.T
    g = -np.ones(n)
    C = np.eye(n)
    l = 2.0 * np.ones(n)
    qp = oracle.QP(n, 0, n)
    qp.init(H, g, None, None, C, l, None)
    qp.solve()
    x_theoretically_optimal = np.array([2.0] * 149 + [3.0])
    assert np.max(np.abs(qp.results.x - x_theoretically_optimal)) < 1e-3


def test_simple_qp_with_infinity_lower_bound(oracle):
    # reference test/data/simple_qp_with_inifinity_lower_bound.mat (dense_qp_solve.py:375-405): its seven
    # arrays (a 3x3 QP) stored as tests/golden/simple_qp_with_infinity_lower_bound.npz
    import os
    m = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simple_qp_with_infinity_lower_bound.npz"))
    P, q = np.asarray(m["P"], float), np.asarray(m["q"], float).ravel()
    A, b = np.asarray(m["A"], float), np.asarray(m["b"], float).ravel()
    C, l, u = np.asarray(m["C"], float), np.asarray(m["l"], float).ravel(), np.asarray(m["u"], float).ravel()
    qp = oracle.QP(3, 1, 3)
    qp.init(P, q, A, b, C, l, u)
    qp.solve()
    pri, dua = oracle.kkt_residuals(P, q, A, b, C, l, u, qp.results.x, qp.results.y, qp.results.z)
    assert pri <= 1e-5 and dua <= 1e-5


def test_ruiz_algebra(oracle, randqp):
    # reference test/src/dense_ruiz_equilibration.cpp:15-72
    for dim in (10, 40, 100):
        randqp.set_seed(1)
        n_eq = n_in = dim // 2
        m = randqp.dense_strongly_convex_qp(dim, n_eq, n_in, 0.15, 1e-2)
        qp = oracle.QP(dim, n_eq, n_in)
        qp.init(m.H, m.g, m.A, m.b, m.C, m.l, m.u)
        s = qp.scaled()
        d = s["delta"]
        D, E, F = d[:dim], d[dim:dim + n_eq], d[dim + n_eq:]
        c = s["c"]
        assert np.max(np.abs(s["H"] - c * (D[:, None] * m.H * D[None, :]))) <= 1e-10
        assert np.max(np.abs(s["g"] - c * D * m.g)) <= 1e-10
        assert np.max(np.abs(s["A"] - E[:, None] * m.A * D[None, :])) <= 1e-10
        assert np.max(np.abs(s["b"] - E * m.b)) <= 1e-10
        assert np.max(np.abs(s["C"] - F[:, None] * m.C * D[None, :])) <= 1e-10


def test_dim_zero_throws(oracle):
    # reference dense/model.hpp:65-68
    with pytest.raises(ValueError):
        oracle.QP(0, 0, 0)


def test_reference_infeasible_qp_known_answer(oracle):
    """reference test/src/dense_qp_eq.cpp:217-256: the status is the reference's own check."""
    import parity_cases as pc
    from proxsuite_amd._ctypes_defs import QPSolverOutput
    P = pc.INFEASIBLE_QP
    q = oracle.QP(2, 0, 3)
    q.init(P["H"], P["g"], None, None, P["C"], P["l"], P["u"])
    q.settings.eps_rel, q.settings.eps_abs = 0.0, 1e-9
    q.solve()
    assert q.results.info.status == QPSolverOutput.PROXQP_PRIMAL_INFEASIBLE


def _closest_feasible_acceptance(H, g, A, b, C, l, u, x, y, z, eps):
    """The reference test's two acceptance lines (test/src/dense_qp_wrapper.cpp:7188-7207,
    test/src/dense_qp_wrapper.py:4803-4821)."""
    import numpy as np
    ne, ni = A.shape[0], C.shape[0]
    scaled_eps = float(np.max(np.abs(A.T @ np.ones(ne) + C.T @ np.ones(ni)))) * eps
    Cx = C @ x
    pri = np.max(np.abs(A.T @ (A @ x - b) + C.T @ (np.maximum(Cx - u, 0) + np.minimum(Cx - l, 0))))
    dua = np.max(np.abs(H @ x + g + A.T @ y + C.T @ z))
    return pri <= scaled_eps and dua <= eps, pri, dua


def _closest_feasible_qp(oracle, dim, ne, ni, eps, verbose=False):
    from proxsuite_amd._ctypes_defs import InitialGuess
    q = oracle.QP(dim, ne, ni)
    s = q.settings
    s.eps_abs, s.eps_rel, s.initial_guess = eps, 0, InitialGuess.NO_INITIAL_GUESS
    s.primal_infeasibility_solving, s.eps_primal_inf, s.eps_dual_inf = True, 1e-4, 1e-4
    s.verbose = int(verbose)  # the reference test sets it (:7178); it only perturbs last bits (solver.hpp:1469-1510)
    return q


def test_reference_primal_infeasibility_solving(oracle, randqp):
    """reference test/src/dense_qp_wrapper.cpp:7153-7215: 20 seeds of dim 20 pushed out of
    feasibility, closest-feasible solving on; the reference's two acceptance lines.  19 seeds pass them.
    Seed 14 falls into a cycle of the reference's BCL rule whose only exit is the safe guard; whether the
    run converges after that exit depends on the phase of the cycle (11 phases of 15 do), and with the
    default safe_guard the oracle sits in one of the 4 that do not -- derived, without the oracle, in
    test_seed14_is_a_fixed_point_of_the_reference_bcl_rule."""
    import parity_cases as pc
    models, dim, ne, ni = pc.infeasible_family(randqp, range(20))
    eps = 1e-5
    for seed, (H, g, A, b, C, l, u) in enumerate(models):
        q = _closest_feasible_qp(oracle, dim, ne, ni, eps, verbose=True)
        q.init(H, g, A, b, C, l, u)
        q.solve()
        ok, pri, dua = _closest_feasible_acceptance(H, g, A, b, C, l, u, q.results.x, q.results.y,
                                                    q.results.z, eps)
        if seed == 14:
            assert not ok and q.results.info.status == QPSolverOutput.PROXQP_MAX_ITER_REACHED
            continue
        assert ok, (seed, pri, dua)


def test_seed14_is_a_fixed_point_of_the_reference_bcl_rule(oracle, randqp):
    """Why seed 14 of test/src/dense_qp_wrapper.cpp:7153-7215 cannot meet the test's acceptance lines
    under the reference sources in /root/reference (instance-level argument).

    The instance is FEASIBLE (b + 10, u - 100 leave a feasible set) but badly scaled: the solution has
    |x| ~ 2e4 and multipliers ~ 1e7.  With NO_INITIAL_GUESS y = z = 0, and every outer iteration whose
    primal residual exceeds bcl_eta_ext is a "bad step" that puts y, z BACK to y_prev, z_prev
    (solver.hpp:604-606) and divides mu by 10 down to the floors mu_min_eq = 1e-9, mu_min_in = 1e-8
    (settings.hpp:222-223, solver.hpp:608-611).  So, as long as no step is good, the k-th subproblem is the
    plain quadratic-penalty problem

        min_x  1/2 x'Hx + g'x + rho/2 |x - x_prev|^2 + |Ax - b|^2 / (2 mu_eq) + |[Cx - u]_+|^2 / (2 mu_in)

    whose minimiser does not depend on the implementation.  In this mode Ruiz leaves the constraint ROWS
    unscaled (ruiz.hpp:170-171: delta.tail(n_eq + n_constraints).setOnes()), the column scaling is a change
    of variables, and the cost scaling c only multiplies g (it is 1 here anyway: after equilibration the mean
    column norm of H is <= 1, ruiz.hpp:278-281), so the residual the BCL rule sees is that of the UNSCALED
    penalty problem.  At the floors the minimiser (x_prev = x: a fixed point) has primal residual 0.129091,
    the BCL threshold there is bcl_eta_ext = 0.1^alpha_bcl * mu_in^alpha_bcl = 0.1^0.1 * (1e-8)^0.1 = 0.125893
    (solver.hpp:616 with settings.hpp:218): bad step again, multipliers back to 0, mu cannot shrink: the
    SAME subproblem is solved again and again.  Both residuals are then exactly unchanged, so the cold-restart
    test `new >= old` (solver.hpp:1700-1712) fires, mu goes back to 1/1.1 with y = z = 0 still, and the
    descent repeats with period 12 (mu = 0.909, 0.0909, ..., 9.1e-8, then 1e-8 four times).  The margin
    (0.1291 vs 0.1259) is 2.5 %, not a rounding tie: relative perturbations of the data up to 1e-3 do not
    change it, and the certificate of primal infeasibility, which would switch to the weighted residual, is a
    factor 30 away from firing.  (With Ruiz row scaling on -- the option off -- the same instance solves in 9
    outer iterations.)

    The ONLY exit from the cycle is the safe guard: once info.iter > safe_guard = 1e4 every step is accepted
    (solver.hpp:585), the multipliers are kept and mu stays where the cycle was at that moment.  From a small
    mu the method of multipliers then converges in a handful of iterations; from mu >= 1e-2 its linear rate
    is far too slow for the remaining outer iterations.  Sweeping the guard over one period shows it: 11 of 15
    consecutive phases end SOLVED within the reference test's acceptance lines, 4 end MAX_ITER_REACHED.  The
    phase at the moment info.iter crosses 1e4 counts inner iterations at a stagnated iterate (one or two per
    outer iteration, decided by `infty_norm(alpha * dw) < 1e-11`, solver.hpp:969), i.e. it is fixed by the last
    bits: the oracle lands on mu = 0.0909 and fails the lines, the MI355X kernel lands on a small mu and passes
    them (tests/parity_cases.py::case_closest_feasible accepts either, with the lines enforced on a SOLVED
    run), and the reference binary's outcome on its own seed 14 is one of the two for the same reason.
    """
    import parity_cases as pc
    (H, g, A, b, C, l, u), = pc.infeasible_family(randqp, [14])[0]
    dim, ne, ni = 20, 5, 5
    # --- plain numpy, no oracle: penalty minimiser at the mu floors, y_prev = z_prev = 0, x_prev = x
    mu_eq, mu_in = 1e-9, 1e-8                      # settings.hpp:222-223
    act = np.ones(ni, bool)
    for _ in range(50):
        K = H + A.T @ A / mu_eq + C[act].T @ C[act] / mu_in
        x = np.linalg.solve(K, -g + A.T @ b / mu_eq + C[act].T @ u[act] / mu_in)
        new = (C @ x - u) > 0
        if (new == act).all():
            break
        act = new
    pri_fixed_point = max(np.max(np.abs(A @ x - b)), np.max(np.maximum(C @ x - u, 0)))
    bcl_eta_ext_floor = 0.1 ** 0.1 * mu_in ** 0.1  # solver.hpp:1379 (init), :616 (bad step), alpha_bcl = 0.1
    assert abs(pri_fixed_point - 0.129091) < 1e-6 and abs(bcl_eta_ext_floor - 0.125893) < 1e-6
    assert pri_fixed_point > bcl_eta_ext_floor     # => bad step, forever
    # feasible all the same: an interior-point-free check through the equality-constrained least squares
    xf = np.linalg.lstsq(np.vstack([A, C]), np.concatenate([b, u - 1.0]), rcond=None)[0]
    assert np.max(np.abs(A @ xf - b)) < 1e-8 and np.all(C @ xf <= u)
    # --- the oracle runs into exactly that fixed point (11 outer iterations reach the floors) ...
    q = _closest_feasible_qp(oracle, dim, ne, ni, 1e-5)
    q.settings.max_iter = 11
    q.init(H, g, A, b, C, l, u)
    q.solve()
    assert abs(q.results.info.pri_res - pri_fixed_point) <= 1e-6 * pri_fixed_point
    assert np.max(np.abs(q.results.y)) == 0 and np.max(np.abs(q.results.z)) == 0
    # --- the exit through the safe guard: outcome by phase of the 12-periodic cycle (one period = 15 values of
    # info.iter, the stagnated outer iterations taking two inner ones)
    outcomes = []
    for guard in range(40, 55):
        q = _closest_feasible_qp(oracle, dim, ne, ni, 1e-5)
        q.settings.safe_guard, q.settings.max_iter = guard, 2500
        q.init(H, g, A, b, C, l, u)
        q.solve()
        ok, pri, dua = _closest_feasible_acceptance(H, g, A, b, C, l, u, q.results.x, q.results.y, q.results.z, 1e-5)
        st = q.results.info.status
        assert (st == QPSolverOutput.PROXQP_SOLVED and ok) or (st == QPSolverOutput.PROXQP_MAX_ITER_REACHED and not ok)
        assert ok == (q.results.info.mu_in < 5e-3), (guard, q.results.info.mu_in)  # decided by mu at the exit
        outcomes.append(ok)
    assert sum(outcomes) == 11 and len(outcomes) == 15
    # --- ... and leaves the option-off run alone (row scaling on): solved in 9 outer iterations
    q = _closest_feasible_qp(oracle, dim, ne, ni, 1e-5)
    q.settings.primal_infeasibility_solving = False
    q.init(H, g, A, b, C, l, u)
    q.solve()
    assert q.results.info.status == QPSolverOutput.PROXQP_SOLVED and q.results.info.iter_ext <= 10


def test_reference_python_infeasibility_family(oracle):
    """reference test/src/dense_qp_wrapper.py:4775-4821 (test_dense_infeasibility_solving): 20 instances of
    generate_mixed_qp(20, i) pushed out of feasibility, the same two acceptance lines.  The instances are
    the committed fixture tests/golden/python_infeasible_family.npz (made by
    tests/golden/make_python_family_fixtures.py with numpy / scipy's legacy global RNG exactly as the
    reference's generate_mixed_qp, :19-48, draws them)."""
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "python_infeasible_family.npz"))
    for i in range(20):
        H, g, A, b, C, u, l = (d["%s_%d" % (k, i)] for k in "HgAbCul")
        q = _closest_feasible_qp(oracle, 20, 5, 5, 1e-5)
        q.settings.eps_dual_inf = 1e-4
        q.init(H, g, A, b, C, l, u)
        q.solve()
        ok, pri, dua = _closest_feasible_acceptance(H, g, A, b, C, l, u, q.results.x, q.results.y,
                                                    q.results.z, 1e-5)
        assert ok, (i, pri, dua)

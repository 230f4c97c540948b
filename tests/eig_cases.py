"""Shared cases of the batched minimal-eigenvalue estimate (pqp_estimate_min_eigenvalues, csrc/pqp_eig.hpp) and of the
per-QP manual_minimal_H_eigenvalue of a bulk init / update.  tests/test_emu_eig.py runs them on the CPU SIMT emulator,
tests/test_gpu_eig.py on the device: a case takes the library (`_native.NativeLib`) it runs on.

Matrices are Q diag(lambda) Q^T, symmetrised, with Q from a seeded numpy QR: the smallest eigenvalue is known by
construction.  Where the spectrum is not prescribed numpy.linalg.eigvalsh is the truth.

Gates (u = 2^-53, ||.||_2 the spectral norm from numpy):
  ExactMethod      |dev - truth| <= 8 n u ||H||_2: the form of the backward-error bound of tridiagonalisation plus bisection;
                   a float64 Hessenberg reduction plus Sturm bisection and eigvalsh differ by at most 0.71 n u ||H||_2 on
                   these shapes, the 8 leaves about a factor ten.
  PowerIteration   converged: |dev - lambda_min| <= 2 sqrt(n) accuracy.  For symmetric M and a unit vector v some eigenvalue
                   lies within ||M v - theta v||_2 <= sqrt(n) ||.||_inf of theta; once for each of the two loops; the gap
                   of the spectrum makes the extreme eigenvalue the one found.  And |dev - host helper| <= 4 sqrt(n) accuracy.
"""
import functools

import numpy as np
import pytest

from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import EigenValueEstimateMethodOption as Opt

U = 2.0 ** -53

# ExactMethod: 1, 2, 3, around the wavefront (63 - 65), either side of the LDS / HBM hand-over of the working copy
# (pqp::EIG_RESIDENT_MAX = 128), more than one pass of the 256 threads over a row (257)
EXACT_ORDERS = (1, 2, 3, 16, 17, 63, 64, 65, 128, 129, 200, 257)
EXACT_ORDER_GPU_ONLY = 600
KINDS = ("random", "linspace", "double", "diagonal", "zero", "negdef", "scaled_down", "scaled_up")
POWER_ORDERS = (2, 3, 17, 64, 65, 129, 200)
POWER_SETTINGS = ((1e-3, 1000), (1e-8, 1000))


def _sym(A):
    return (A + A.T) / 2


def _orthogonal(n, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Q


def from_spectrum(lam, rng):
    lam = np.asarray(lam, dtype=np.float64)
    Q = _orthogonal(len(lam), rng)
    return _sym(Q @ np.diag(lam) @ Q.T)


@functools.lru_cache(maxsize=None)
def exact_kind(kind, n, seed=0):
    """(H, truth) of one kind at order n; computed once per (kind, n, seed) and shared (do not write into H)"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind in ("random", "scaled_down", "scaled_up"):
        H = _sym(np.random.default_rng([seed, n]).standard_normal((n, n)))  # (the same matrix under the three kinds)
        H = H * {"random": 1.0, "scaled_down": 1e-8, "scaled_up": 1e8}[kind]
        truth = np.linalg.eigvalsh(H)[0]
    elif kind == "linspace":
        lam = np.linspace(-3, 5, n)
        H, truth = from_spectrum(lam, rng), float(lam.min())
    elif kind == "double":  # a DOUBLE smallest eigenvalue
        lam = np.concatenate([[-2.0, -2.0], np.linspace(1, 4, max(n - 2, 0))])[:n]
        H, truth = from_spectrum(lam, rng), -2.0
    elif kind == "diagonal":
        d = rng.standard_normal(n)
        H, truth = np.diag(d), float(d.min())
    elif kind == "zero":
        H, truth = np.zeros((n, n)), 0.0
    elif kind == "negdef":
        M = rng.standard_normal((n, n))
        H = -_sym(M @ M.T + np.eye(n))
        truth = np.linalg.eigvalsh(H)[0]
    else:
        raise KeyError(kind)
    H.setflags(write=False)
    return H, float(truth)


def exact_gate(H):
    n = H.shape[0]
    return 8 * n * U * np.linalg.norm(H, 2)


def check_exact(got, cases, what):
    """every value within its gate; returns the worst |dev - truth| / (n u ||H||_2) (0 for the zero matrix)"""
    worst = 0.0
    for i, (H, truth) in enumerate(cases):
        err, gate = abs(float(got[i]) - truth), exact_gate(H)
        ratio = err / (gate / 8) if gate > 0 else 0.0
        print("%s [%d] order %d: dev %.17g truth %.17g |err| %.3g = %.3f n u ||H||_2 (gate 8)" % (
            what, i, H.shape[0], got[i], truth, err, ratio))
        worst = max(worst, ratio)
        assert np.isfinite(got[i]) and err <= gate, (what, i, got[i], truth, err, gate)
    return worst


def case_exact_order(lib, n, to_input=np.stack):
    """all kinds at order n in ONE launch of len(KINDS) matrices"""
    cases = [exact_kind(k, n) for k in KINDS]
    got = N.estimate_min_eigenvalues(to_input([H for H, _ in cases]), Opt.ExactMethod, lib=lib)
    return check_exact(np.asarray(got.cpu() if hasattr(got, "cpu") else got), cases, "exact")


def case_exact_single(lib):
    """one launch of a single matrix"""
    H, truth = exact_kind("random", 17)
    got = N.estimate_min_eigenvalues(H[None], Opt.ExactMethod, lib=lib)
    assert got.shape == (1,)
    check_exact(got, [(H, truth)], "single")


def mixed_70():
    return [exact_kind(KINDS[i % len(KINDS)], 65, seed=i // len(KINDS)) for i in range(70)]


def case_exact_mixed(lib, to_input=np.stack):
    """one launch of 70 matrices of mixed kinds at order 65 (more workgroups than one round of the emulated device)"""
    cases = mixed_70()
    got = N.estimate_min_eigenvalues(to_input([H for H, _ in cases]), Opt.ExactMethod, lib=lib)
    return got, check_exact(np.asarray(got.cpu() if hasattr(got, "cpu") else got), cases, "mixed")


def host_helper(H, *a):
    from proxsuite_amd.proxqp import dense
    return dense.estimate_minimal_eigen_value_of_symmetric_matrix(H, *a)


@functools.lru_cache(maxsize=None)
def power_pair(n):
    """spectrum linspace(-1, 1, n) with the ends replaced by -2 and 4, and its negative: (H, lambda_min) twice"""
    lam = np.linspace(-1, 1, n)
    lam[0], lam[-1] = -2.0, 4.0
    H = from_spectrum(lam, np.random.default_rng([7, n]))
    H.setflags(write=False)
    return (H, -2.0), (-H, -4.0)


def case_power_converged(lib, n, accuracy, nb):
    cases = power_pair(n)
    got = N.estimate_min_eigenvalues(np.stack([H for H, _ in cases]), Opt.PowerIteration, accuracy, nb, lib=lib)
    for (H, lam_min), dev in zip(cases, got):
        host = host_helper(H, Opt.PowerIteration, accuracy, nb)
        print("power order %d accuracy %g: dev %.17g lambda_min %g |err| %.3g (gate %.3g), |dev - host| %.3g" % (
            n, accuracy, dev, lam_min, abs(dev - lam_min), 2 * np.sqrt(n) * accuracy, abs(dev - host)))
        assert abs(dev - lam_min) <= 2 * np.sqrt(n) * accuracy
        assert abs(dev - host) <= 4 * np.sqrt(n) * accuracy


def case_power_cut_short(lib):
    """nb = 3: Rayleigh quotients lie inside the spectrum in both loops, so the result does, up to rounding"""
    for n in (17, 65, 129):
        H, _ = exact_kind("random", n)
        lam = np.linalg.eigvalsh(H)
        dev = float(N.estimate_min_eigenvalues(H[None], Opt.PowerIteration, 1e-3, 3, lib=lib)[0])
        slack = exact_gate(H)
        print("cut short order %d: dev %.17g in [%.17g, %.17g]" % (n, dev, lam[0], lam[-1]))
        assert np.isfinite(dev) and lam[0] - slack <= dev <= lam[-1] + slack


def case_power_nb_zero(lib):
    """nb <= 0: both loops return eig = 0, the reference's arithmetic gives min(0 - 0, 0) = 0"""
    H, _ = exact_kind("random", 17)
    for nb in (0, -5):
        assert float(N.estimate_min_eigenvalues(H[None], Opt.PowerIteration, 1e-3, nb, lib=lib)[0]) == 0.0


def case_power_degenerate(lib):
    """2 I at order 5, the zero matrix, order 1: the shifted iterate may be exactly zero, where the reference divides by a
    zero norm (rounding-dependent).  The call returns; each value is NaN or within the converged gate."""
    for H, lam_min in ((2 * np.eye(5), 2.0), (np.zeros((5, 5)), 0.0), (np.array([[3.0]]), 3.0), (np.array([[-3.0]]), -3.0)):
        dev = float(N.estimate_min_eigenvalues(H[None], Opt.PowerIteration, 1e-3, 1000, lib=lib)[0])
        print("degenerate order %d: dev %r (lambda_min %g)" % (H.shape[0], dev, lam_min))
        assert np.isnan(dev) or abs(dev - lam_min) <= 2 * np.sqrt(H.shape[0]) * 1e-3


def case_errors(lib):
    import ctypes as C
    Hs = np.stack([exact_kind("random", 9, seed=s)[0] for s in range(5)])
    Hs[3, 2, 6] += 1e-9  # far above eps ||H||_F
    for method in (Opt.ExactMethod, Opt.PowerIteration):
        with pytest.raises(ValueError, match=r"H is not symmetric\..*\b3\b"):
            N.estimate_min_eigenvalues(Hs, method, lib=lib)
    # the reference's rule is RELATIVE (isApprox): an asymmetry of a few eps ||H||_F passes, and a zero matrix is symmetric
    ok = np.stack([exact_kind("random", 9)[0], np.zeros((9, 9))])
    ok[0, 1, 2] *= 1 + 2.0 ** -52
    assert N.estimate_min_eigenvalues(ok, Opt.ExactMethod, lib=lib).shape == (2,)
    # an order above the limit (8192) is refused before anything is read
    dummy, out = np.zeros(4), np.zeros(1)
    rc = lib.L.pqp_estimate_min_eigenvalues(0, 1, 8193, C.c_void_p(dummy.ctypes.data), int(Opt.ExactMethod), 1e-3, 1000,
                                            C.c_void_p(out.ctypes.data), None)
    assert rc == -4  # PQP_ERR_UNSUPPORTED
    with pytest.raises(N.NativeError, match="error -4"):
        lib.check(rc)
    assert N.estimate_min_eigenvalues(np.zeros((0, 5, 5)), Opt.ExactMethod, lib=lib).shape == (0,)
    assert lib.L.pqp_estimate_min_eigenvalues(0, 0, 5, None, int(Opt.ExactMethod), 1e-3, 1000, None, None) == 0
    with pytest.raises(ValueError):
        N.estimate_min_eigenvalues(np.zeros((2, 3, 4)), Opt.ExactMethod, lib=lib)


def _helpers_matrix(seed=4, n=12):
    """the model of api_cases.case_nonconvex_helpers"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    H = (M + M.T) / 2
    g = rng.standard_normal(n)
    return H, g


def case_2d_unchanged():
    """the 2-D call keeps its code path: bit-identical to what it was before the batched entry existed (restated here)"""
    from proxsuite_amd.proxqp import dense
    from proxsuite_amd.utils import random_qp as rq

    def before(H, method=Opt.ExactMethod, accuracy=1.0e-3, nb=1000):
        H = np.ascontiguousarray(np.asarray(H, dtype=np.float64))
        n = H.shape[0]
        if method == Opt.ExactMethod:
            return float(rq.min_eigenvalue_symmetric(H))

        def power(op):
            rhs = np.full(n, 1.0 / np.sqrt(n))
            dw = op(rhs)
            eig = 0.0
            for _ in range(int(nb)):
                rhs = dw / np.linalg.norm(dw)
                dw = op(rhs)
                eig = float(rhs @ dw)
                if np.max(np.abs(dw - eig * rhs)) <= accuracy:
                    break
            return eig

        dominant = power(lambda v: H @ v)
        min_eig = dominant - power(lambda v: dominant * v - H @ v)
        return float(min(min_eig, dominant))

    H, _ = _helpers_matrix()
    f = dense.estimate_minimal_eigen_value_of_symmetric_matrix
    for args in ((), (Opt.ExactMethod, 1e-6, 10000), (Opt.PowerIteration,), (Opt.PowerIteration, 1e-10, 100000)):
        a, b = f(H, *args), before(H, *args)
        assert isinstance(a, float) and a.hex() == b.hex(), (args, a, b)
    with pytest.raises(ValueError, match=r"^H is not symmetric\.$"):
        f(H + np.triu(np.ones(H.shape), 1))
    with pytest.raises(ValueError, match="wrong argument size"):
        f(np.zeros((3, 4)))


def case_dense_3d(lib, monkeypatch, to_input=np.stack):
    """dense.estimate_minimal_eigen_value_of_symmetric_matrix on a 3-D input: the device entry, B values"""
    from proxsuite_amd.proxqp import dense
    monkeypatch.setattr(N, "_lib", lib)  # (the library `load()` hands out: the emulator's in the CPU suite)
    cases = [exact_kind(k, 16) for k in KINDS]
    Hs = to_input([H for H, _ in cases])
    got = dense.estimate_minimal_eigen_value_of_symmetric_matrix(Hs)
    assert type(got) is type(Hs) and tuple(got.shape) == (len(cases),)
    check_exact(np.asarray(got.cpu() if hasattr(got, "cpu") else got), cases, "dense 3-D")
    p = dense.estimate_minimal_eigen_value_of_symmetric_matrix(Hs, dense.EigenValueEstimateMethodOption.PowerIteration, 1e-6, 50)
    assert tuple(p.shape) == (len(cases),)
    bad = np.stack([H for H, _ in cases])
    bad[5, 0, 3] += 1.0
    with pytest.raises(ValueError, match=r"^H is not symmetric\.$"):
        dense.estimate_minimal_eigen_value_of_symmetric_matrix(to_input(list(bad)))


def case_end_to_end(lib, make_batch=None):
    """Six different indefinite Hessians of order 12 on the box [-1, 1]^n (the model of case_nonconvex_helpers, seeds
    4 .. 9): estimates from the batched exact call, ONE bulk init with the array, against a handle initialised QP by QP."""
    n, B = 12, 6
    make_batch = make_batch or (lambda: N.Batch(B, n, 0, n, lib=lib))
    models = [_helpers_matrix(s) for s in range(4, 4 + B)]
    H = np.stack([m[0] for m in models])
    g = np.stack([m[1] for m in models])
    Cm = np.stack([np.eye(n)] * B)
    l, u = -np.ones((B, n)), np.ones((B, n))
    e = N.estimate_min_eigenvalues(H, Opt.ExactMethod, lib=lib)
    assert np.all(e < 0) and len(set(e.tolist())) == B
    check_exact(e, [(h, np.linalg.eigvalsh(h)[0]) for h in H], "end to end")

    bulk, one = make_batch(), N.Batch(B, n, 0, n, lib=lib)
    for b in (bulk, one):
        for i in range(B):
            b.settings(i).eps_abs = 1e-9
    rho0 = bulk.settings(0).default_rho
    bulk.init(-1, H, g, None, None, Cm, l, u, manual_minimal_H_eigenvalue=e)
    for i in range(B):
        one.init(i, H[i], g[i], None, None, Cm[i], l[i], u[i], manual_minimal_H_eigenvalue=float(e[i]))
    for i in range(B):
        assert bulk.settings(i).default_H_eigenvalue_estimate == e[i]
        assert bulk.settings(i).default_rho == rho0 + abs(e[i])
        assert one.settings(i).default_rho == bulk.settings(i).default_rho
    bulk.solve()
    one.solve()
    xb, yb, zb, _, _, info = bulk.results()
    xo, yo, zo, _, _, _ = one.results()
    for i in range(B):
        assert info[i].minimal_H_eigenvalue_estimate == e[i]
        assert info[i].status == 0, (i, info[i].status)
        assert np.max(np.abs(H[i] @ xb[i] + g[i] + zb[i])) <= 1e-9
        assert np.all(np.abs(xb[i]) <= 1 + 1e-9)
    # the same kernel and the same arithmetic as the handle that was initialised QP by QP with the scalar argument
    assert np.array_equal(xb, xo) and np.array_equal(yb, yo) and np.array_equal(zb, zo)

    # update adds |e[i]| again per QP, as the scalar call does
    bulk.update(-1, manual_minimal_H_eigenvalue=e)
    for i in range(B):
        one.update(i, manual_minimal_H_eigenvalue=float(e[i]))
        assert bulk.settings(i).default_rho == (rho0 + abs(e[i])) + abs(e[i])
        assert bulk.settings(i).default_rho == one.settings(i).default_rho
    bulk.close()
    one.close()

    # a NaN entry is "absent", as the scalar's NaN is: QP 2 stays at the estimate 0
    holes = e.copy()
    holes[2] = np.nan
    b = make_batch()
    b.init(-1, H, g, None, None, Cm, l, u, manual_minimal_H_eigenvalue=holes)
    for i in range(B):
        want = 0.0 if i == 2 else e[i]
        assert b.settings(i).default_H_eigenvalue_estimate == want
        assert b.settings(i).default_rho == rho0 + abs(want)
    # one entry for one addressed QP; any other length is refused
    b.init(2, H[2], g[2], None, None, Cm[2], l[2], u[2], manual_minimal_H_eigenvalue=e[2:3])
    assert b.settings(2).default_H_eigenvalue_estimate == e[2]
    with pytest.raises(ValueError, match="manual_minimal_H_eigenvalue"):
        b.init(-1, H, g, None, None, Cm, l, u, manual_minimal_H_eigenvalue=e[:3])
    b.close()

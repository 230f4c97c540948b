"""Cases of the forward-mode sensitivities (pqp_batch_tangent_multi, csrc/pqp_tangent.hpp), shared by
tests/test_emu_tangent.py (CPU emulator) and tests/test_gpu_tangent.py (MI355X).

Settings as tests/backward_multi_cases.py: forward eps_abs = 1e-9, eps_rel = 0; backward (eps, rho, mu) = (1e-5, 1e-7, 1e-7).
QPs from randqp.dense_strongly_convex_qp_batch, default shape (10, 4, 7), B = 6, K = 5.  Tangents are standard normal with a
fixed seed; dH is NOT symmetric.  Every case asserts that each QP has an active and an inactive inequality.

Gates.
  assembly : per entry (m + 2) 2^-52 sum |terms of that entry|, m the number of products summed -- the bound of a dot
             product in any order, with or without contraction; computed here from the absolute values.
  vs backward_multi (the untouched path, on a SECOND handle with the same init + solve, fed ld = (r_x | r_y | r_z)):
             1e-10 (1 + max |ref|), the project's gate for two kernels of one algorithm, on x, y and the ACTIVE z rows;
             inactive rows of T_z are exactly 0; the flags are equal.  Used where backward_multi is right: identity
             equilibration (its repeated scaling is by 1), or a right-hand side without z part.
  adjoint  : T_x[i] = sum over the parameters of <dL/dtheta, dtheta> with dL/dtheta from pqp_batch_backward for ld = e_i:
             1e-6 (1 + max |ref|), the project's gate between independently written restatements at these settings.
  KKT      : T_y, T_z under Ruiz equilibration against a numpy solve of the regularised, equilibrated KKT system built from
             pqp_batch_get_scaled and the returned flags.  The margin is measured: the same numpy restatement against
             backward_multi for x-only rows on the same QPs (`measure_m0`), on commit db806a7 on the emulator, gives the
             largest relative discrepancy m0 = 1.733e-15 (M0 below); the gate is max(10 m0, 1e-12) (1 + max |ref|) =
             1e-12 (1 + max |ref|), never above 1e-6.
"""
import ctypes as C

import numpy as np
import pytest

import backward_multi_cases as bc
from proxsuite_amd import _native as N

EPS, BW = bc.EPS, bc.BW
# measured by measure_m0 on commit db806a7 (CPU emulator, plain and mirrored batches of `default_model`)
M0 = 1.733e-15
KKT_GATE = max(10 * M0, 1e-12)
assert KKT_GATE <= 1e-6
NAMES = ("H", "g", "A", "b", "C", "l", "u")
U = 2.0 ** -52


def tails(n, ne, ni):
    return dict(H=(n, n), g=(n,), A=(ne, n), b=(ne,), C=(ni, n), l=(ni,), u=(ni,))


def random_tangents(B, K, n, ne, ni, names=NAMES, shared=(), seed=11):
    """name -> [B, K, ...] ([K, ...] for the names in `shared`), standard normal; every name draws from its own stream so
    that a subset of names has the values the full set has"""
    out = {}
    for k, name in enumerate(NAMES):
        if name in names:
            rng = np.random.default_rng(seed + k)
            lead = (K,) if name in shared else (B, K)
            out[name] = rng.standard_normal(lead + tails(n, ne, ni)[name])
    return out


def kw(t):
    return {"d" + k: v for k, v in t.items()}


def default_model(randqp, mirror=False, B=6, n=10, ne=4, ni=7):
    model = bc.model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    return bc.mirrored(model) if mirror else model


def solved(lib, model, precond=True, **kwargs):
    H, g, A, bb, Cm, l, u = model
    B, n = g.shape
    ne = 0 if A is None else A.shape[1]
    ni = 0 if Cm is None else Cm.shape[1]
    b = N.Batch(B, n, ne, ni, lib=lib, **kwargs)
    bc._settings(b, eps_abs=EPS, eps_rel=0)
    b.init(-1, H, g, A, bb, Cm, l, u, compute_preconditioner=precond)
    b.solve()
    return b


def full(t, name, B, K, n, ne, ni):
    """tangent `name` as a [B, K, ...] array: zeros when absent, broadcast when shared"""
    shape = (B, K) + tails(n, ne, ni)[name]
    if name not in t:
        return np.zeros(shape)
    return np.broadcast_to(t[name], shape) if t[name].ndim == len(shape) - 1 else t[name]


def rhs_numpy(t, x, y, z, K):
    """(R, S): the three formulas (r_x | r_y | dC x) in numpy and per entry (m + 2) * sum |terms|"""
    B, n = x.shape
    ne, ni = y.shape[1], z.shape[1]
    f = {k: full(t, k, B, K, n, ne, ni) for k in NAMES}
    X, Y, Z = x[:, None, :], y[:, None, :], z[:, None, :]
    sym = 0.5 * (f["H"] + np.swapaxes(f["H"], -1, -2))
    mv = lambda M, v: np.einsum("bkij,bkj->bki", M, np.broadcast_to(v, M.shape[:2] + (M.shape[3],)))
    mtv = lambda M, v: np.einsum("bkij,bki->bkj", M, np.broadcast_to(v, M.shape[:3]))
    rx = mv(sym, X) + f["g"] + mtv(f["A"], Y) + mtv(f["C"], Z)
    ry = mv(f["A"], X) - f["b"]
    rz = mv(f["C"], X)
    a = {k: np.abs(v) for k, v in f.items()}
    sx = 0.5 * (mv(a["H"], np.abs(X)) + mtv(a["H"], np.abs(X))) + a["g"] + mtv(a["A"], np.abs(Y)) + mtv(a["C"], np.abs(Z))
    sy = mv(a["A"], np.abs(X)) + a["b"]
    sz = mv(a["C"], np.abs(X))
    S = np.concatenate([(2 * n + ne + ni + 2) * sx, (n + 2) * sy, (n + 2) * sz], axis=-1)
    return np.concatenate([rx, ry, rz], axis=-1), S


def call(b, t, K=None, shared=(), **more):
    rows = more.get("count", len(more["idx"]) if "idx" in more else b.B)
    ntot = b.n + b.n_eq + b.n_in
    if K is None:
        K = next(v.shape[0 if k in shared else 1] for k, v in t.items())
    rhs = np.full((rows, K, ntot), np.nan)
    T, active = b.tangent_multi(*BW, shared=shared, rhs=rhs, n_dir=K, **kw(t), **more)
    return T, active, rhs


def check_active(active, ni, mirror=False):
    n_active = np.count_nonzero(active, axis=1)
    print("active inequalities per QP:", n_active.tolist(), "flags:", sorted(set(active.ravel().tolist())))
    assert np.all(n_active >= 1) and np.all(n_active < ni), n_active
    assert np.any(active & (2 if mirror else 1))


def ld_of(rhs, active, t, n, ne):
    """the loss derivative whose backward_multi solve is the tangent: (r_x | r_y | r_z), r_z = 0 on inactive rows"""
    B, K, ntot = rhs.shape
    ni = ntot - n - ne
    ld = rhs.copy()
    up, low = ((active & 1) != 0)[:, None, :], ((active & 2) != 0)[:, None, :]
    rz = ld[..., n + ne:]
    rz -= np.where(up, full(t, "u", B, K, n, ne, ni), 0.0) + np.where(low, full(t, "l", B, K, n, ne, ni), 0.0)
    rz[np.broadcast_to((active == 0)[:, None, :], rz.shape)] = 0.0
    return ld


def gate_vs_backward(T, active, ref_batch, ld, n, ne, what, **sel):
    """T against backward_multi on `ref_batch` (re-solved first): x, y, active z rows within 1e-10 (1 + max |ref|); exact
    zeros on inactive rows; equal flags"""
    ref_batch.solve()
    V, ref_active = ref_batch.backward_multi(ld, *BW, **sel)
    assert np.array_equal(active, ref_active), what
    on = np.broadcast_to((active != 0)[:, None, :], T[..., n + ne:].shape)
    assert np.all(T[..., n + ne:][~on] == 0.0), what + ": inactive rows of T_z must be exactly 0"
    bc.gate(T[..., :n + ne], V[..., :n + ne], 1e-10, what + " T_x, T_y vs backward_multi")
    bc.gate(T[..., n + ne:][on], V[..., n + ne:][on], 1e-10, what + " T_z (active rows) vs backward_multi")


def kkt_numpy(b, q, r, active, rho, mu):
    """numpy solve of the regularised, equilibrated KKT system of QP q at the active rows for the right-hand sides r
    ([K, ntot]: (r_x | r_y | r_z)); returns the unscaled [K, ntot] with zeros on inactive rows.  Call before anything
    rewrites the scaled model."""
    n, ne, ni = b.n, b.n_eq, b.n_in
    s = b.scaled(q)
    c, dX, dE, dI = s["c"], s["delta"][:n], s["delta"][n:n + ne], s["delta"][n + ne:]
    J = np.flatnonzero(active)
    na = len(J)
    M = np.zeros((n + ne + na, n + ne + na))
    M[:n, :n] = s["H"] + rho * np.eye(n)
    M[:n, n:n + ne], M[n:n + ne, :n] = s["A"].T, s["A"]
    M[:n, n + ne:], M[n + ne:, :n] = s["C"][J].T, s["C"][J]
    M[n:, n:] = -mu * np.eye(ne + na)
    rhs = np.concatenate([-r[:, :n] * dX * c, -r[:, n:n + ne] * dE, -r[:, n + ne:][:, J] * dI[J]], axis=1)
    sol = np.linalg.solve(M, rhs.T).T
    out = np.zeros_like(r)
    out[:, :n] = sol[:, :n] * dX
    out[:, n:n + ne] = sol[:, n:n + ne] * dE / c
    out[:, n + ne + J] = sol[:, n + ne:] * dI[J] / c
    return out


def measure_m0(lib, randqp):
    """largest relative discrepancy between the numpy restatement and backward_multi for x-only rows (x, y, active z)"""
    worst = 0.0
    for mirror in (False, True):
        model = default_model(randqp, mirror)
        B, n = model[1].shape
        ne, ni = model[2].shape[1], model[4].shape[1]
        b = solved(lib, model)
        ld = bc.random_rows(B, 5, n, ne, ni, dual_rows=0)
        probe, act = solved(lib, model).backward_multi(ld, *BW)
        ref = np.stack([kkt_numpy(b, q, ld[q], act[q], BW[1], BW[2]) for q in range(B)])
        V, active = b.backward_multi(ld, *BW)
        assert np.array_equal(active, act)
        on = np.concatenate([np.ones((B, n + ne), bool), active != 0], axis=1)[:, None, :]
        on = np.broadcast_to(on, V.shape)
        worst = max(worst, float(np.max(np.abs(V - ref)[on])) / (1 + float(np.max(np.abs(ref[on])))))
        b.close()
    return worst


# ---- 1. assembly against numpy -------------------------------------------------------------------------------------------------
def gate_rhs(rhs, t, x, y, z, K, what):
    ref, S = rhs_numpy(t, x, y, z, K)
    err = np.abs(rhs - ref)
    ratio = float(np.max(err / np.where(S > 0, U * S, 1.0)))
    print("%s: max |rhs - numpy| %.3e, worst entry at %.3f of its gate" % (what, float(err.max()), ratio))
    assert np.all(np.isfinite(rhs)) and np.all(err <= U * S), (what, ratio)


def case_assembly(lib, randqp):
    B, n, ne, ni, K = 6, 10, 4, 7, 5
    model = default_model(randqp)
    b = solved(lib, model)
    x, y, z = b.results()[:3]
    t = random_tangents(B, K, n, ne, ni)
    assert not np.allclose(t["H"], np.swapaxes(t["H"], -1, -2))
    T, active, rhs = call(b, t)
    check_active(active, ni)
    gate_rhs(rhs, t, x, y, z, K, "all seven")
    _, _, again = call(b, t)
    assert np.array_equal(rhs, again), "the assembly repeats its bits"
    only_c = {"C": t["C"]}
    gate_rhs(call(b, only_c)[2], only_c, x, y, z, K, "only dC")
    vec = {k: t[k] for k in ("g", "b", "l", "u")}
    r = call(b, vec)[2]
    assert np.array_equal(r, np.concatenate([t["g"], -t["b"], np.zeros((B, K, ni))], axis=-1)), "vectors only"
    sh = random_tangents(B, K, n, ne, ni, shared=("H", "A", "C"))
    mat = dict(sh, **{k: np.ascontiguousarray(np.broadcast_to(sh[k], (B,) + sh[k].shape)) for k in ("H", "A", "C")})
    r_sh, r_mat = call(b, sh, shared=("H", "A", "C")), call(b, mat)
    assert np.array_equal(r_sh[2], r_mat[2]) and np.array_equal(r_sh[0], r_mat[0]), "shared matrices vs materialised copies"
    gate_rhs(r_sh[2], sh, x, y, z, K, "shared matrices")
    mixed = {k: t[k] for k in ("H", "b", "C", "u")}
    gate_rhs(call(b, mixed)[2], mixed, x, y, z, K, "absent mixed with present")
    b.close()


# ---- 2. the solve against backward_multi, identity equilibration ---------------------------------------------------------------
def case_solve_identity(lib, randqp, mirror=False):
    B, n, ne, ni, K = 6, 10, 4, 7, 5
    model = default_model(randqp, mirror)
    b, r = solved(lib, model, precond=False), solved(lib, model, precond=False)
    t = random_tangents(B, K, n, ne, ni)
    T, active, rhs = call(b, t)
    assert T.shape == (B, K, n + ne + ni) and active.shape == (B, ni) and active.dtype == np.int32
    check_active(active, ni, mirror)
    gate_vs_backward(T, active, r, ld_of(rhs, active, t, n, ne), n, ne, "identity equilibration" + (", mirrored" if mirror else ""))
    b.close()
    r.close()
    return T, active


# ---- 3. Ruiz equilibration on --------------------------------------------------------------------------------------------------
def case_equilibrated(lib, randqp, mirror=False):
    B, n, ne, ni, K = 6, 10, 4, 7, 5
    model = default_model(randqp, mirror)
    b, r = solved(lib, model), solved(lib, model)
    what = "equilibrated" + (", mirrored" if mirror else "")
    # tangents without z part: backward_multi is right under any equilibration
    zfree = random_tangents(B, K, n, ne, ni, names=("H", "g", "A", "b"))
    T, active, rhs = call(b, zfree)
    check_active(active, ni, mirror)
    gate_vs_backward(T, active, r, ld_of(rhs, active, zfree, n, ne), n, ne, what + ", z-free")
    # the full set: T_x against the adjoint identity
    t = random_tangents(B, K, n, ne, ni)
    b.solve()
    T, active, rhs = call(b, t)
    ref = np.zeros((B, K, n))
    for i in range(n):
        e = np.zeros((B, n + ne + ni))
        e[:, i] = 1.0
        r.solve()
        r.backward(e, *BW)
        J = r.backward_results(-1)
        for name in NAMES:
            d = full(t, name, B, K, n, ne, ni)
            ref[:, :, i] += np.einsum("be,bke->bk", J["dL_d" + name].reshape(B, -1), d.reshape(B, K, -1))
    bc.gate(T[..., :n], ref, 1e-6, what + " T_x vs adjoint identity")
    # T_y, T_z against the numpy KKT solve
    b.solve()
    ld = ld_of(rhs, active, t, n, ne)
    ref = np.stack([kkt_numpy(b, q, ld[q], active[q], BW[1], BW[2]) for q in range(B)])
    T2, active2, _ = call(b, t)
    assert np.array_equal(T2, T) and np.array_equal(active2, active)
    bc.gate(T, ref, KKT_GATE, what + " T vs numpy KKT solve")
    on = np.broadcast_to((active != 0)[:, None, :], T[..., n + ne:].shape)
    assert np.all(T[..., n + ne:][~on] == 0.0)
    b.close()
    r.close()


# ---- 4. every kernel instance --------------------------------------------------------------------------------------------------
def both_checks(lib, model, what, K=2, expect_threads=None, env=None, **kwargs):
    """z-free tangents against backward_multi with the preconditioner on, the full set with it off"""
    B, n = model[1].shape
    ne = 0 if model[2] is None else model[2].shape[1]
    ni = 0 if model[4] is None else model[4].shape[1]
    names = tuple(k for k in NAMES if not (ne == 0 and k in "Ab") and not (ni == 0 and k in "Clu"))
    for precond in (True, False):
        if env:
            env[0].setenv(*env[1])
        b, r = solved(lib, model, precond=precond, **kwargs), solved(lib, model, precond=precond, **kwargs)
        if env:
            env[0].delenv(env[1][0])
        if expect_threads:
            assert b.launch_config()[0] == expect_threads
        t = random_tangents(B, K, n, ne, ni, names=tuple(k for k in names if k in "HgAb") if precond else names)
        T, active, rhs = call(b, t)
        gate_vs_backward(T, active, r, ld_of(rhs, active, t, n, ne), n, ne,
                         "%s, %s" % (what, "z-free, equilibrated" if precond else "full set, identity equilibration"))
        b.close()
        r.close()


def case_width(lib, randqp, n, ne, ni, B, K, threads):
    model = bc.model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2))
    both_checks(lib, model, "%d threads" % threads, K=K, expect_threads=threads)


def case_hbm_forced(lib, randqp, monkeypatch):
    model = default_model(randqp, B=3)
    both_checks(lib, model, "HBM form", K=3, expect_threads=1024, env=(monkeypatch, ("PQP_FORCE_HBM_VECTORS", "1")))


def case_diag_structure(lib, randqp, n=12, B=3):
    from proxsuite_amd._ctypes_defs import HessianType
    H, g, Cm, l, u = np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, n))
    for s in range(B):
        randqp.set_seed(s)
        m = randqp.dense_box_constrained_qp(n, 0, n, 0.15, 1e-2)
        H[s] = np.diag(np.diag(m.H))
        g[s], Cm[s], l[s], u[s] = m.g, m.C, m.l, m.u
    both_checks(lib, (H, g, None, None, Cm, l, u), "diagonal structure", K=3, hessian_type=int(HessianType.Diagonal))


# ---- 5. addressing, state, errors ----------------------------------------------------------------------------------------------
def case_addressing(lib, randqp):
    B, n, ne, ni, K = 6, 10, 4, 7, 5
    ntot = n + ne + ni
    model = default_model(randqp)
    b, r = solved(lib, model, precond=False), solved(lib, model, precond=False)
    t = random_tangents(B, K, n, ne, ni)
    whole, active_whole, _ = call(b, t)
    # a range in the middle of the batch, into a prefilled buffer of the whole batch
    out, flags = np.full((B, K, ntot), 7.25), np.full((B, ni), -3, dtype=np.int32)
    part = {k: np.ascontiguousarray(v[2:5]) for k, v in t.items()}
    b.solve()
    b.tangent_multi(*BW, first=2, count=3, into=(out[2:5], flags[2:5]), **kw(part))
    assert np.all(out[:2] == 7.25) and np.all(out[5:] == 7.25) and np.all(flags[:2] == -3) and np.all(flags[5:] == -3)
    assert np.array_equal(out[2:5], whole[2:5]) and np.array_equal(flags[2:5], active_whole[2:5])
    # the subset form, shuffled: slot i belongs to QP idx[i]
    idx = [4, 0, 5, 2]
    sub = {k: np.ascontiguousarray(v[idx]) for k, v in t.items()}
    b.solve()
    T, active, rhs = call(b, sub, idx=idx)
    assert np.array_equal(T, whole[idx]) and np.array_equal(active, active_whole[idx])
    gate_vs_backward(T, active, r, ld_of(rhs, active, sub, n, ne), n, ne, "subset", idx=idx)
    # K = 1 equals row 0 of K = 5
    b.solve()
    one = {k: np.ascontiguousarray(v[:, :1]) for k, v in t.items()}
    T1, a1, _ = call(b, one)
    assert np.array_equal(T1[:, 0], whole[:, 0]) and np.array_equal(a1, active_whole)
    b.close()
    r.close()


def case_state(lib, randqp):
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    model = default_model(randqp, B=B)
    b, r, third = solved(lib, model), solved(lib, model), solved(lib, model)
    t = random_tangents(B, K, n, ne, ni)
    # the tangent call ALONE on b, backward() alone on r: the state each leaves behind
    call(b, t)
    r.backward(np.ones((B, n + ne + ni)), *BW)
    ib, ir = b.results()[5], r.results()[5]
    for i in range(B):
        assert (ib[i].rho, ib[i].mu_eq, ib[i].mu_in) == (ir[i].rho, ir[i].mu_eq, ir[i].mu_in) == (BW[1], BW[2], BW[2]), i
    b.solve()
    r.solve()
    rb, rr = b.results(), r.results()
    for k in range(3):
        assert np.array_equal(rb[k], rr[k]), "xyz"[k]
    for i in range(B):
        for f in ("iter", "iter_ext", "mu_updates", "rho_updates", "status", "rho", "mu_eq", "mu_in"):
            assert getattr(rb[5][i], f) == getattr(rr[5][i], f), (i, f)
    # on a third handle: a backward() behind a tangent call (what a jvp followed by a backward does) gives the jacobians of a
    # backward() behind the solve (r, solved again above), bit for bit
    call(third, t)
    third.backward(np.ones((B, n + ne + ni)), *BW)
    r.backward(np.ones((B, n + ne + ni)), *BW)
    jt, jr = third.backward_results(-1), r.backward_results(-1)
    for name in jr:
        assert np.array_equal(jt[name], jr[name]), name
    third.close()
    b.close()
    r.close()


def case_errors(lib, randqp):
    L = lib.L
    DP, IP, I64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    INVALID, UNSUPPORTED = -1, -4
    none7 = (None,) * 7
    boxed = N.Batch(2, 4, 0, 2, box_constraints=True, lib=lib)
    buf = np.zeros(2 * 3 * 10)
    assert L.pqp_batch_tangent_multi(boxed._h, 0, 2, 1, *none7, 0, *BW, buf.ctypes.data_as(DP), None, None) == UNSUPPORTED
    boxed.close()
    B, n, ne, ni, K = 3, 10, 4, 7, 2
    ntot = n + ne + ni
    b = solved(lib, default_model(randqp, B=B))
    dg, out = np.ones((B, K, n)), np.full((B, K, ntot), 7.25)
    flags = np.full((B, ni), -3, dtype=np.int32)
    pg, po, pf = dg.ctypes.data_as(DP), out.ctypes.data_as(DP), flags.ctypes.data_as(IP)
    t = lambda: (None, pg, None, None, None, None, None, 0)
    dup = np.array([1, 1], dtype=np.int64)
    assert L.pqp_batch_tangent_multi_subset(b._h, dup.ctypes.data_as(I64), 2, K, *t(), *BW, po, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi_subset(b._h, None, 2, K, *t(), *BW, po, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi(b._h, 0, B, K, *t(), *BW, None, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi(b._h, 0, B, -1, *t(), *BW, po, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi(b._h, 0, B, 1 << 61, *t(), *BW, po, pf, None) == INVALID  # (the size overflows)
    assert L.pqp_batch_tangent_multi(b._h, 1, B, K, *t(), *BW, po, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi(b._h, -1, 1, K, *t(), *BW, po, pf, None) == INVALID
    assert L.pqp_batch_tangent_multi(None, 0, B, K, *t(), *BW, po, pf, None) == INVALID
    x0 = b.results()[0].copy()
    assert L.pqp_batch_tangent_multi(b._h, 0, B, 0, *t(), *BW, po, pf, None) == 0
    assert L.pqp_batch_tangent_multi(b._h, 0, 0, K, *t(), *BW, po, pf, None) == 0
    assert np.all(out == 7.25) and np.all(flags == -3)
    info = b.results()[5]
    assert all(info[i].rho != BW[1] for i in range(B)) and np.array_equal(b.results()[0], x0)  # (nothing ran)
    # all tangents null: zeros
    assert L.pqp_batch_tangent_multi(b._h, 0, B, K, *none7, 0, *BW, po, pf, None) == 0
    assert np.all(out == 0.0) and np.all(flags >= 0)
    T, _ = b.tangent_multi(*BW, n_dir=3)
    assert T.shape == (B, 3, ntot) and np.all(T == 0.0)
    b.close()
    # a dual infeasible QP in the range (the instance of backward_multi_cases.case_errors)
    H, g = np.diag([1.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0])
    Cm, l, u = np.array([[1.0, 0.0, 0.0]]), np.array([-np.inf]), np.array([1.0])
    d = N.Batch(2, 3, 0, 1, lib=lib)
    bc._settings(d, eps_abs=EPS, eps_rel=0)
    d.init(0, H + np.diag([0.0, 0.0, 1.0]), g, None, None, Cm, l, u)
    d.init(1, H, g, None, None, Cm, l, u)
    d.solve()
    from proxsuite_amd._ctypes_defs import QPSolverOutput
    assert d.results(1)[5].status == QPSolverOutput.PROXQP_DUAL_INFEASIBLE
    with pytest.raises(ValueError, match="not feasible"):
        d.tangent_multi(*BW, dg=np.ones((2, 1, 3)))
    T, _ = d.tangent_multi(*BW, dg=np.ones((1, 1, 3)), first=0, count=1)  # (the feasible QP alone is served)
    assert np.all(np.isfinite(T))
    d.close()


# ---- 6. facades ------------------------------------------------------------------------------------------------------------------
def case_dense_facade(lib, randqp, monkeypatch):
    from proxsuite_amd.proxqp import dense
    n, ne, ni, K = 10, 4, 7, 5
    model = default_model(randqp, B=1)
    monkeypatch.setattr(N, "_lib", lib)  # (the library `load()` hands out: the emulator's in the CPU suite)
    qp = dense.QP(n, ne, ni)
    qp.settings.eps_abs = EPS
    qp.settings.eps_rel = 0
    qp.init(*(v[0] for v in model), compute_preconditioner=False)
    qp.solve()
    qp.solve()
    dense.compute_backward(qp, np.ones(n + ne + ni), *BW)
    before = {k: np.array(getattr(qp.model.backward_data, k)) for k in ("dL_dH", "dL_dg", "dL_db")}
    qp.solve()
    t = random_tangents(1, K, n, ne, ni)
    r = solved(lib, model, precond=False)
    b = solved(lib, model, precond=False)
    T, active, rhs = call(b, t)
    many = dense.compute_forward_sensitivity(qp, *(t[k][0] for k in NAMES), *BW)
    assert many["dx"].shape == (K, n) and many["dy"].shape == (K, ne) and many["dz"].shape == (K, ni)
    assert many["active"].shape == (ni,)
    got = np.concatenate([many["dx"], many["dy"], many["dz"]], axis=1)[None]
    gate_vs_backward(got, many["active"][None], r, ld_of(rhs, active, t, n, ne), n, ne, "dense facade, K directions")
    qp.solve()
    one = dense.compute_forward_sensitivity(qp, *(t[k][0, 0] for k in NAMES), *BW)
    assert one["dx"].shape == (n,) and one["dy"].shape == (ne,) and one["dz"].shape == (ni,)
    assert np.array_equal(one["dx"], many["dx"][0]) and np.array_equal(one["dz"], many["dz"][0])
    qp.solve()
    some = dense.compute_forward_sensitivity(qp, dg=t["g"][0, 0], du=t["u"][0, 0], eps=BW[0], rho=BW[1], mu=BW[2])
    assert some["dx"].shape == (n,) and np.all(np.isfinite(some["dx"]))
    for k, v in before.items():  # qp.model.backward_data is left alone
        assert np.array_equal(np.array(getattr(qp.model.backward_data, k)), v), k
    b.close()
    r.close()


# ---- GPU only --------------------------------------------------------------------------------------------------------------------
def case_rocm_tensors(lib, randqp):
    import torch
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    b = solved(lib, default_model(randqp, B=B))
    t = random_tangents(B, K, n, ne, ni)
    T, active, rhs = call(b, t)
    b.solve()
    dev = {k: torch.from_numpy(v).to("cuda") for k, v in t.items()}
    rt = torch.zeros((B, K, n + ne + ni), dtype=torch.float64, device="cuda")
    Tt, at = b.tangent_multi(*BW, rhs=rt, **kw(dev))
    assert Tt.is_cuda and at.is_cuda and at.dtype == torch.int32
    assert np.array_equal(Tt.cpu().numpy(), T) and np.array_equal(at.cpu().numpy(), active) and np.array_equal(rt.cpu().numpy(), rhs)
    b.solve()
    Th, ah = b.tangent_multi(*BW, **{k: torch.from_numpy(v) for k, v in kw(t).items()})
    assert not Th.is_cuda and np.array_equal(Th.numpy(), T) and np.array_equal(ah.numpy(), active)
    b.close()


def case_torch_helper(lib, randqp, device="cuda"):
    import torch
    from proxsuite_amd.torch import qplayer
    B, n, ne, ni = 3, 6, 2, 4
    model = default_model(randqp, B=B, n=n, ne=ne, ni=ni)
    t = random_tangents(B, 1, n, ne, ni)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = qplayer.solution_tangents(*(dev(v) for v in model), *(dev(t[k][:, 0]) for k in NAMES), eps=EPS,
                                    eps_backward=BW[0], rho_backward=BW[1], mu_backward=BW[2])
    assert len(out) == 6 and all(o.device.type == device for o in out)
    # the same QPs through _native with the settings qplayer gives its handle
    from proxsuite_amd._ctypes_defs import InitialGuess
    b = N.Batch(B, n, ne, ni, lib=lib)
    b.set_all_settings(primal_infeasibility_solving=0, max_iter=1000, max_iter_in=100, default_rho=5.0e-5,
                       refactor_rho_threshold=5.0e-5, eps_abs=EPS, initial_guess=int(InitialGuess.EQUALITY_CONSTRAINED_INITIAL_GUESS))
    b.init(-1, *model, rho=5.0e-5)
    b.solve()
    T, active, _ = call(b, t)
    x, y, z = b.results()[:3]
    got = torch.cat(out[3:], dim=1).cpu().numpy()
    bc.gate(torch.cat(out[:3], dim=1).cpu().numpy(), np.concatenate([x, y, z], axis=1), 1e-10, "solution_tangents (x, y, z)")
    bc.gate(got, T[:, 0], 1e-10, "solution_tangents vs _native")
    b.close()


def case_forward_ad(randqp, shared_matrices, device="cuda"):
    import torch
    import torch.autograd.forward_ad as fwAD
    from proxsuite_amd.torch import qplayer
    B, n, ne, ni = 3, 6, 2, 4
    model = list(default_model(randqp, B=B, n=n, ne=ne, ni=ni))
    t = random_tangents(B, 1, n, ne, ni, shared=("H", "A", "C") if shared_matrices else ())
    tang = [t[k][0] if (shared_matrices and k in "HAC") else t[k][:, 0] for k in NAMES]
    if shared_matrices:
        for k in (0, 2, 4):
            model[k] = model[k][0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    prim, tang = [dev(v) for v in model], [dev(v) for v in tang]
    kwargs = dict(eps=EPS, eps_backward=BW[0], rho_backward=BW[1], mu_backward=BW[2])
    ref = qplayer.solution_tangents(*prim, *tang, **kwargs)
    fn = qplayer.QPFunction(structural_feasibility=True, **kwargs)
    weights = [torch.from_numpy(np.random.default_rng(3 + k).standard_normal(tuple(r.shape))).to(device) for k, r in enumerate(ref[:3])]

    def grads(dual):
        leaves = [p.clone().requires_grad_(True) for p in prim]
        if dual:
            with fwAD.dual_level():
                outs = fn(*[fwAD.make_dual(p, d) for p, d in zip(leaves, tang)])
                unpacked = [fwAD.unpack_dual(o) for o in outs]
                tangents = [u.tangent.detach().clone() for u in unpacked]
                loss = sum((u.primal * w).sum() for u, w in zip(unpacked, weights))
                g = torch.autograd.grad(loss, leaves, allow_unused=True)
        else:
            tangents = None
            outs = fn(*leaves)
            g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, weights)), leaves, allow_unused=True)
        return tangents, g
    tangents, g_dual = grads(True)
    for name, got, want in zip(("dx", "dy", "dz"), tangents, ref[3:]):
        assert got.dtype == prim[0].dtype
        bc.gate(got.cpu().numpy(), want.cpu().numpy(), 1e-10, "forward_ad %s vs solution_tangents" % name)
    _, g_plain = grads(False)
    for k, (a, bb) in enumerate(zip(g_dual, g_plain)):
        assert (a is None) == (bb is None) and (a is None or torch.equal(a, bb)), "gradient of %s after jvp" % NAMES[k]

"""Cases of the backward pass for K loss derivatives per QP (pqp_batch_backward_multi, Solver::backward_multi), shared by
tests/test_emu_backward_multi.py (CPU emulator) and tests/test_gpu_backward_multi.py (MI355X).

Settings of every case unless it says otherwise: forward eps_abs = 1e-9, eps_rel = 0; backward (eps, rho, mu) =
(1e-5, 1e-7, 1e-7), as tests/parity_cases.py::case_backward.

Gates.
  vs single: max |got - ref| <= 1e-10 (1 + max |ref|), the project's gate for two kernels of one algorithm
             (tests/parity_cases.py).  `ref` is the untouched single-row path (pqp_batch_backward*) on a SECOND handle with
             the same init + solve, re-solved before every single call.  The number of entries that are not bit-identical is
             printed, not asserted (the rows go one after the other through the same iterative_solve: zero is expected).
  vs oracle: 1e-6 (1 + max |ref|), the gate of case_backward.
  matrices : dL_dH, dL_dA, dL_dC rebuilt in numpy from a row V and (x, y, z) against the single path's: two products and
             one sum per entry, each within one rounding whether the compiler contracts them or not: 1e-13 (1 + max |ref|).
"""
import numpy as np
import pytest

from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import HessianType

EPS = 1e-9
BW = (1e-5, 1e-7, 1e-7)
LDS_OF_A_CU = 160 * 1024


def _settings(b, **kw):
    for i in range(b.B):
        s = b.settings(i)
        for k, v in kw.items():
            setattr(s, k, v)


def solved_batch(lib, model, **kw):
    """a handle with the model of `model` = (H, g, A, b, C, l, u) ([B, ...] arrays, None for absent blocks), solved"""
    H, g, A, bb, Cm, l, u = model
    B, n = g.shape
    ne = 0 if A is None else A.shape[1]
    ni = 0 if Cm is None else Cm.shape[1]
    b = N.Batch(B, n, ne, ni, lib=lib, **kw)
    _settings(b, eps_abs=EPS, eps_rel=0)
    b.init(-1, H, g, A, bb, Cm, l, u)
    b.solve()
    return b


def model_of(m):
    return (m.H, m.g, m.A if m.A.shape[1] else None, m.b if m.A.shape[1] else None, m.C if m.C.shape[1] else None,
            m.l if m.C.shape[1] else None, m.u if m.C.shape[1] else None)


def mirrored(model):
    """C -> -C, l = -u, u = 1e20: the same feasible set, every constraint that was active from above now from below"""
    H, g, A, bb, Cm, l, u = model
    return H, g, A, bb, -Cm, -u, np.full_like(u, 1e20)


def random_rows(B, K, n, ne, ni, dual_rows, seed=5):
    """K loss derivatives per QP: every row has an x part, the last `dual_rows` of them y and z parts as well"""
    rng = np.random.default_rng(seed)
    ld = np.zeros((B, K, n + ne + ni))
    ld[:, :, :n] = rng.standard_normal((B, K, n))
    if dual_rows:
        ld[:, K - dual_rows:, n:] = rng.standard_normal((B, dual_rows, ne + ni))
    return ld


def derive(V, active, n, ne):
    """the vector-shaped jacobians from rows V [..., K, ntot] and flags [..., n_in]"""
    Vz = V[..., n + ne:]
    up, low = ((active & 1) != 0)[..., None, :], ((active & 2) != 0)[..., None, :]
    return dict(dL_dg=V[..., :n], dL_db=-V[..., n:n + ne], dL_du=np.where(up, -Vz, 0.0), dL_dl=np.where(low, -Vz, 0.0))


def single_path(ref_batch, ld, first=None, idx=None):
    """the untouched single-row path on `ref_batch`: one solve + one backward launch per row k; dict name -> [rows, K, ...]"""
    K = ld.shape[1]
    out = {}
    for k in range(K):
        ref_batch.solve()
        row = np.ascontiguousarray(ld[:, k])
        if idx is not None:
            ref_batch.backward_subset(idx, row, *BW)
            sel = list(idx)
        elif first is not None:
            ref_batch.backward(row, *BW, first=first, count=ld.shape[0])
            sel = list(range(first, first + ld.shape[0]))
        else:
            ref_batch.backward(row, *BW)
            sel = list(range(ref_batch.B))
        res = ref_batch.backward_results(-1)
        for name, v in res.items():
            out.setdefault(name, []).append(v[sel])
    return {name: np.stack(v, axis=1) for name, v in out.items()}


def gate(got, ref, rel, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    diff = float(np.max(np.abs(got - ref)))
    bound = rel * (1 + float(np.max(np.abs(ref))))
    print("%s: max |difference| %.3e (gate %.3e), %d of %d entries not bit-identical"
          % (what, diff, bound, int(np.count_nonzero(got != ref)), ref.size))
    assert np.all(np.isfinite(got)), what
    assert diff <= bound, (what, diff, bound)


def gate_vs_single(V, active, ref, n, ne, what):
    for name, v in derive(V, active, n, ne).items():
        gate(v, ref[name], 1e-10, "%s %s vs single" % (what, name))


def oracle_rows(oracle, model, ld, qps=None):
    """the oracle's compute_backward for every QP and row: dict name -> [B, K, ...]"""
    H, g, A, bb, Cm, l, u = model
    B, K = ld.shape[:2]
    n = g.shape[1]
    ne = 0 if A is None else A.shape[1]
    ni = 0 if Cm is None else Cm.shape[1]
    out = {}
    for i in (range(B) if qps is None else qps):
        q = oracle.QP(n, ne, ni)
        q.settings.eps_abs = EPS
        q.settings.eps_rel = 0
        q.init(H[i], g[i], None if A is None else A[i], None if A is None else bb[i], None if Cm is None else Cm[i],
               None if Cm is None else l[i], None if Cm is None else u[i])
        rows = {}
        for k in range(K):
            q.solve()
            for name, v in q.compute_backward(ld[i, k], *BW).items():
                rows.setdefault(name, []).append(np.array(v))
        for name, v in rows.items():
            out.setdefault(name, []).append(np.stack(v))
    return {name: np.stack(v) for name, v in out.items()}


# ---- 1. rows equal single calls ----------------------------------------------------------------------------------------------
def case_rows_equal_single(lib, randqp, mirror=False):
    B, n, ne, ni, K = 6, 10, 4, 7, 5
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    if mirror:
        model = mirrored(model)
    ld = random_rows(B, K, n, ne, ni, dual_rows=3)
    b, r = solved_batch(lib, model), solved_batch(lib, model)
    x, y, z = b.results()[:3]
    V, active = b.backward_multi(ld, *BW)
    assert V.shape == (B, K, n + ne + ni) and active.shape == (B, ni) and active.dtype == np.int32
    # the condition of the case: every QP has an active and an inactive inequality
    n_active = np.count_nonzero(active, axis=1)
    print("active inequalities per QP:", n_active.tolist(), "flags:", sorted(set(active.ravel().tolist())))
    assert np.all(n_active >= 1) and np.all(n_active < ni), n_active
    if mirror:
        assert np.any(active & 2), "the mirrored batch must have constraints active from below"
    else:
        assert np.any(active & 1)
    ref = single_path(r, ld)
    what = "mirrored" if mirror else "plain"
    gate_vs_single(V, active, ref, n, ne, what)
    Vx, Vy, Vz = V[..., :n], V[..., n:n + ne], V[..., n + ne:]
    X, Y, Z = x[:, None, :], y[:, None, :], z[:, None, :]
    dH = 0.5 * (Vx[..., :, None] * X[..., None, :] + X[..., :, None] * Vx[..., None, :])
    dA = Vy[..., :, None] * X[..., None, :] + Y[..., :, None] * Vx[..., None, :]
    dC = Vz[..., :, None] * X[..., None, :] + Z[..., :, None] * Vx[..., None, :]
    gate(dH, ref["dL_dH"], 1e-13, what + " dL_dH rebuilt")
    gate(dA, ref["dL_dA"], 1e-13, what + " dL_dA rebuilt")
    gate(dC, ref["dL_dC"], 1e-13, what + " dL_dC rebuilt")
    b.close()
    r.close()
    return V, active


# ---- 2. the full Jacobian --------------------------------------------------------------------------------------------------
def case_full_jacobian(lib, oracle, randqp, monkeypatch):
    n, ne, ni = 10, 5, 2
    randqp.set_seed(1)
    m = randqp.dense_strongly_convex_qp(n, ne, ni, 0.85, 1e-1)
    # the oracle loop of tests/test_oracle_backward.py
    q = oracle.QP(n, ne, ni)
    q.settings.eps_abs = EPS
    q.settings.eps_rel = 0
    q.init(m.H, m.g, m.A, m.b, m.C, m.l, m.u)
    q.solve()
    dx_dg, dx_db = np.zeros((n, n)), np.zeros((n, ne))
    for i in range(n):
        e = np.zeros(n + ne + ni)
        e[i] = 1.0
        bd = q.compute_backward(e, *BW)
        dx_dg[i], dx_db[i] = bd["dL_dg"], bd["dL_db"]
    # the handle: K = n identity rows
    b = solved_batch(lib, tuple(v[None] for v in (m.H, m.g, m.A, m.b, m.C, m.l, m.u)))
    ld = np.zeros((1, n, n + ne + ni))
    ld[0, :, :n] = np.eye(n)
    V, active = b.backward_multi(ld, *BW)
    got = derive(V[0], active[0], n, ne)
    gate(got["dL_dg"], dx_dg, 1e-6, "handle dx_dg vs oracle")
    gate(got["dL_db"], dx_db, 1e-6, "handle dx_db vs oracle")
    b.close()
    # dense.solution_jacobians on a dense.QP
    from proxsuite_amd.proxqp import dense
    monkeypatch.setattr(N, "_lib", lib)  # (the library `load()` hands out: the emulator's in the CPU suite)
    qp = dense.QP(n, ne, ni)
    qp.settings.eps_abs = EPS
    qp.settings.eps_rel = 0
    qp.init(m.H, m.g, m.A, m.b, m.C, m.l, m.u)
    qp.solve()
    before = {k: np.array(getattr(qp.model.backward_data, k)) for k in ("dL_dH", "dL_dg", "dL_db")}
    J = dense.solution_jacobians(qp, *BW)
    assert J["dx_dg"].shape == (n, n) and J["dx_db"].shape == (n, ne)
    assert J["dx_du"].shape == (n, ni) and J["dx_dl"].shape == (n, ni)
    gate(J["dx_dg"], dx_dg, 1e-6, "dense dx_dg vs oracle")
    gate(J["dx_db"], dx_db, 1e-6, "dense dx_db vs oracle")
    for k, v in before.items():  # qp.model.backward_data is left alone
        assert np.array_equal(np.array(getattr(qp.model.backward_data, k)), v), k
    qp.solve()
    r = dense.compute_backward_multi(qp, ld[0, :3], *BW)
    assert r["vectors"].shape == (3, n + ne + ni) and r["active"].shape == (ni,)
    gate(r["dL_dg"], dx_dg[:3], 1e-6, "dense compute_backward_multi dL_dg vs oracle")


# ---- 3. every workgroup width ------------------------------------------------------------------------------------------------
WIDTHS = [(264, 8, 12, 2, 3, 512), (520, 8, 12, 1, 2, 1024)]


def case_width(lib, randqp, n, ne, ni, B, K, threads):
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2))
    b, r = solved_batch(lib, model), solved_batch(lib, model)
    assert b.launch_config()[0] == threads
    ld = random_rows(B, K, n, ne, ni, dual_rows=1)
    V, active = b.backward_multi(ld, *BW)
    gate_vs_single(V, active, single_path(r, ld), n, ne, "%d threads" % threads)
    b.close()
    r.close()


# ---- 4. per-QP vectors in HBM ------------------------------------------------------------------------------------------------
def case_hbm_forced(lib, oracle, randqp, monkeypatch):
    B, n, ne, ni, K = 3, 10, 4, 7, 4
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    ld = random_rows(B, K, n, ne, ni, dual_rows=2)
    lds_form = solved_batch(lib, model)
    ref = single_path(lds_form, ld)
    lds_form.close()
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    b = solved_batch(lib, model)
    monkeypatch.delenv("PQP_FORCE_HBM_VECTORS")
    assert b.launch_config()[0] == 1024
    V, active = b.backward_multi(ld, *BW)
    gate_vs_single(V, active, ref, n, ne, "HBM form")
    # backward() + backward_results() on such a handle: all seven jacobians vs the oracle
    orc = oracle_rows(oracle, model, ld[:, K - 1:])
    b.solve()
    b.backward(np.ascontiguousarray(ld[:, K - 1]), *BW)
    got = b.backward_results(-1)
    assert sorted(got) == sorted(orc)
    for name, v in orc.items():
        gate(got[name], v[:, 0], 1e-6, "HBM form backward() %s vs oracle" % name)
    b.close()


def case_hbm_real_shape(lib, oracle, randqp, n=400, ne=150, ni=600, B=2, K=2):
    """(400, 150, 600): 168 824 bytes of per-QP vectors, above the 163 840 of a CU's LDS ((380, 140, 560) has 160 224 and
    stays in LDS).  The rows have an x part only: with 600 inequalities the reference's repeated delta_in scaling of a
    z part (delta_in[a] ** (n_in - i)) leaves numbers of the order 1e80, against which nothing is checked.  Every row is
    gated on its own."""
    probe = N.Batch(1, n, ne, ni, lib=lib)
    lds = probe.launch_config()[1]
    probe.close()
    print("lds_bytes of (%d, %d, %d): %d" % (n, ne, ni, lds))
    assert lds > LDS_OF_A_CU, "shape does not take the HBM-vector form: %d bytes" % lds
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2))
    ld = random_rows(B, K, n, ne, ni, dual_rows=0)
    b = solved_batch(lib, model)
    V, active = b.backward_multi(ld, *BW)
    orc = oracle_rows(oracle, model, ld)
    for name, v in derive(V, active, n, ne).items():
        for k in range(K):
            gate(v[:, k], orc[name][:, k], 1e-6, "large shape backward_multi row %d %s vs oracle" % (k, name))
    b.solve()
    b.backward(np.ascontiguousarray(ld[:, 0]), *BW)
    got = b.backward_results(-1)
    for name, v in orc.items():
        gate(got[name], v[:, 0], 1e-6, "large shape backward() %s vs oracle" % name)
    b.close()


# ---- 5. the diagonal-structure branch ----------------------------------------------------------------------------------------
def case_diag_structure(lib, randqp, n=12, B=3, K=3):
    """a batch built as the C5-like batches of tests/parity_cases.py: diagonal Hessian type, no equalities, one variable
    per inequality row (C = I)"""
    H, g, Cm, l, u = np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, n, n)), np.zeros((B, n)), np.zeros((B, n))
    for s in range(B):
        randqp.set_seed(s)
        m = randqp.dense_box_constrained_qp(n, 0, n, 0.15, 1e-2)
        H[s] = np.diag(np.diag(m.H))
        g[s], Cm[s], l[s], u[s] = m.g, m.C, m.l, m.u
    model = (H, g, None, None, Cm, l, u)
    kw = dict(hessian_type=int(HessianType.Diagonal))
    b, r = solved_batch(lib, model, **kw), solved_batch(lib, model, **kw)
    ld = random_rows(B, K, n, 0, n, dual_rows=1)
    V, active = b.backward_multi(ld, *BW)
    print("active flags:", active.tolist())
    gate_vs_single(V, active, single_path(r, ld), n, 0, "diagonal structure")
    b.close()
    r.close()


# ---- 6. addressing -----------------------------------------------------------------------------------------------------------
def case_addressing(lib, randqp):
    B, n, ne, ni, K = 6, 10, 4, 7, 2
    ntot = n + ne + ni
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    ld = random_rows(B, K, n, ne, ni, dual_rows=1)
    b, r = solved_batch(lib, model), solved_batch(lib, model)
    # a range in the middle of the batch, into a prefilled buffer of the whole batch: the other rows stay as they were
    out, flags = np.full((B, K, ntot), 7.25), np.full((B, ni), -3, dtype=np.int32)
    b.backward_multi(ld[2:5], *BW, first=2, count=3, into=(out[2:5], flags[2:5]))
    assert np.all(out[:2] == 7.25) and np.all(out[5:] == 7.25) and np.all(flags[:2] == -3) and np.all(flags[5:] == -3)
    gate_vs_single(out[2:5], flags[2:5], single_path(r, ld[2:5], first=2), n, ne, "range")
    # the subset form, shuffled: slot i belongs to QP idx[i]
    idx = [4, 0, 5, 2]
    b.solve()
    V, active = b.backward_multi(ld[idx], *BW, idx=idx)
    gate_vs_single(V, active, single_path(r, ld[idx], idx=idx), n, ne, "subset")
    # K = 1 equals backward() on the same QP
    b.solve()
    r.solve()
    V1, a1 = b.backward_multi(ld[3:4, :1], *BW, first=3, count=1)
    r.backward(ld[3, :1], *BW, first=3, count=1)
    one = r.backward_results(3)
    for name, v in derive(V1[0], a1[0], n, ne).items():
        gate(v[0], one[name], 1e-10, "K = 1 %s vs backward()" % name)
    b.close()
    r.close()


# ---- 7. the state left behind ------------------------------------------------------------------------------------------------
def case_state(lib, randqp):
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    ld = random_rows(B, K, n, ne, ni, dual_rows=1)
    b, r = solved_batch(lib, model), solved_batch(lib, model)
    b.backward_multi(ld, *BW)
    r.backward(np.ascontiguousarray(ld[:, K - 1]), *BW)
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
    b.close()
    r.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def case_errors(lib, randqp):
    import ctypes as C
    L = lib.L
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    INVALID, UNSUPPORTED = -1, -4
    boxed = N.Batch(2, 4, 0, 2, box_constraints=True, lib=lib)
    buf = np.zeros(2 * 3 * 8)
    p = buf.ctypes.data_as(DP)
    assert L.pqp_batch_backward_multi(boxed._h, 0, 2, 1, p, *BW, p, None) == UNSUPPORTED
    boxed.close()
    B, n, ne, ni, K = 3, 10, 4, 7, 2
    ntot = n + ne + ni
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    b = solved_batch(lib, model)
    ld, out = np.ones((B, K, ntot)), np.full((B, K, ntot), 7.25)
    flags = np.full((B, ni), -3, dtype=np.int32)
    pl, po, pf = ld.ctypes.data_as(DP), out.ctypes.data_as(DP), flags.ctypes.data_as(IP)
    I64 = C.POINTER(C.c_int64)
    dup = np.array([1, 1], dtype=np.int64)
    assert lib.L.pqp_batch_backward_multi_subset(b._h, dup.ctypes.data_as(I64), 2, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_multi(b._h, 0, B, K, None, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_multi(b._h, 0, B, K, pl, *BW, None, pf) == INVALID
    assert L.pqp_batch_backward_multi(b._h, 0, B, -1, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_multi(b._h, 0, B, 1 << 61, pl, *BW, po, pf) == INVALID  # (the size overflows)
    assert L.pqp_batch_backward_multi(b._h, 1, B, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_multi(b._h, -1, 1, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_multi(None, 0, B, K, pl, *BW, po, pf) == INVALID
    x0 = b.results()[0].copy()
    assert L.pqp_batch_backward_multi(b._h, 0, B, 0, pl, *BW, po, pf) == 0
    assert L.pqp_batch_backward_multi(b._h, 0, 0, K, pl, *BW, po, pf) == 0
    assert np.all(out == 7.25) and np.all(flags == -3)
    info = b.results()[5]
    assert all(info[i].rho != BW[1] for i in range(B)) and np.array_equal(b.results()[0], x0)  # (nothing ran)
    b.close()
    # a dual infeasible QP in the range (the instance of tests/parity_cases.py::case_infeasibility_statuses)
    H, g = np.diag([1.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0])
    Cm, l, u = np.array([[1.0, 0.0, 0.0]]), np.array([-np.inf]), np.array([1.0])
    d = N.Batch(2, 3, 0, 1, lib=lib)
    _settings(d, eps_abs=EPS, eps_rel=0)
    d.init(0, H + np.diag([0.0, 0.0, 1.0]), g, None, None, Cm, l, u)
    d.init(1, H, g, None, None, Cm, l, u)
    d.solve()
    from proxsuite_amd._ctypes_defs import QPSolverOutput
    assert d.results(1)[5].status == QPSolverOutput.PROXQP_DUAL_INFEASIBLE
    l2, o2 = np.ones((2, 1, 4)), np.zeros((2, 1, 4))
    with pytest.raises(ValueError, match="not feasible"):
        d.backward_multi(l2, *BW)
    assert L.pqp_batch_backward_multi(d._h, 0, 2, 1, l2.ctypes.data_as(DP), *BW, o2.ctypes.data_as(DP), None) == INVALID
    V, _ = d.backward_multi(l2[:1], *BW, first=0, count=1)  # (the feasible QP alone is served)
    assert np.all(np.isfinite(V))
    d.close()


# ---- 9. GPU only: ROCm tensors ---------------------------------------------------------------------------------------------
def case_rocm_tensors(lib, randqp):
    import torch
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    model = model_of(randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1))
    ld = random_rows(B, K, n, ne, ni, dual_rows=1)
    b = solved_batch(lib, model)
    V, active = b.backward_multi(ld, *BW)
    b.solve()
    Vt, at = b.backward_multi(torch.from_numpy(ld).to("cuda"), *BW)
    assert Vt.is_cuda and at.is_cuda and at.dtype == torch.int32
    assert np.array_equal(Vt.cpu().numpy(), V) and np.array_equal(at.cpu().numpy(), active)
    b.solve()
    Vh, ah = b.backward_multi(torch.from_numpy(ld), *BW)
    assert not Vh.is_cuda and np.array_equal(Vh.numpy(), V) and np.array_equal(ah.numpy(), active)
    b.close()


def case_torch_helper(randqp):
    import torch
    from proxsuite_amd.torch import qplayer
    B, n, ne, ni = 3, 6, 2, 4
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    Q, p, A, bb, G, l, u = (t(v) for v in (m.H, m.g, m.A, m.b, m.C, m.l, m.u))
    x, dx_dp, dx_db, dx_dl, dx_du = qplayer.solution_jacobians(Q, p, A, bb, G, l, u, eps=EPS, eps_backward=BW[0],
                                                               rho_backward=BW[1], mu_backward=BW[2])
    assert tuple(dx_dp.shape) == (B, n, n) and tuple(dx_db.shape) == (B, n, ne)
    assert tuple(dx_dl.shape) == (B, n, ni) and tuple(dx_du.shape) == (B, n, ni) and dx_dp.is_cuda
    fn = qplayer.QPFunction(eps=EPS, eps_backward=BW[0], rho_backward=BW[1], mu_backward=BW[2])
    ref = {k: [] for k in ("p", "b", "l", "u")}
    for i in range(n):
        leaves = [v.clone().requires_grad_(True) for v in (p, bb, l, u)]
        xs, _, _ = fn(Q, leaves[0], A, leaves[1], G, leaves[2], leaves[3])
        grads = torch.autograd.grad(xs[:, i].sum(), leaves)
        for k, gk in zip(("p", "b", "l", "u"), grads):
            ref[k].append(gk)
    gate(x.cpu().numpy(), xs.detach().cpu().numpy(), 1e-10, "torch helper x")
    for k, got in (("p", dx_dp), ("b", dx_db), ("l", dx_dl), ("u", dx_du)):
        gate(got.cpu().numpy(), torch.stack(ref[k], dim=1).cpu().numpy(), 1e-10, "torch helper dx/d%s vs autograd loop" % k)

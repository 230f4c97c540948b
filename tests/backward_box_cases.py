"""Cases of the backward pass for QPs with box constraints (pqp_batch_backward_box, Solver::backward_box), shared by
tests/test_emu_backward_box.py (CPU emulator) and tests/test_gpu_backward_box.py (MI355X).

Settings: forward eps_abs = 1e-9, eps_rel = 0; backward BW = (1e-5, 1e-7, 1e-7); gate(got, ref, rel) of
tests/backward_multi_cases.py: max |got - ref| <= rel (1 + max |ref|).

How a box case is made (make_case): a dense_strongly_convex_qp_batch(B, n, n_eq, n_in, 0.85, 1e-1) is solved WITHOUT box on
the oracle; about a quarter of the variables get u_box_k = x*_k - 0.1 (bound active from above), another quarter
l_box_k = x*_k + 0.1 (active from below), the rest x*_k -+ 1.  check_case asserts what every case must meet: status
SOLVED, per QP a box row active from above, one from below and one inactive (with n_in > 0 also a general row active and
one inactive), and strict complementarity by 1e-3 for every row of [C; I].  The seeds below were picked so that this holds.

The reference of the semantic gate is the oracle's compute_backward on the SAME QP stated with rows: C' = [C; I],
u' = [u; u_box], l' = [l; l_box], with compute_preconditioner = False on both sides (with identity equilibration the two
statements are the same computation; with Ruiz on their equilibrations differ, see case_ruiz)."""
import numpy as np
import pytest

from backward_multi_cases import BW, EPS, gate, solved_batch
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import DenseBackend, HessianType

SOLVED = 0
NAMES7 = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_du", "dL_dl")

# seed0 of dense_strongly_convex_qp_batch per shape (n, n_eq, n_in, hessian): chosen on the oracle and the emulator so that
# check_case holds for every QP of the case
SEEDS = {(20, 7, 9, "dense"): 0, (33, 5, 0, "dense"): 14, (70, 0, 0, "dense"): 7, (70, 0, 0, "diag"): 0,
         (12, 0, 6, "zero"): 0, (10, 3, 4, "dense"): 7, (264, 8, 12, "dense"): 28, (520, 8, 12, "dense"): 49,
         (10, 4, 7, "dense"): 2191, (561, 8, 12, "dense"): 0}


class Case:
    """H, g, A, b, C, l, u, l_box, u_box: [B, ...] arrays (A / C with zero rows when absent)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.B, self.n = self.g.shape
        self.ne, self.ni = self.A.shape[1], self.C.shape[1]
        self.nc = self.ni + self.n

    def box_model(self, sel=slice(None)):
        o = lambda a, k: a[sel] if k else None
        return dict(H=self.H[sel], g=self.g[sel], A=o(self.A, self.ne), b=o(self.b, self.ne), C=o(self.C, self.ni),
                    l=o(self.l, self.ni), u=o(self.u, self.ni), l_box=self.l_box[sel], u_box=self.u_box[sel])

    def rows_model(self):
        """the same QPs with the bounds as rows n_in .. n_in + n - 1 of C"""
        eye = np.broadcast_to(np.eye(self.n), (self.B, self.n, self.n))
        return dict(H=self.H, g=self.g, A=self.A if self.ne else None, b=self.b if self.ne else None,
                    C=np.ascontiguousarray(np.concatenate([self.C, eye], axis=1)),
                    l=np.concatenate([self.l, self.l_box], axis=1), u=np.concatenate([self.u, self.u_box], axis=1))


def make_case(oracle, randqp, B, n, ne, ni, hessian="dense", seed0=None):
    seed0 = SEEDS[(n, ne, ni, hessian)] if seed0 is None else seed0
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.85, 1e-1, seed0=seed0)
    l_box, u_box = np.zeros((B, n)), np.zeros((B, n))
    for i in range(B):
        q = oracle.QP(n, ne, ni)
        q.settings.eps_abs, q.settings.eps_rel = EPS, 0
        q.init(m.H[i], m.g[i], m.A[i] if ne else None, m.b[i] if ne else None, m.C[i] if ni else None,
               m.l[i] if ni else None, m.u[i] if ni else None)
        q.solve()
        x = q.results.x
        kind = np.arange(n) % 4  # 0: pushed down from above, 1: pushed up from below, 2 / 3: a loose interval
        u_box[i] = np.where(kind == 0, x - 0.1, x + 1.0)
        l_box[i] = np.where(kind == 1, x + 0.1, x - 1.0)
    H = m.H
    if hessian == "diag":
        H = np.ascontiguousarray(H * np.eye(n))
    elif hessian == "zero":
        H = np.zeros_like(H)
    return Case(H=H, g=m.g, A=m.A, b=m.b, C=m.C, l=m.l, u=m.u, l_box=l_box, u_box=u_box, hessian=hessian)


def hessian_kw(case):
    return {"diag": dict(hessian_type=int(HessianType.Diagonal)), "zero": dict(hessian_type=int(HessianType.Zero))}.get(
        case.hessian, {})


def box_batch(lib, case, precond=False, eps=EPS, sel=slice(None), **kw):
    """a handle with box constraints holding the QPs of `case`, solved"""
    model = case.box_model(sel)
    b = N.Batch(model["g"].shape[0], case.n, case.ne, case.ni, box_constraints=True, lib=lib, **hessian_kw(case), **kw)
    for i in range(b.B):
        s = b.settings(i)
        s.eps_abs, s.eps_rel = eps, 0
    b.init(-1, compute_preconditioner=precond, **model)
    b.solve()
    return b


def rows_batch(lib, case, precond=False, **kw):
    """the existing path: a handle WITHOUT box constraints on the row-stated QPs, solved"""
    model = case.rows_model()
    b = N.Batch(case.B, case.n, case.ne, case.nc, lib=lib, **hessian_kw(case), **kw)
    for i in range(b.B):
        s = b.settings(i)
        s.eps_abs, s.eps_rel = EPS, 0
    b.init(-1, compute_preconditioner=precond, **model)
    b.solve()
    return b


def check_case(case, b):
    """the conditions every case must meet, on the solution of the box handle `b`; returns (x, y, z)"""
    x, y, z, _, _, info = b.results()
    check_solution(case, x, z, [info[i].status for i in range(b.B)])
    return x, y, z


def check_solution(case, x, z, status):
    n, ni = case.n, case.ni
    for i in range(x.shape[0]):
        assert status[i] == SOLVED, (i, status[i])
        xb = x[i]
        rows = np.concatenate([case.C[i] @ xb, xb])
        up = np.concatenate([case.u[i], case.u_box[i]])
        lo = np.concatenate([case.l[i], case.l_box[i]])
        slack = np.minimum(up - rows, rows - lo)  # distance to the nearer bound
        zi = np.abs(z[i])
        strict = np.maximum(zi, np.abs(slack)) >= 1e-3
        both = (zi >= 1e-3) & (np.abs(slack) >= 1e-3)
        assert np.all(strict) and not np.any(both), (i, np.flatnonzero(~strict), np.flatnonzero(both))
        zb = z[i, ni:]
        assert np.any(zb >= 1e-3) and np.any(zb <= -1e-3) and np.any(np.abs(zb) < 1e-3), (i, "box rows", zb)
        if ni:
            assert np.any(zi[:ni] >= 1e-3) and np.any(zi[:ni] < 1e-3), (i, "general rows", z[i, :ni])


def random_rows(B, K, n, ne, nc, dual_rows, seed=5):
    """K loss derivatives per QP: every row has an x part, the last `dual_rows` of them y, z_in and z_box parts as well"""
    rng = np.random.default_rng(seed)
    ld = np.zeros((B, K, n + ne + nc))
    ld[:, :, :n] = rng.standard_normal((B, K, n))
    if dual_rows:
        ld[:, K - dual_rows:, n:] = rng.standard_normal((B, dual_rows, ne + nc))
    return ld


def derive(V, active, x, y, z, n, ne, ni):
    """the nine jacobians from a row V [ntot], the flags [n_c] and the solution of one QP"""
    Vx, Vy, Vz = V[:n], V[n:n + ne], V[n + ne:]
    up, low = (active & 1) != 0, (active & 2) != 0
    du, dl = np.where(up, -Vz, 0.0), np.where(low, -Vz, 0.0)
    return dict(dL_dH=0.5 * (np.outer(Vx, x) + np.outer(x, Vx)), dL_dg=Vx, dL_dA=np.outer(Vy, x) + np.outer(y, Vx),
                dL_db=-Vy, dL_dC=np.outer(Vz[:ni], x) + np.outer(z[:ni], Vx), dL_du=du[:ni], dL_dl=dl[:ni],
                dL_du_box=du[ni:], dL_dl_box=dl[ni:])


def split_rows_result(r, ni):
    """the jacobians of the row-stated QP in the names of the box form"""
    out = {k: r[k] for k in ("dL_dH", "dL_dg", "dL_dA", "dL_db")}
    out.update(dL_dC=r["dL_dC"][..., :ni, :], dL_du=r["dL_du"][..., :ni], dL_dl=r["dL_dl"][..., :ni],
               dL_du_box=r["dL_du"][..., ni:], dL_dl_box=r["dL_dl"][..., ni:])
    return out


def oracle_rows_reference(oracle, case, ld, bw=BW, dense_backend=None):
    """the oracle's compute_backward on the row-stated QPs (no preconditioner), per QP and row: a list [B][K] of dicts in
    the names of the box form, and the oracle's active sets [B, n_c] (bit 0 from above, bit 1 from below)"""
    m = case.rows_model()
    B, K = ld.shape[:2]
    kw = dict(hessian_type={"diag": HessianType.Diagonal, "zero": HessianType.Zero}.get(case.hessian, HessianType.Dense))
    if dense_backend is not None:
        kw["dense_backend"] = dense_backend
    out, flags = [], np.zeros((B, case.nc), dtype=np.int32)
    for i in range(B):
        q = oracle.QP(case.n, case.ne, case.nc, **kw)
        q.settings.eps_abs, q.settings.eps_rel = EPS, 0
        q.init(m["H"][i], m["g"][i], None if m["A"] is None else m["A"][i], None if m["b"] is None else m["b"][i],
               m["C"][i], m["l"][i], m["u"][i], compute_preconditioner=False)
        rows = []
        for k in range(K):
            q.solve()
            if k == 0:
                s = m["C"][i] @ q.results.x + q.results.z
                flags[i] = ((s - m["u"][i]) >= 0) * 1 + ((s - m["l"][i]) <= 0) * 2
            rows.append(split_rows_result({n_: np.array(v) for n_, v in q.compute_backward(ld[i, k], *bw).items()}, case.ni))
        out.append(rows)
    return out, flags


def gate_against(V, active, sol, ref, case, rel, what):
    """rows V [B, K, ntot] + flags of the box path against a [B][K] list of reference dicts"""
    x, y, z = sol
    for i in range(V.shape[0]):
        for k in range(V.shape[1]):
            got = derive(V[i, k], active[i], x[i], y[i], z[i], case.n, case.ne, case.ni)
            for name, v in ref[i][k].items():
                gate(got[name], v, rel, "%s QP %d row %d %s" % (what, i, k, name))


# ---- 1. against the oracle on the row-stated QP ------------------------------------------------------------------------------
def case_vs_oracle(lib, oracle, randqp, n=20, ne=7, ni=9, B=4, K=3, hessian="dense", dual_rows=1, threads=None,
                   expect_diag=False, **kw):
    case = make_case(oracle, randqp, B, n, ne, ni, hessian)
    b = box_batch(lib, case, **kw)
    if threads is not None:
        assert b.launch_config()[0] == threads, b.launch_config()
    sol = check_case(case, b)
    if expect_diag:
        assert b.primal_factor(0)["meta"]["diag_mode"] == 1, "the handle does not run the diagonal-structure mode"
    ld = random_rows(B, K, n, ne, case.nc, dual_rows)
    V, active = b.backward_box(ld, *BW)
    assert V.shape == (B, K, n + ne + ni + n) and active.shape == (B, ni + n) and active.dtype == np.int32
    ref, flags = oracle_rows_reference(oracle, case, ld, dense_backend=kw.get("dense_backend"))
    print("flags per QP:", [sorted(set(a.tolist())) for a in active], "active rows:", np.count_nonzero(active, axis=1).tolist())
    assert np.array_equal(active, flags), "active sets differ from the oracle's"
    gate_against(V, active, sol, ref, case, 1e-6, "box vs oracle(rows)")
    b.close()
    return case


# ---- 2. with Ruiz on -------------------------------------------------------------------------------------------------------
def kkt_truth(case, i, x, z, ld_x):
    """the unregularised KKT system of QP i on its active set, solved in numpy: (dL_dg, dL_db, dL_du', dL_dl') over the
    n_c rows of [C; I].  Unique under strict complementarity."""
    n, ne, nc = case.n, case.ne, case.nc
    Cf = np.concatenate([case.C[i], np.eye(n)])
    rows = Cf @ x + z
    up = (rows - np.concatenate([case.u[i], case.u_box[i]])) >= 0
    lo = (rows - np.concatenate([case.l[i], case.l_box[i]])) <= 0
    J = np.flatnonzero(up | lo)
    Bm = np.concatenate([case.A[i], Cf[J]])
    K0 = np.block([[case.H[i], Bm.T], [Bm, np.zeros((Bm.shape[0], Bm.shape[0]))]])
    v = np.linalg.solve(K0, -np.concatenate([ld_x, np.zeros(Bm.shape[0])]))
    vz = np.zeros(nc)
    vz[J] = v[n + ne:]
    return np.concatenate([v[:n], -v[n:n + ne], np.where(up, -vz, 0.0), np.where(lo, -vz, 0.0)])


def flat_vectors(V, active, n, ne):
    Vz = V[n + ne:]
    return np.concatenate([V[:n], -V[n:n + ne], np.where(active & 1, -Vz, 0.0), np.where(active & 2, -Vz, 0.0)])


def case_ruiz(lib, oracle, randqp, n=20, ne=7, ni=9, B=4, K=2):
    case = make_case(oracle, randqp, B, n, ne, ni)
    b, r = box_batch(lib, case, precond=True), rows_batch(lib, case, precond=True)
    x, y, z = check_case(case, b)
    ld = random_rows(B, K, n, ne, case.nc, dual_rows=0)
    V, active = b.backward_box(ld, *BW)
    Vr, ar = r.backward_multi(ld, *BW)
    assert np.array_equal(active, ar), "the two statements disagree on the active sets"
    for i in range(B):
        for k in range(K):
            truth = kkt_truth(case, i, x[i], z[i], ld[i, k, :n])
            scale = 1 + float(np.max(np.abs(truth)))
            e_box = float(np.max(np.abs(flat_vectors(V[i, k], active[i], n, ne) - truth)))
            e_rows = float(np.max(np.abs(flat_vectors(Vr[i, k], ar[i], n, ne) - truth)))
            print("QP %d row %d: e_box %.3e  e_rows %.3e  (1 + max |truth| = %.3e)" % (i, k, e_box, e_rows, scale))
            assert e_rows <= 1e-4 * scale, ("the reference path is off the truth", i, k, e_rows)
            assert e_box <= 3 * e_rows + 1e-12 * scale, (i, k, e_box, e_rows)
    b.close()
    r.close()


# ---- 3. finite differences ---------------------------------------------------------------------------------------------------
def case_finite_differences(lib, oracle, randqp):
    n, ne, ni = 10, 3, 4
    case = make_case(oracle, randqp, 1, n, ne, ni)
    w = np.random.default_rng(0).standard_normal(n)
    b = box_batch(lib, case, precond=True, eps=1e-11)
    check_case(case, b)
    ld = np.zeros((1, 1, n + ne + ni + n))
    ld[0, 0, :n] = w
    V, active = b.backward_box(ld, 1e-9, 1e-9, 1e-9)
    bd = b.backward_box_results(0)
    b.close()
    box_flags = active[0, ni:]
    print("box flags:", box_flags.tolist())

    def loss(**change):
        c = Case(**{**{k: getattr(case, k) for k in ("H", "g", "A", "b", "C", "l", "u", "l_box", "u_box", "hessian")}, **change})
        bb = box_batch(lib, c, precond=True, eps=1e-11)
        v = float(w @ bb.results()[0][0])
        bb.close()
        return v

    h = 1e-6
    pick = lambda mask: list(np.flatnonzero(mask)[:2])
    for name, key in (("u_box", "dL_du_box"), ("l_box", "dL_dl_box")):
        bit = 1 if name == "u_box" else 2
        ks = (pick(box_flags & bit) + pick(box_flags == 0))[:3]  # active rows of that side and inactive ones
        assert len(ks) == 3 and (box_flags[ks[0]] & bit) and box_flags[ks[-1]] == 0, ks
        for k in ks:
            p, m_ = getattr(case, name).copy(), getattr(case, name).copy()
            p[0, k] += h
            m_[0, k] -= h
            fd = (loss(**{name: p}) - loss(**{name: m_})) / (2 * h)
            print("d loss / d %s[%d]: fd %.9e analytic %.9e" % (name, k, fd, bd[key][k]))
            assert abs(fd - bd[key][k]) < 1e-5, (name, k, fd, bd[key][k])
    for k in (0, 1, 6):
        p, m_ = case.g.copy(), case.g.copy()
        p[0, k] += h
        m_[0, k] -= h
        fd = (loss(g=p) - loss(g=m_)) / (2 * h)
        assert abs(fd - bd["dL_dg"][k]) < 1e-5, ("g", k, fd, bd["dL_dg"][k])
    for (i, j) in [(0, 0), (1, 4), (5, 2)]:
        p, m_ = case.H.copy(), case.H.copy()
        p[0, i, j] += h
        m_[0, i, j] -= h
        if i != j:
            p[0, j, i] += h
            m_[0, j, i] -= h
        fd = (loss(H=p) - loss(H=m_)) / (2 * h)
        ref = bd["dL_dH"][i, j] + (bd["dL_dH"][j, i] if i != j else 0)
        assert abs(fd - ref) < 1e-5, ("H", i, j, fd, ref)


# ---- 4. forms ----------------------------------------------------------------------------------------------------------------
FORMS = {
    "box_only_with_equalities": dict(n=33, ne=5, ni=0, B=2, K=2),
    "box_only_dense_hessian": dict(n=70, ne=0, ni=0, B=2, K=2),
    "diagonal_structure": dict(n=70, ne=0, ni=0, B=2, K=2, hessian="diag", expect_diag=True),
    "zero_hessian": dict(n=12, ne=0, ni=6, B=2, K=2, hessian="zero"),
    "primal_ldlt": dict(n=20, ne=7, ni=9, B=2, K=2, dense_backend=int(DenseBackend.PrimalLDLT)),
}
WIDTHS = [(264, 8, 12, 2, 2, 512), (520, 8, 12, 1, 2, 1024)]


def case_form(lib, oracle, randqp, name):
    case_vs_oracle(lib, oracle, randqp, **FORMS[name])


def case_width(lib, oracle, randqp, n, ne, ni, B, K, threads):
    case_vs_oracle(lib, oracle, randqp, n=n, ne=ne, ni=ni, B=B, K=K, threads=threads)


def case_hbm_real_shape(lib, oracle, randqp):
    """(561, 8, 12) with box: the smallest shape of the (n, 8, 12) family of WIDTHS whose per-QP vectors (163 936 bytes)
    exceed the 163 840 of a CU's LDS; (560, 8, 12) has 163 696 and stays in LDS"""
    for n, beyond in ((560, False), (561, True)):
        probe = N.Batch(1, n, 8, 12, box_constraints=True, lib=lib)
        lds = probe.launch_config()[1]
        probe.close()
        assert (lds > 160 * 1024) == beyond, (n, lds)
    case_vs_oracle(lib, oracle, randqp, n=561, ne=8, ni=12, B=2, K=2, threads=1024)


def case_hbm_forced(lib, oracle, randqp, monkeypatch):
    monkeypatch.setenv("PQP_FORCE_HBM_VECTORS", "1")
    case_vs_oracle(lib, oracle, randqp, n=10, ne=4, ni=7, B=3, K=2, threads=1024)
    monkeypatch.delenv("PQP_FORCE_HBM_VECTORS")


# ---- 5. addressing, state, errors --------------------------------------------------------------------------------------------
def single_calls(r, ld, first=None, idx=None):
    """K single calls (n_rhs = 1) on the twin handle `r`, re-solved before each: rows [rows, K, ntot] and flags"""
    out = []
    for k in range(ld.shape[1]):
        r.solve()
        V, a = r.backward_box(np.ascontiguousarray(ld[:, k:k + 1]), *BW, first=first, count=None if first is None else ld.shape[0],
                              idx=idx)
        out.append(V[:, 0])
    return np.stack(out, axis=1), a


def case_addressing(lib, oracle, randqp):
    B, n, ne, ni, K = 6, 10, 4, 7, 2
    case = make_case(oracle, randqp, B, n, ne, ni)
    nc, ntot = case.nc, n + ne + case.nc
    ld = random_rows(B, K, n, ne, nc, dual_rows=1)
    b, r = box_batch(lib, case), box_batch(lib, case)
    check_case(case, b)
    # a range in the middle of the batch, into prefilled buffers of the whole batch: the other rows stay as they were
    out, flags = np.full((B, K, ntot), 7.25), np.full((B, nc), -3, dtype=np.int32)
    b.backward_box(ld[2:5], *BW, first=2, count=3, into=(out[2:5], flags[2:5]))
    assert np.all(out[:2] == 7.25) and np.all(out[5:] == 7.25) and np.all(flags[:2] == -3) and np.all(flags[5:] == -3)
    Vs, fs = single_calls(r, ld[2:5], first=2)
    gate(out[2:5], Vs, 1e-10, "range: K rows vs K single calls")
    assert np.array_equal(flags[2:5], fs)
    # the subset form, shuffled: slot i belongs to QP idx[i]
    idx = [4, 0, 5, 2]
    b.solve()
    V, active = b.backward_box(ld[idx], *BW, idx=idx)
    Vs, fs = single_calls(r, ld[idx], idx=idx)
    gate(V, Vs, 1e-10, "subset: K rows vs K single calls")
    assert np.array_equal(active, fs)
    # K = 1 fills the nine jacobians: equal to those derived from the row
    b.solve()
    V1, a1 = b.backward_box(ld[3:4, :1], *BW, first=3, count=1)
    x, y, z = b.results()[:3]
    one = b.backward_box_results(3)
    assert sorted(one) == sorted(NAMES7 + ("dL_dl_box", "dL_du_box"))
    for name, v in derive(V1[0, 0], a1[0], x[3], y[3], z[3], n, ne, ni).items():
        gate(one[name], v, 1e-10, "K = 1 %s: the n_rhs = 1 jacobians vs the row" % name)
    whole = b.backward_box_results(-1)
    assert whole["dL_dl_box"].shape == (B, n) and np.array_equal(whole["dL_du_box"][3], one["dL_du_box"])
    # out = NULL and active = NULL are served
    b.solve()
    import ctypes as C
    row = np.ascontiguousarray(ld[3:4, :1])
    assert lib.L.pqp_batch_backward_box(b._h, 3, 1, 1, row.ctypes.data_as(C.POINTER(C.c_double)), *BW, None, None) == 0
    for name, v in b.backward_box_results(3).items():
        assert np.array_equal(v, one[name]), name
    b.close()
    r.close()


def case_state(lib, oracle, randqp):
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    case = make_case(oracle, randqp, B, n, ne, ni)
    ld = random_rows(B, K, n, ne, case.nc, dual_rows=1)
    b, r = box_batch(lib, case), box_batch(lib, case)
    V, _ = b.backward_box(ld, *BW)
    Vr, _ = r.backward_box(ld, *BW)
    assert np.array_equal(V, Vr)
    ib = b.results()[5]
    for i in range(B):
        assert (ib[i].rho, ib[i].mu_eq, ib[i].mu_in) == (BW[1], BW[2], BW[2]), i
    b.solve()
    r.solve()
    rb, rr = b.results(), r.results()
    for k in range(3):
        assert np.array_equal(rb[k], rr[k]), "xyz"[k]
    for i in range(B):
        assert rb[5][i].status == SOLVED
        for f in ("iter", "iter_ext", "mu_updates", "rho_updates", "status", "rho", "mu_eq", "mu_in"):
            assert getattr(rb[5][i], f) == getattr(rr[5][i], f), (i, f)
    check_case(case, b)  # ... and the re-solve found the solution again
    b.close()
    r.close()


def case_errors(lib, oracle, randqp):
    import ctypes as C
    L = lib.L
    DP, IP, I64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    INVALID, UNSUPPORTED = -1, -4
    B, n, ne, ni, K = 3, 10, 4, 7, 2
    case = make_case(oracle, randqp, B, n, ne, ni)
    ntot, nc = n + ne + case.nc, case.nc
    b = box_batch(lib, case)
    ld, out = np.ones((B, K, ntot)), np.full((B, K, ntot), 7.25)
    flags = np.full((B, nc), -3, dtype=np.int32)
    pl, po, pf = ld.ctypes.data_as(DP), out.ctypes.data_as(DP), flags.ctypes.data_as(IP)
    # the existing entries still refuse a box handle
    assert L.pqp_batch_backward_multi(b._h, 0, B, K, pl, *BW, po, pf) == UNSUPPORTED
    assert L.pqp_batch_backward_range(b._h, 0, B, pl, *BW) == UNSUPPORTED
    assert L.pqp_batch_backward(b._h, pl, *BW) == UNSUPPORTED
    dup = np.array([1, 1], dtype=np.int64)
    assert L.pqp_batch_backward_box_subset(b._h, dup.ctypes.data_as(I64), 2, K, pl, *BW, po, pf) == INVALID
    bad = np.array([0, B], dtype=np.int64)
    assert L.pqp_batch_backward_box_subset(b._h, bad.ctypes.data_as(I64), 2, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box_subset(b._h, None, 2, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box(b._h, 0, B, K, None, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box(b._h, 0, B, -1, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box(b._h, 0, B, 1 << 61, pl, *BW, po, pf) == INVALID  # (the size overflows)
    assert L.pqp_batch_backward_box(b._h, 1, B, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box(b._h, -1, 1, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_backward_box(None, 0, B, K, pl, *BW, po, pf) == INVALID
    assert L.pqp_batch_get_backward_box(b._h, 0, None, None) == INVALID  # (no n_rhs = 1 call yet)
    x0 = b.results()[0].copy()
    assert L.pqp_batch_backward_box(b._h, 0, B, 0, pl, *BW, po, pf) == 0
    assert L.pqp_batch_backward_box(b._h, 0, 0, K, pl, *BW, po, pf) == 0
    assert np.all(out == 7.25) and np.all(flags == -3)
    info = b.results()[5]
    assert all(info[i].rho != BW[1] for i in range(B)) and np.array_equal(b.results()[0], x0)  # (nothing ran)
    # n_rhs > 1 leaves the jacobian arrays alone
    b.backward_box(ld[:, :1], *BW)
    before = b.backward_box_results(-1)
    b.solve()
    b.backward_box(2 * ld, *BW)
    after = b.backward_box_results(-1)
    for name, v in before.items():
        assert np.array_equal(after[name], v), name
    b.close()
    # a handle without box constraints is sent to the existing entries
    plain = N.Batch(2, 4, 0, 2, lib=lib)
    buf = np.zeros(2 * 3 * 12)
    p = buf.ctypes.data_as(DP)
    assert L.pqp_batch_backward_box(plain._h, 0, 2, 1, p, *BW, p, None) == INVALID
    assert b"pqp_batch_backward_multi" in L.pqp_last_error()
    plain.close()
    # A QP of a box handle initialised without bounds has them at +-infinity and no active box row.
    # (The refusal of a DUAL INFEASIBLE QP is the check of pqp_batch_backward_multi, shared code, tested in
    # tests/backward_multi_cases.py::case_errors.  It cannot be provoked here: with box constraints neither the oracle nor
    # the engine certifies dual infeasibility of an unbounded QP -- the instance of case_infeasibility_statuses, with or
    # without finite bounds on the other variables, ends at the iteration limit on both.)
    H, g = np.diag([1.0, 1.0, 1.0]), np.array([0.0, 0.0, -1.0])
    Cm, l, u = np.array([[1.0, 0.0, 0.0]]), np.array([-np.inf]), np.array([1.0])
    d = N.Batch(1, 3, 0, 1, box_constraints=True, lib=lib)
    s = d.settings(0)
    s.eps_abs, s.eps_rel = EPS, 0
    d.init(0, H, g, None, None, Cm, l, u)
    d.solve()
    assert d.results(0)[5].status == SOLVED
    V, a = d.backward_box(np.ones((1, 1, 3 + 1 + 3)), *BW)
    assert np.all(np.isfinite(V)) and not np.any(a[0, 1:]), a
    d.close()


# ---- 5b. proxqp.dense on a QP with box constraints ---------------------------------------------------------------------------
def case_dense_api(lib, oracle, randqp, monkeypatch):
    from proxsuite_amd.proxqp import dense
    monkeypatch.setattr(N, "_lib", lib)  # (the library `load()` hands out: the emulator's in the CPU suite)
    B, n, ne, ni = 3, 20, 7, 9
    case = make_case(oracle, randqp, B, n, ne, ni)
    ld = random_rows(B, 1, n, ne, case.nc, dual_rows=1)
    ref, flags = oracle_rows_reference(oracle, case, ld)

    def solved(i, box=True):
        qp = dense.QP(n, ne, ni, box)
        qp.settings.eps_abs, qp.settings.eps_rel = EPS, 0
        m = case.box_model(i)
        if box:
            qp.init(m["H"], m["g"], m["A"], m["b"], m["C"], m["l"], m["u"], m["l_box"], m["u_box"], False)
        else:
            qp.init(m["H"], m["g"], m["A"], m["b"], m["C"], m["l"], m["u"], False)
        qp.solve()
        return qp

    qp = solved(0)
    dense.compute_backward(qp, ld[0, 0], *BW)
    for name, v in ref[0][0].items():
        gate(getattr(qp.model.backward_data, name), v, 1e-6, "dense.compute_backward %s" % name)
    qp.solve()
    r = dense.compute_backward_multi(qp, ld[0], *BW)
    assert r["vectors"].shape == (1, n + ne + ni + n) and np.array_equal(r["active"], flags[0])
    for name in ("dL_dg", "dL_db", "dL_du", "dL_dl", "dL_du_box", "dL_dl_box"):
        gate(r[name][0], ref[0][0][name], 1e-6, "dense.compute_backward_multi %s" % name)
    qp.solve()
    J = dense.solution_jacobians(qp, *BW)
    assert J["dx_dl_box"].shape == (n, n) and J["dx_du_box"].shape == (n, n) and J["dx_du"].shape == (n, ni)
    with pytest.raises(ValueError):
        dense.compute_backward(qp, ld[0, 0, :n + ne + ni], *BW)
    # a QP without box: the two new members stay zero
    plain = solved(0, box=False)
    dense.compute_backward(plain, ld[0, 0, :n + ne + ni], *BW)
    assert plain.model.backward_data.dL_dl_box.shape == (n,) and not np.any(plain.model.backward_data.dL_du_box)
    # solve_backward_in_parallel over three box QPs
    qps = [solved(i) for i in range(B)]
    dense.solve_backward_in_parallel(None, qps, [ld[i, 0] for i in range(B)], *BW)
    for i in range(B):
        for name, v in ref[i][0].items():
            gate(getattr(qps[i].model.backward_data, name), v, 1e-6, "solve_backward_in_parallel QP %d %s" % (i, name))


# ---- GPU only: ROCm tensors --------------------------------------------------------------------------------------------------
def case_rocm_tensors(lib, oracle, randqp):
    import torch
    B, n, ne, ni, K = 4, 10, 4, 7, 3
    case = make_case(oracle, randqp, B, n, ne, ni)
    ld = random_rows(B, K, n, ne, case.nc, dual_rows=1)
    b = box_batch(lib, case)
    V, active = b.backward_box(ld, *BW)
    b.solve()
    Vt, at = b.backward_box(torch.from_numpy(ld).to("cuda"), *BW)
    assert Vt.is_cuda and at.is_cuda and at.dtype == torch.int32
    assert np.array_equal(Vt.cpu().numpy(), V) and np.array_equal(at.cpu().numpy(), active)
    b.solve()
    Vh, ah = b.backward_box(torch.from_numpy(ld), *BW)
    assert not Vh.is_cuda and np.array_equal(Vh.numpy(), V) and np.array_equal(ah.numpy(), active)
    b.close()


# ---- GPU only: the torch layer -----------------------------------------------------------------------------------------------
def shared_case(oracle, randqp, B, n, ne, ni, seed):
    """Q, A, b, G, l, u of ONE QP shared by the batch, p per QP; bounds per QP as make_case places them"""
    randqp.set_seed(seed)
    m = randqp.dense_strongly_convex_qp(n, ne, ni, 0.85, 1e-1)
    g = m.g[None] + 0.5 * np.random.default_rng(seed).standard_normal((B, n))
    l_box, u_box = np.zeros((B, n)), np.zeros((B, n))
    for i in range(B):
        q = oracle.QP(n, ne, ni)
        q.settings.eps_abs, q.settings.eps_rel = EPS, 0
        q.init(m.H, g[i], m.A if ne else None, m.b if ne else None, m.C if ni else None, m.l if ni else None,
               m.u if ni else None)
        q.solve()
        x = q.results.x
        kind = np.arange(n) % 4
        u_box[i] = np.where(kind == 0, x - 0.1, x + 1.0)
        l_box[i] = np.where(kind == 1, x + 0.1, x - 1.0)
    t = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
    return Case(H=t(m.H), g=g, A=t(m.A), b=t(m.b), C=t(m.C), l=t(m.l), u=t(m.u), l_box=l_box, u_box=u_box, hessian="dense")


TORCH_SEEDS = {(10, 3, 4): 3, (10, 3, 0): 0}


def _torch_compare(oracle, randqp, n, ne, ni, B=3):
    import torch
    from proxsuite_amd.torch import QPFunction, QPFunctionBox
    case = shared_case(oracle, randqp, B, n, ne, ni, TORCH_SEEDS[(n, ne, ni)])
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    empty = torch.empty(0, dtype=torch.float64, device=dev)
    w = t(np.random.default_rng(1).standard_normal((B, n)))
    kw = dict(eps=EPS, eps_backward=BW[0], rho_backward=BW[1], mu_backward=BW[2])

    def leaves(*arrays):
        return [t(a).requires_grad_(True) for a in arrays]

    # the box layer: p, l_box, u_box per QP; Q, A, b, G, l, u shared by the batch
    Q, p, lb, ub = leaves(case.H[0], case.g, case.l_box, case.u_box)
    A, bb = (t(case.A[0]), t(case.b[0])) if ne else (empty, empty)
    G, l, u = (t(case.C[0]), t(case.l[0]), t(case.u[0])) if ni else (empty, empty, empty)
    x, y, z, zb = QPFunctionBox(**kw)(Q, p, A, bb, G, l, u, lb, ub)
    assert tuple(x.shape) == (B, n) and tuple(y.shape) == (B, ne) and tuple(z.shape) == (B, ni) and tuple(zb.shape) == (B, n)
    xs, zs = x.detach().cpu().numpy(), torch.cat((z, zb), dim=1).detach().cpu().numpy()
    check_solution(case, xs, zs, [SOLVED] * B)  # (complementarity and the active pattern; the status shows in the residuals below)
    for i in range(B):
        pri, dua = oracle.kkt_residuals(case.H[i], case.g[i], case.A[i], case.b[i], case.C[i], case.l[i], case.u[i], xs[i],
                                        y[i].detach().cpu().numpy(), zs[i], case.l_box[i], case.u_box[i])
        assert pri <= 1e-8 and dua <= 1e-8, (i, pri, dua)
    got = torch.autograd.grad((w * x).sum(), (Q, p, lb, ub))
    # the existing layer on the row-stated QP: G' = [G; I] shared, l' = [l; l_box], u' = [u; u_box] per QP
    rows = case.rows_model()
    Qr, pr, lr, ur = leaves(case.H[0], case.g, rows["l"], rows["u"])
    xr, _, _ = QPFunction(**kw)(Qr, pr, A, bb, t(rows["C"][0]), lr, ur)
    ref = torch.autograd.grad((w * xr).sum(), (Qr, pr, lr, ur))
    gate(xs, xr.detach().cpu().numpy(), 1e-7, "x of the two statements")
    ref = (ref[0], ref[1], ref[2][:, ni:], ref[3][:, ni:])
    # the truth of rule 2 (case_ruiz), for the quantities whose two statements differ by more than the gate under Ruiz
    wn = w.cpu().numpy()
    truth_v = np.stack([kkt_truth(case, i, xs[i], zs[i], wn[i]) for i in range(B)])
    vx = truth_v[:, :n]
    truth = (sum(0.5 * (np.outer(vx[i], xs[i]) + np.outer(xs[i], vx[i])) for i in range(B)), vx,
             truth_v[:, n + ne + case.nc + ni:], truth_v[:, n + ne + ni:n + ne + case.nc])
    for name, g_, r_, t_ in zip(("dL/dQ (shared: the sum)", "dL/dp", "dL/dl_box", "dL/du_box"), got, ref, truth):
        g_, r_ = g_.cpu().numpy(), r_.cpu().numpy()
        assert g_.shape == r_.shape == t_.shape, (name, g_.shape, r_.shape, t_.shape)
        diff, bound = float(np.max(np.abs(g_ - r_))), 1e-6 * (1 + float(np.max(np.abs(r_))))
        scale = 1 + float(np.max(np.abs(t_)))
        e_box, e_rows = float(np.max(np.abs(g_ - t_))), float(np.max(np.abs(r_ - t_)))
        print("%s: |box - rows| %.3e (gate %.3e)  e_box %.3e  e_rows %.3e" % (name, diff, bound, e_box, e_rows))
        if diff > bound:  # Ruiz makes the two statements differ: rule 2
            assert e_rows <= 1e-4 * scale, (name, e_rows)
            assert e_box <= 3 * e_rows + 1e-12 * scale, (name, e_box, e_rows)
    assert np.any(got[2].cpu().numpy() != 0) and np.any(got[3].cpu().numpy() != 0)


def case_torch_layer(oracle, randqp):
    _torch_compare(oracle, randqp, 10, 3, 4)


def case_torch_no_G(oracle, randqp):
    _torch_compare(oracle, randqp, 10, 3, 0)

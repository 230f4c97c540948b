"""TEST INFRASTRUCTURE ONLY.  The backward pass of the closest-feasible QPLayer (QPFunction(structural_feasibility=False),
pqp_batch_backward_closest_feasible, csrc/pqp_infeas.hpp): the cases shared by the emulator tests
(tests/test_emu_infeas_backward.py) and the GPU tests (tests/test_gpu_infeas_backward.py).

The yardstick is `restated_backward`: a numpy restatement, per QP, of the reference's Python
(bindings/python/proxsuite/torch/qplayer.py:403-610) whose linear system is solved by the CPU oracle as the QP the
reference hands to ProxQP -- with three corrections the chain rule and finite differences decide (case_yardstick_fd):
dG = dG1[ns:] - dG1[:ns] instead of the +G half alone, the SUM over the batch for shared parameters instead of the mean,
fp64 throughout.  To keep a comparison about the backward alone it takes x, y, z, se and the P1 / P2 flags from the
device's forward: active constraints sit at s ~ 0, where P2 = (s <= 0) is decided at the rounding level on either side.
`check_flags` keeps that from hiding an error."""
import numpy as np

from proxsuite_amd._ctypes_defs import HessianType, InitialGuess

SHAPES = [(10, 3, 6), (8, 0, 5)]
WIDE_SHAPE = (48, 12, 32)  # inner QP 284 x 200: wider than one 256-thread row pass, more than one row tile per block
EPS_FORWARD = 1e-9
RHO_FORWARD = 5.0e-5
# Outer iterations of the device forwards.  An infeasible QP never meets eps: its closest-feasible iterate stalls near 1e-8
# of its limit after ~20 outer iterations (oracle, every shape and seed used here: |x_50 - x_1000| <= 2e-8) and the
# layer's default of 1000 only repeats them -- minutes on the emulator.  The comparisons below take the forward as the
# device left it, so they do not depend on how far it went.
MAX_ITER_FORWARD = 50


def make_qp(n, ne, ns, seed, infeasible=False):
    """strongly convex, double-sided; `infeasible`: one empty box"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    H = M @ M.T / n + 0.1 * np.eye(n)
    g = rng.standard_normal(n)
    A = rng.standard_normal((ne, n))
    C = rng.standard_normal((ns, n))
    x0 = rng.standard_normal(n)
    b = A @ x0
    l = C @ x0 - rng.uniform(0.0, 1.0, ns)
    u = C @ x0 + rng.uniform(0.0, 1.0, ns)
    if infeasible:
        l[1] = u[1] + 0.7
    return dict(H=H, g=g, A=A, b=b, C=C, l=l, u=u)


def make_batch(shape, B):
    """seeds 0 .. B-1, the second half of them infeasible"""
    return [make_qp(*shape, seed=s, infeasible=(s >= (B + 1) // 2)) for s in range(B)]


def single_sided(qp):
    return np.concatenate((-qp["C"], qp["C"])), np.concatenate((-qp["l"], qp["u"]))


def dims(n, ne, ni):
    """(n_row, n_col) of the linear system of a single-sided QP with ni rows"""
    return n + 2 * ni + 2 * ne, 2 * n + 2 * ni + ne + (n if ne else 0)


def numpy_flags(G1, h, x, z):
    """(flags, the quantity that decides P1, the quantity that decides P2)"""
    s = G1 @ x - h
    q1 = np.minimum(s, 0.0) + z
    return (q1 >= 0.0).astype(np.int32) | ((s <= 0.0).astype(np.int32) << 1), q1, s


def check_flags(flags, G1, h, x, z, n, ne):
    own, q1, s = numpy_flags(G1, h, x, z)
    far1, far2 = np.abs(q1) > 1e-6, np.abs(s) > 1e-6
    assert np.array_equal((flags & 1)[far1], (own & 1)[far1]), (flags, own, q1)
    assert np.array_equal((flags & 2)[far2], (own & 2)[far2]), (flags, own, s)
    assert np.count_nonzero(~far1 | ~far2) <= n + ne, (q1, s)


def assemble(H, A, G1, flags):
    """K of qplayer.py:435-471 from the P1 / P2 flags"""
    n, ne, ni = H.shape[0], A.shape[0], G1.shape[0]
    n_row, n_col = dims(n, ne, ni)
    P1, P2 = (flags & 1) != 0, (flags & 2) != 0
    K = np.zeros((n_row, n_col))
    K[:n, :n] = H
    if ne:
        K[:n, n:n + ne] = A.T
        K[n:n + ne, :n] = A
        K[n + ne + ni:n + 2 * ne + ni, n:n + ne] = -np.eye(ne)
        K[n + ne + ni:n + 2 * ne + ni, n + ne + 2 * ni:2 * n + ne + 2 * ni] = A
    K[:n, n + ne:n + ne + ni] = G1.T
    K[n + ne:n + ne + ni, :n] = G1
    K[n + 2 * ne + ni:, n + ne:n + ne + ni] = -np.eye(ni)
    K[n + ne:n + ne + ni, n + ne + ni:n + ne + 2 * ni] = np.diag((~P1).astype(float))
    K[n + 2 * ne + ni:, n + ne + ni:n + ne + 2 * ni] = -np.diag((P1 & P2).astype(float))
    K[n + 2 * ne + ni:, n + ne + 2 * ni + (n if ne else 0):] = (~P2).astype(float)[:, None] * G1
    return K


def reference_rhs(n, ne, ns, z, dl_dx, dl_dlam, dl_dnu, dl_dse, dl_dsi):
    """the right-hand side of qplayer.py:473-503 from the derivatives of the layer's five (double-sided) outputs"""
    ni = 2 * ns
    rhs = np.zeros(n + 2 * ni + 2 * ne)
    rhs[:n] = -dl_dx
    rhs[n:n + ne] = -dl_dlam
    active = -z[:ns] + z[ns:] >= 0
    for at, v in ((n + ne, dl_dnu), (n + 2 * ne + ni, dl_dsi)):
        rhs[at:at + ns][~active] = v[~active]
        rhs[at + ns:at + ni][active] = -v[active]
    rhs[n + ne + ni:n + 2 * ne + ni] = -dl_dse
    return rhs


def restated_backward(O, H, A, G1, h, x, y, z, se, rhs, flags=None, eps=1e-9, rho=1e-3, max_iter=10):
    """the solution w of K w = rhs as the reference computes it (qplayer.py:505-537: a QP with zero Hessian, K as
    equality constraints, no inequalities) and the seven jacobians of the SINGLE-SIDED QP (qplayer.py:568-598)"""
    n, ne, ni = H.shape[0], A.shape[0], G1.shape[0]
    if flags is None:
        flags = numpy_flags(G1, h, x, z)[0]
    K = assemble(H, A, G1, flags)
    n_row, n_col = K.shape
    qp = O.QP(n_col, n_row, 0, hessian_type=HessianType.Zero)
    qp.settings.primal_infeasibility_solving = 1
    qp.settings.eps_abs = eps
    qp.settings.max_iter = max_iter
    qp.settings.default_rho = rho
    qp.settings.refactor_rho_threshold = rho
    qp.init(A=K, b=rhs)
    qp.solve()
    w = np.array(qp.results.x)
    dx, dlam, dnu = w[:n], w[n:n + ne], w[n + ne:n + ne + ni]
    b5 = w[n + ne + 2 * ni:2 * n + ne + 2 * ni] if ne else np.zeros(n)
    b6 = w[n + ne + 2 * ni + (n if ne else 0):]
    p2c = np.maximum(G1 @ x - h, 0.0)
    return dict(solution=w, dL_dH=0.5 * (np.outer(dx, x) + np.outer(x, dx)), dL_dg=dx.copy(),
                dL_dA=np.outer(dlam, x) + np.outer(y, dx) + np.outer(se, b5), dL_db=-dlam,
                dL_dC=np.outer(dnu, x) + np.outer(z, dx) + np.outer(p2c, b6), dL_du=-dnu, dL_dl=np.zeros(ni))


JACOBIANS = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_du", "dL_dl")


def fold(r, ns):
    """the gradients of the double-sided parameters (Q, p, A, b, G, l, u) from the single-sided jacobians"""
    return (r["dL_dH"], r["dL_dg"], r["dL_dA"], r["dL_db"], r["dL_dC"][ns:] - r["dL_dC"][:ns], -r["dL_du"][:ns],
            r["dL_du"][ns:])


def close(got, want, what=""):
    """the gate of api_cases.case_backward_api, relative to the array's largest entry (on infeasible QPs the multipliers
    of violated rows reach 1e7 and above)"""
    want = np.asarray(want)
    err = float(np.max(np.abs(np.asarray(got) - want), initial=0.0))
    gate = 1e-6 * (1.0 + float(np.max(np.abs(want), initial=0.0)))
    print("%-28s err %.3e gate %.3e" % (what, err, gate))
    assert err <= gate, (what, err, gate)


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI level: a handle set up and solved as the layer's forward does it


def solved_handle(N, qps, lib=None):
    n, ne, ns = qps[0]["H"].shape[0], qps[0]["A"].shape[0], qps[0]["C"].shape[0]
    B = len(qps)
    batch = N.Batch(B, n, ne, 2 * ns, lib=lib)
    batch.set_all_settings(primal_infeasibility_solving=1, max_iter=MAX_ITER_FORWARD, max_iter_in=100, default_rho=RHO_FORWARD,
                           refactor_rho_threshold=RHO_FORWARD, eps_abs=EPS_FORWARD,
                           initial_guess=int(InitialGuess.EQUALITY_CONSTRAINED_INITIAL_GUESS))
    G1 = np.stack([single_sided(q)[0] for q in qps])
    h = np.stack([single_sided(q)[1] for q in qps])
    st = lambda k: np.stack([q[k] for q in qps])
    batch.init(-1, st("H"), st("g"), st("A") if ne else None, st("b") if ne else None, G1, np.full_like(h, -1.0e20), h,
               rho=RHO_FORWARD)
    batch.solve()
    return batch, G1, h


def random_rows(B, n, ne, ni, seed=7):
    return np.random.default_rng(seed).standard_normal((B, n + 2 * ne + 2 * ni))


def _ld_on(device, ld):
    if device is None:
        return ld
    import torch
    return torch.as_tensor(ld, device=device)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def case_capi(N, O, shape, B=4, device=None, eps=1e-9):
    """solution rows, flags and the seven arrays of the single-sided QP against the restatement"""
    qps = make_batch(shape, B)
    n, ne, ns = shape
    batch, G1, h = solved_handle(N, qps)
    ld = random_rows(B, n, ne, 2 * ns)
    sol, flags = batch.backward_closest_feasible(_ld_on(device, ld), eps)
    sol, flags = _host(sol), _host(flags)
    x, y, z, se, _, info = batch.results()
    got = batch.backward_results(-1)
    for i, q in enumerate(qps):
        check_flags(flags[i], G1[i], h[i], x[i], z[i], n, ne)
        ref = restated_backward(O, q["H"], q["A"], G1[i], h[i], x[i], y[i], z[i], se[i], -ld[i], flags[i], eps)
        close(sol[i], ref["solution"], "qp %d solution" % i)
        for k in JACOBIANS:
            close(got[k][i], ref[k], "qp %d %s" % (i, k))
    batch.close()


def case_capi_errors(N, shape=(10, 3, 6)):
    import pytest
    n, ne, ns = shape
    qps = make_batch(shape, 2)
    batch, G1, h = solved_handle(N, qps)
    ld = random_rows(2, n, ne, 2 * ns)
    # count == 0: nothing is touched (not even the arrays of get_backward, which do not exist yet)
    sol, flags = batch.backward_closest_feasible(ld[:0], 1e-9, first=1, count=0)
    assert sol.shape == (0, dims(n, ne, 2 * ns)[1]) and flags.shape == (0, 2 * ns)
    with pytest.raises(ValueError):
        batch.backward_results(-1)
    with pytest.raises(ValueError):  # a bad range
        batch.backward_closest_feasible(ld, 1e-9, first=1, count=2)
    # a finite lower bound on one QP: PQP_ERR_INVALID_ARGUMENT, nothing is solved
    l = np.full_like(h, -1.0e20)
    l[1, 3] = h[1, 3] - 50.0
    batch.update(-1, l=l)
    batch.solve()
    with pytest.raises(ValueError, match="single-sided"):
        batch.backward_closest_feasible(ld, 1e-9)
    assert not np.any(batch.backward_results(-1)["dL_dg"])
    batch.close()
    boxed = N.Batch(1, n, ne, 2 * ns, box_constraints=True)
    with pytest.raises(N.NativeError, match="-4"):  # PQP_ERR_UNSUPPORTED
        boxed.backward_closest_feasible(ld[:1], 1e-9)
    boxed.close()


def case_passes(N, shape=(10, 3, 6), device=None, B=5):
    """B = 5 in passes of 2 (three passes), in one pass of 5 and with the pass size left to the library: the same bits"""
    qps = make_batch(shape, B)
    n, ne, ns = shape
    batch, _, _ = solved_handle(N, qps)
    ld = _ld_on(device, random_rows(B, n, ne, 2 * ns))
    runs = []
    for per_pass in (2, 5, 0):
        sol, flags = batch.backward_closest_feasible(ld, 1e-9, qps_per_pass=per_pass)
        runs.append((_host(sol).copy(), _host(flags).copy(), batch.backward_results(-1)))
    assert np.any(runs[0][0]) and np.any(runs[0][2]["dL_dC"])
    for sol, flags, arrays in runs[1:]:
        assert np.array_equal(sol, runs[0][0]) and np.array_equal(flags, runs[0][1])
        for k in JACOBIANS:
            assert np.array_equal(arrays[k], runs[0][2][k]), k
    batch.close()


def case_range(N, shape=(10, 3, 6), device=None):
    """first = 1, count = 2 of B = 4: the arrays of slots 0 and 3 stay as they were, 1 and 2 are those of a full call"""
    B = 4
    qps = make_batch(shape, B)
    n, ne, ns = shape
    batch, _, _ = solved_handle(N, qps)
    ld_a, ld_b = random_rows(B, n, ne, 2 * ns, 7), random_rows(B, n, ne, 2 * ns, 8)
    batch.backward_closest_feasible(_ld_on(device, ld_b), 1e-9)
    full_b = batch.backward_results(-1)
    batch.backward_closest_feasible(_ld_on(device, ld_a), 1e-9)
    full_a = batch.backward_results(-1)
    sol, flags = batch.backward_closest_feasible(_ld_on(device, ld_b[1:3]), 1e-9, first=1, count=2)
    assert tuple(sol.shape) == (2, dims(n, ne, 2 * ns)[1]) and tuple(flags.shape) == (2, 2 * ns)
    got = batch.backward_results(-1)
    for k in JACOBIANS:
        assert np.array_equal(got[k][[0, 3]], full_a[k][[0, 3]]), k
        assert np.array_equal(got[k][1:3], full_b[k][1:3]), k
    assert not np.array_equal(full_a["dL_dg"], full_b["dL_dg"])
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# the layer


def _layer_run(QPFunction, qps, device, shared=(), eps_backward=1e-9, seed=11):
    """loss = sum of fixed random weights times the five outputs; returns (gradients by name, handle, weights)"""
    import torch
    n, ne, ns = qps[0]["H"].shape[0], qps[0]["A"].shape[0], qps[0]["C"].shape[0]
    B = len(qps)
    names = ("H", "g", "A", "b", "C", "l", "u")
    params = {}
    for k in names:
        a = qps[0][k] if k in shared else np.stack([q[k] for q in qps])
        if k in ("A", "b") and ne == 0:
            params[k] = torch.empty(0, dtype=torch.float64, device=device)
        else:
            params[k] = torch.tensor(a, dtype=torch.float64, device=device, requires_grad=True)
    rng = np.random.default_rng(seed)
    w = [rng.standard_normal(s) for s in ((B, n), (B, ne), (B, ns), (B, ne), (B, ns))]
    f = QPFunction(eps=EPS_FORWARD, maxIter=MAX_ITER_FORWARD, eps_backward=eps_backward, structural_feasibility=False)
    outs = f(*[params[k] for k in names])
    loss = sum((torch.tensor(wk, device=device) * o).sum() for wk, o in zip(w, outs) if wk.size)
    loss.backward()
    grads = {k: (None if params[k].grad is None else params[k].grad.detach().cpu().numpy()) for k in names}
    return grads, outs[0].grad_fn.batch, w, outs


def case_layer(QPFunction, O, shape, device="cpu", B=4, eps_backward=1e-9):
    """QPFunction(structural_feasibility=False): loss.backward() returns seven gradients of the right shapes, each equal
    to the restatement (which takes the forward and the flags from the device)"""
    qps = make_batch(shape, B)
    n, ne, ns = shape
    grads, batch, w, outs = _layer_run(QPFunction, qps, device, eps_backward=eps_backward)
    x, y, z, se, _, _ = batch.results()
    want_shapes = dict(H=(B, n, n), g=(B, n), A=(B, ne, n), b=(B, ne), C=(B, ns, n), l=(B, ns), u=(B, ns))
    for k, s in want_shapes.items():
        if k in ("A", "b") and ne == 0:
            assert grads[k] is None
        else:
            assert grads[k] is not None and grads[k].shape == s and np.all(np.isfinite(grads[k])), k
    # the flags of the same handle, by a call of the C-ABI of its own (the rows do not matter for them)
    _, flags = batch.backward_closest_feasible(np.zeros((B, dims(n, ne, 2 * ns)[0])), eps_backward)
    for i, q in enumerate(qps):
        G1, h = single_sided(q)
        check_flags(flags[i], G1, h, x[i], z[i], n, ne)
        rhs = reference_rhs(n, ne, ns, z[i], w[0][i], w[1][i], w[2][i], w[3][i], w[4][i])
        ref = fold(restated_backward(O, q["H"], q["A"], G1, h, x[i], y[i], z[i], se[i], rhs, flags[i], eps_backward), ns)
        for k, v in zip(("H", "g", "A", "b", "C", "l", "u"), ref):
            if grads[k] is not None:
                close(grads[k][i], v, "qp %d d%s" % (i, k))
    del outs


def case_shared(QPFunction, shape=(10, 3, 6), device="cpu", B=4):
    """Q, A, G shared by the batch, p, b, l, u batched: the shared gradients are the batch SUM of the fully batched run"""
    qps = make_batch(shape, B)
    for q in qps[1:]:  # the same matrices in every QP; b, l, u stay those of the QP's own point
        for k in ("H", "A", "C"):
            q[k] = qps[0][k]
    full = _layer_run(QPFunction, qps, device)[0]
    shared = _layer_run(QPFunction, qps, device, shared=("H", "A", "C"))[0]
    for k in ("H", "A", "C"):
        assert shared[k].shape == full[k].shape[1:]
        s = full[k].sum(axis=0)
        assert np.max(np.abs(shared[k] - s)) <= 1e-12 * (1.0 + np.max(np.abs(s))), k
    for k in ("g", "b", "l", "u"):
        assert np.array_equal(shared[k], full[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick itself against finite differences (oracle only)


def oracle_forward(O, qp, eps):
    """the closest-feasible solution of the single-sided restatement, with the layer's settings"""
    n, ne, ns = qp["H"].shape[0], qp["A"].shape[0], qp["C"].shape[0]
    G1, h = single_sided(qp)
    o = O.QP(n, ne, 2 * ns)
    o.settings.primal_infeasibility_solving = 1
    o.settings.max_iter, o.settings.max_iter_in = 1000, 100
    o.settings.default_rho = o.settings.refactor_rho_threshold = RHO_FORWARD
    o.settings.eps_abs = eps
    o.init(qp["H"], qp["g"], qp["A"] if ne else None, qp["b"] if ne else None, G1, np.full(2 * ns, -1.0e20), h,
           rho=RHO_FORWARD)
    o.solve()
    r = o.results
    return np.array(r.x), np.array(r.y), np.array(r.z), np.array(r.se)


def case_yardstick_fd(O, seed, infeasible, shape=(10, 3, 6), step=1e-3):
    """restated_backward (oracle forward, its own flags, eps_backward = 1e-9) against central differences of the
    oracle's closest-feasible x for the loss w^T x: p, b, l, u, every entry of A and C, symmetric perturbations of H.
    Gate 1e-3 (1 + max |fd|); the reference's half-only dG must fail it."""
    n, ne, ns = shape
    qp = make_qp(n, ne, ns, seed, infeasible)
    w = np.random.default_rng(100 + seed).standard_normal(n)
    G1, h = single_sided(qp)
    x, y, z, se = oracle_forward(O, qp, 1e-9)
    zero = np.zeros
    rhs = reference_rhs(n, ne, ns, z, w, zero(ne), zero(ns), zero(ne), zero(ns))
    single = restated_backward(O, qp["H"], qp["A"], G1, h, x, y, z, se, rhs, None, 1e-9)
    ours = dict(zip(("H", "g", "A", "b", "C", "l", "u"), fold(single, ns)))

    def loss(**changed):
        return float(w @ oracle_forward(O, dict(qp, **changed), 1e-11)[0])

    def central(key, idx, symmetric=False):
        vals = []
        for sgn in (1.0, -1.0):
            a = qp[key].copy()
            a[idx] += sgn * step
            if symmetric and idx[0] != idx[1]:
                a[idx[::-1]] += sgn * step
            vals.append(loss(**{key: a}))
        return (vals[0] - vals[1]) / (2.0 * step)

    fd = {}
    for k in ("g", "b", "l", "u", "A", "C"):
        fd[k] = np.array([central(k, idx) for idx in np.ndindex(qp[k].shape)]).reshape(qp[k].shape)
    # H + t (E_ij + E_ji): d loss / dt = dH_ij + dH_ji (the diagonal: E_ii once)
    fdH, ourH = [], []
    for i in range(n):
        for j in range(i, n):
            fdH.append(central("H", (i, j), symmetric=True))
            ourH.append(ours["H"][i, j] + (ours["H"][j, i] if i != j else 0.0))
    fd["H"], ours["H"] = np.array(fdH), np.array(ourH)
    for k, v in fd.items():
        err, gate = np.max(np.abs(ours[k] - v)), 1e-3 * (1.0 + np.max(np.abs(v)))
        print("seed %d infeasible %d d%s: err %.3e gate %.3e (max |fd| %.3e)" % (seed, infeasible, k, err, gate, np.max(np.abs(v))))
        assert err <= gate, (k, err, gate)
    half = single["dL_dC"][ns:]  # what the reference returns for dG (qplayer.py:605)
    assert np.max(np.abs(half - fd["C"])) > 1e-3 * (1.0 + np.max(np.abs(fd["C"])))

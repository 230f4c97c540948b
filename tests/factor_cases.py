"""Direct checks of the factors the linear-algebra engine leaves in HBM (shared by tests/test_emu_factors.py and
tests/test_gpu_factors.py, as parity_cases.py is shared by the parity tests).

A whole solve cannot see a factor that is wrong in its 9th digit: every KKT solve is followed by iterative
refinement on the unfactorised operator, which absorbs the error in an extra step that nothing counts.  Here every
stage of setup_factorization -- the LDL^T of H_s + rho I, the explicit inverse W = L^{-1}, Z = B W^T, the Gram matrix
G = Z D^{-1} Z^T -- and the (edited) inverse factor of the dual Schur block / of P_J are read back
(pqp_batch_get_primal_factor, pqp_batch_get_schur_factor) and judged against THEIR OWN inputs, also read from the
device (pqp_batch_get_scaled), in np.longdouble (64-bit mantissa on x86).

Gates.  u = 2^-53, gamma_k = k u / (1 - k u).  The four componentwise gates are the standard rounding-error bounds
of the operations (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3, 8, 10); they hold for any order
of summation, with or without FMA, so a ratio |residual| / bound above 1 is a defect and not a tolerance to tune:

  ldlt   L diag(dF) L^T - (H_s + rho I)      <= gamma_{n+1} |L| |D| |L^T|  (+ a propagated term, because F does not
                                                store the diagonal blocks of L: see the end of this text)
  winv   WL L - I  and  L WL - I             <= gamma_n M(L)^{-1} |L|,  M(L) = 2I - |L| (covers substitution and
                                                Neumann-product orders alike; vacuous on the 16 x 16 diagonal blocks,
                                                for the same reason: see the end of this text)
  z      Zr - B WL^T                         <= gamma_n |B| |WL^T|
  g      G - Zr diag(1/dF) Zr^T              <= gamma_{n+3} |Zr| |1/dF| |Zr^T|

A correct double-precision kernel sits at 0.01 - 0.12 of these bounds; one that loses three digits fails.
Entries whose bound is zero (the structural zeros) must have a residual of exactly zero: ratios are
|residual| / (bound + tiny).

The dual Schur block S = M_J + G_JJ (condition numbers up to 1e12 at the mu floors) and P_J of the PrimalLDLT engine
have no componentwise bound that textbook float64 meets; their identity W S W^T = D is judged normwise,
max|.| / max(1, max|D|): an unedited factor against 8 x the same metric of a plain float64 factorisation +
substitution inverse of the SAME S computed here, + 64 u; a factor that has taken rank-1 edits against the project's
1e-11, with the ratio to a fresh float64 factorisation recorded.

The forward leg compares G with B (H_s + rho I)^{-1} B^T computed entirely in long double, relative to max|G|; its
size depends on the conditioning, so the same error of a plain float64 chain on the same matrices sets the scale:
device <= 8 x that + 64 u.

Where the device stores something else than the textbook object it is said here:
  * F holds L in the UPPER mirror (F[j][i] = L_ij, i > j) and d_j on the diagonal.  The lower mirror outside the
    16 x 16 diagonal blocks is written by the blocked factorisation only (n > 112); the register-resident one
    (n <= 112) leaves it alone.  Inside diagonal block b both strict triangles hold inv(L_bb) and its transpose, not
    L_bb: L_bb is recovered here as the long-double inverse of that block (exact to 2^-64, 2000 times below u).
    The recovered block is the device's own only up to the error of the stored inverse, |L_bb| gamma_16 M(L_bb)^{-1} |L_bb|
    by the winv bound of one block; that difference dL enters the ldlt identity as dL D L^T + L D dL^T, and exactly
    this term is added to the ldlt bound.  It is not small against the issue's gamma_{n+1} |L| |D| |L^T|: on generator-
    like matrices it is a median 8 x / 2 x / 0.6 x / 0.14 x that bound at n = 16 / 33 / 64 / 128 and up to 230 x / 410 x
    / 80 x / 14 x on single entries -- still ~1e-13 relative, where the mutation that drops one factor of the Neumann
    product measures 1e4 - 1e11 times the widened bound.  (Without it the structural zeros of a sparse H_s inside a diagonal block, which
    the inverse of an inverse fills with 1e-17, would read as infinite ratios.)
  * winv says NOTHING about the diagonal blocks: WL's diagonal blocks are the stored inv(L_bb) bit for bit (asserted)
    and L_bb is the long-double inverse of that same block, so WL L - I vanishes there by construction (winv = 0 for
    every n <= 16).  winv judges the block forward substitution below the diagonal blocks; inv(L_bb) itself -- the
    Neumann product -- is judged through ldlt (a wrong inverse makes the recovered L_bb wrong by far more than the added
    term) and through wkw, which does not go through F at all.
  * wkw: WL (H_s + rho I) WL^T - diag(dF), the pair the solver actually applies, judged normwise like the Schur row
    (8 x the float64 comparator on the same matrix + 64 u).
"""
import numpy as np

from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import DenseBackend, HessianType, InitialGuess

LD = np.longdouble
U = 2.0 ** -53
TINY = float(np.finfo(np.float64).tiny)
EPS = 1e-9
EDITED_TOL = 1e-11  # (tests/parity_cases.py::case_schur_factor_identity)


def gamma(k):
    return k * U / (1.0 - k * U)


def ratio(res, bound):
    """max |res| / (bound + tiny): 0 / 0 -> 0, a non-zero residual on a structural zero -> huge"""
    if res.size == 0:
        return 0.0
    assert np.all(np.isfinite(res)), "non-finite residual"
    return float(np.max(np.abs(res) / (np.asarray(bound, dtype=LD) + LD(TINY))))


# ---- the reference: textbook routines, run in long double (and in float64 for the comparators) --------------------
def ldlt_unblocked(A):
    """right-looking unblocked LDL^T of a symmetric positive definite matrix in the dtype of A"""
    A = A.copy()
    n = A.shape[0]
    L = np.eye(n, dtype=A.dtype)
    d = np.zeros(n, dtype=A.dtype)
    for k in range(n):
        d[k] = A[k, k]
        L[k + 1:, k] = A[k + 1:, k] / d[k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], A[k + 1:, k])
    return L, d


def unit_lower_inverse(L):
    """X with L X = I by forward substitution, row by row, in the dtype of L"""
    n = L.shape[0]
    X = np.eye(n, dtype=L.dtype)
    for i in range(1, n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i])
    return X


def mm(a, b):
    return np.asarray(a, dtype=LD) @ np.asarray(b, dtype=LD)


def L_of_F(F):
    """the unit lower factor out of the device's F buffer (see the module docstring)"""
    n = F.shape[0]
    L = np.triu(F, 1).T.astype(LD) + np.eye(n, dtype=LD)
    for j0 in range(0, n, 16):
        s = slice(j0, min(j0 + 16, n))
        V = np.tril(F[s, s], -1).astype(LD) + np.eye(s.stop - s.start, dtype=LD)
        L[s, s] = unit_lower_inverse(V)
    return L


def constraint_matrix(sc, pf, box):
    rows = [sc["A"], sc["C"]]
    if box:
        rows.append(np.diag(pf["i_scaled"]))
    return np.concatenate(rows, axis=0)


# ---- per-stage checks ---------------------------------------------------------------------------------------------
def check_structure_dense(pf, G, box, n, nb):
    """without tolerance: transposed copies come from the same registers / an LDS transposition"""
    F, WL, WU, Zr, Zc, dF = (pf[k] for k in ("F", "WL", "WU", "Zr", "Zc", "dF"))
    assert np.array_equal(WU, WL.T), "WU != WL^T"
    assert np.array_equal(Zc, Zr.T), "Zc != Zr^T"
    assert np.array_equal(G, G.T), "G != G^T"
    assert np.all(WL[np.triu_indices(n, 1)] == 0.0), "strict upper triangle of WL"
    assert np.all(np.diag(WL) == 1.0), "unit diagonal of WL"
    assert np.all(dF > 0), "dF > 0"
    assert np.array_equal(np.diag(F), dF), "diagonal of F is D"
    # the diagonal blocks carry inv(L_bb) in both triangles; beyond 112 columns the blocked factorisation writes both
    # mirrors of L as well
    for j0 in range(0, n, 16):
        s = slice(j0, min(j0 + 16, n))
        assert np.array_equal(np.tril(F[s, s], -1), np.triu(F[s, s], 1).T), ("diagonal block of F not mirrored", j0)
        assert np.array_equal(np.tril(WL[s, s], -1), np.tril(F[s, s], -1)), ("W_bb is not the block's inverse", j0)
    if n > 112:
        assert np.array_equal(F, F.T), "F not mirrored"


def check_primal_dense(pf, sc, G, box, forward=True):
    """the four componentwise gates + the forward leg of one QP with a dense Hessian; returns {stage: ratio}"""
    n = sc["H"].shape[0]
    rho = pf["rho"]
    Hs = np.triu(sc["H"]) + np.triu(sc["H"], 1).T  # (the factorisation reads the upper triangle)
    K = Hs.astype(LD) + LD(rho) * np.eye(n, dtype=LD)
    L = L_of_F(pf["F"])
    d = pf["dF"].astype(LD)
    WL = pf["WL"]
    B = constraint_matrix(sc, pf, box)
    Zr = pf["Zr"]
    aL = np.abs(L).astype(np.float64)
    out = {}
    # L_bb is the inverse of what the device stores, V_bb = fl(inv(L_bb)) with |V_bb L_bb - I| <= E_b (the winv gate of
    # one block, k = 16): the recovered block differs from the device's own by at most |L_bb| E_b to first order, and
    # that difference dL reaches the identity as dL D L^T + L D dL^T.  Both terms are added to the bound.
    dL = np.zeros((n, n))
    for j0 in range(0, n, 16):
        s = slice(j0, min(j0 + 16, n))
        m = s.stop - s.start
        dL[s, s] = aL[s, s] @ (gamma(m) * np.linalg.solve(2.0 * np.eye(m) - aL[s, s], aL[s, s]))
    prop = (dL * np.abs(pf["dF"])) @ aL.T
    out["ldlt"] = ratio(mm(L * d, L.T) - K, gamma(n + 1) * ((aL * np.abs(pf["dF"])) @ aL.T) + prop + prop.T)
    # the pair the solver applies, (W, D), against the matrix itself: normwise like the Schur row, independent of F
    out["wkw"] = check_inverse_factor(WL, pf["dF"], K, False)[0]
    Minv_L = np.linalg.solve(2.0 * np.eye(n) - aL, aL)
    out["winv_left"] = ratio(mm(WL, L) - np.eye(n, dtype=LD), gamma(n) * Minv_L)
    out["winv_right"] = ratio(mm(L, WL) - np.eye(n, dtype=LD), gamma(n) * Minv_L)
    if B.shape[0]:
        out["z"] = ratio(Zr.astype(LD) - mm(B, WL.T), gamma(n) * (np.abs(B) @ np.abs(WL.T)))
        t = 1.0 / pf["dF"]
        out["g"] = ratio(G.astype(LD) - mm(Zr.astype(LD) * (LD(1) / d), Zr.T),
                         gamma(n + 3) * ((np.abs(Zr) * np.abs(t)) @ np.abs(Zr.T)))
        if forward:
            out["g_forward"] = forward_leg(K, B, G)
    return out


def gram_chain(K, B):
    """B K^{-1} B^T through the textbook chain (LDL^T, substitution inverse, two products) in the dtype of K"""
    L, d = ldlt_unblocked(K)
    W = unit_lower_inverse(L)
    Z = B.astype(K.dtype) @ W.T
    return (Z / d) @ Z.T


def forward_leg(K, B, G):
    """error of the device's G against the long-double chain, over 8 x the error of the float64 chain + 64 u"""
    exact = gram_chain(K, B)
    scale = float(np.max(np.abs(exact)))
    if scale == 0.0:  # (a tiny QP whose sparse constraint rows are all zero)
        return 0.0 if not np.any(G) else np.inf
    e64 = float(np.max(np.abs(gram_chain(K.astype(np.float64), B).astype(LD) - exact))) / scale
    edev = float(np.max(np.abs(G.astype(LD) - exact))) / scale
    return edev / (8.0 * e64 + 64.0 * U)


def check_primal_identity_L(pf, sc, G, box, dm):
    """diagonal / zero Hessian: L = I.  dF, Zr, Zc are copies / one addition (exact); G gets its gate"""
    n = sc["H"].shape[0]
    hess = pf["meta"]["hessian"]
    dref = (np.diag(sc["H"]) if hess == int(HessianType.Diagonal) else np.zeros(n)) + pf["rho"]
    assert np.array_equal(pf["dF"], dref), "dF != diag(H_s) + rho"
    assert np.all(pf["dF"] > 0)
    out = {}
    if dm:
        ni = sc["C"].shape[0]
        zd = np.concatenate([np.diag(sc["C"]) if ni else np.zeros(0), pf["i_scaled"] if box else np.zeros(0)])
        nd = zd.size
        col = np.concatenate([np.arange(ni), np.arange(n) if box else np.zeros(0, int)]).astype(int)
        assert np.array_equal(pf["Zr"].ravel()[:nd], zd), "zd"
        gd = G.ravel()[:nd]
        ref = zd.astype(LD) ** 2 / pf["dF"][col].astype(LD)
        out["g"] = ratio(gd.astype(LD) - ref, gamma(2) * np.abs(ref.astype(np.float64)))
        return out
    B = constraint_matrix(sc, pf, box)
    assert np.array_equal(pf["Zr"], B), "Zr != B"
    assert np.array_equal(pf["Zc"], B.T), "Zc != B^T"
    assert np.array_equal(G, G.T), "G != G^T"
    if B.shape[0]:
        d = pf["dF"].astype(LD)
        out["g"] = ratio(G.astype(LD) - mm(B.astype(LD) / d, B.T), gamma(n + 3) * ((np.abs(B) / pf["dF"]) @ np.abs(B.T)))
    return out


def inverse_factor_metric(W, d, S):
    """max |W S W^T - D| / max(1, max |D|), evaluated in long double"""
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(d)), "non-finite entry in an inverse factor"
    return float(np.max(np.abs(mm(mm(W, S), W.T) - np.diag(d.astype(LD))))) / max(1.0, float(np.max(np.abs(d))))


def float64_factor_metric(S):
    """the same metric for a plain float64 factorisation + substitution inverse of the same matrix"""
    S64 = np.asarray(S, dtype=np.float64)
    L, d = ldlt_unblocked(S64)
    return inverse_factor_metric(unit_lower_inverse(L), d, S)


def check_inverse_factor(W, d, S, edited):
    """gate of the Schur / PrimalLDLT rows; returns (ratio against the gate, metric, metric of the float64 comparator)"""
    met = inverse_factor_metric(W, d, S)
    m64 = float64_factor_metric(S)
    gate = EDITED_TOL if edited else 8.0 * m64 + 64.0 * U
    return met / gate, met, m64


def schur_block(sf, ne):
    """(W, D, S, live) of the dual Schur block as the device keeps it: slot order, holes as identity rows"""
    WS, dS, G, slots, meta, mus = sf
    ns = meta["n_slots"]
    r = ne + ns
    cid = np.concatenate([np.arange(ne), ne + slots[:ns]]).astype(int)
    live = np.concatenate([np.ones(ne, bool), slots[:ns] >= 0])
    cidc = np.where(live, cid, 0)
    S = G[np.ix_(cidc, cidc)].astype(LD) + np.diag(np.concatenate([np.full(ne, mus[0]), np.full(ns, mus[1])]).astype(LD))
    S[~live, :] = 0
    S[:, ~live] = 0
    S[~live, ~live] = 1.0
    Wfull = WS[:r, :r]
    assert np.all(Wfull[np.triu_indices(r, 1)] == 0.0), "strict upper triangle of W_S"
    assert np.all(np.diag(Wfull) == 1.0), "unit diagonal of W_S"
    assert np.all(dS[:r] > 0), "D_S > 0"
    for h in np.nonzero(~live)[0]:
        assert np.all(Wfull[h, :h] == 0.0) and np.all(Wfull[h + 1:, h] == 0.0) and dS[h] == 1.0, ("hole", int(h))
    assert int(live[ne:].sum()) == meta["n_c"]
    return Wfull, dS[:r], S, r


def primal_ldlt_matrix(pf, sc, sf, box):
    """P_J = H_s + rho I + A_s^T A_s / mu_eq + C_J^T C_J / mu_in (box rows: i_k^2 / mu_in on the diagonal), long double"""
    _, _, _, slots, meta, mus = sf
    n, ni = sc["H"].shape[0], sc["C"].shape[0]
    hess = pf["meta"]["hessian"]
    H = sc["H"] if hess == int(HessianType.Dense) else (np.diag(np.diag(sc["H"])) if hess == int(HessianType.Diagonal) else np.zeros((n, n)))
    P = H.astype(LD) + LD(pf["rho"]) * np.eye(n, dtype=LD)
    if sc["A"].shape[0]:
        P += mm(sc["A"].T, sc["A"]) / LD(mus[0])
    act = np.array([c for c in slots[:meta["n_slots"]] if c >= 0], dtype=int)
    gen = act[act < ni]
    if gen.size:
        P += mm(sc["C"][gen].T, sc["C"][gen]) / LD(mus[1])
    for k in act[act >= ni] - ni:
        P[k, k] += LD(pf["i_scaled"][k]) ** 2 / LD(mus[1])
    return P


# ---- drivers ------------------------------------------------------------------------------------------------------
class Worst(dict):
    """worst ratio per stage over the QPs of a case"""

    def take(self, out):
        for k, v in out.items():
            if not v <= self.get(k, 0.0):  # (a NaN stays: max(0.0, nan) would drop it)
                self[k] = v

    def line(self, label):
        return "%-44s " % label + "  ".join("%s=%.3g" % kv for kv in self.items())


def make_models(randqp, B, n, ne, ni, box, hessian, cond, seed0=0):
    """generator QPs; cond=True: strong convexity 1e-6 (used without preconditioner: cond(H_s + rho I) ~ 1e8)"""
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-6 if cond else 1e-2, seed0=seed0)
    H = m.H
    if hessian == int(HessianType.Diagonal):
        H = np.stack([np.diag(np.abs(np.diag(h)) + 1e-2) for h in m.H])
    elif hessian == int(HessianType.Zero):
        H = np.zeros_like(m.H)
    kw = {}
    if box:
        rng = np.random.default_rng(seed0 + 7)
        xs, sh = rng.standard_normal((B, n)), rng.uniform(0.1, 1.0, (B, n))
        kw = dict(l_box=xs - sh, u_box=xs + sh)
    return m, H, kw


def kernel_threads(label):
    """threads per workgroup of a solve kernel, from its label: the one-wavefront kernels run 64, the others say"""
    if label.startswith(("pqp_diag_kernel<", "pqp_dwave_kernel<")):
        return 64
    assert label.startswith(("pqp_solve_kernel<", "pqp_solve_hbm_kernel<")), label
    return int(label.split("<")[1].split(",")[0])


def assert_kernel(b, threads=None, pair=None):
    """what ran, from the launch itself (Batch.last_kernel: the label the launch left on the handle, not a forecast): a
    case must not silently test the other kernel"""
    k = b.last_kernel
    assert k, "no solve has been launched"
    if pair is True:
        assert k.startswith("pqp_dwave_kernel<") and b.last_prologue_ms > 0, ("the one-wavefront pair did not run", k, b.last_prologue_ms)
    elif pair is False:
        assert not k.startswith("pqp_dwave_kernel<") and b.last_prologue_ms == 0, ("the one-wavefront pair ran", k)
    if threads is not None:
        assert kernel_threads(k) == threads, (k, threads)


def solve_batch(lib, randqp, B, n, ne, ni, box=False, hessian=int(HessianType.Dense), cond=False, backend=0,
                max_iter=None, diag_c=False, seed0=0):
    m, H, kw = make_models(randqp, B, n, ne, ni, box, hessian, cond, seed0)
    Cm = m.C
    if diag_c:  # C without off-diagonal entries, n_in == dim: the diagonal-structure signature
        Cm = np.stack([np.diag(np.diag(c) + 1.0) for c in m.C])
    b = N.Batch(B, n, ne, ni, box_constraints=box, hessian_type=hessian, dense_backend=backend, lib=lib)
    st = dict(eps_abs=EPS, eps_rel=0, initial_guess=int(InitialGuess.NO_INITIAL_GUESS))
    if max_iter is not None:
        st["max_iter"] = max_iter
    for i in range(B):
        s = b.settings(i)
        for k, v in st.items():
            setattr(s, k, v)
    b.init(-1, H, m.g, m.A if ne else None, m.b if ne else None, Cm if ni else None, m.l if ni else None,
           m.u if ni else None, compute_preconditioner=not cond, **kw)
    b.solve()
    return b


def take_schur(worst, sf, ne, gate_edited=True):
    """the Schur row on one QP's factor, if it is valid and not empty: unedited against the float64 comparator, edited
    against 1e-11 (`gate_edited=False`: recorded under a name the cases do not assert); returns the block's rows, 0 if
    nothing was checked"""
    meta = sf[4]
    if not meta["ls_valid"] or ne + meta["n_slots"] == 0:
        return 0
    W, d, S, r = schur_block(sf, ne)
    rt = check_inverse_factor(W, d, S, bool(meta["ls_edited"]))[0]
    worst.take({("schur_edited" if gate_edited else "schur_edited_recorded") if meta["ls_edited"] else "schur": rt})
    return r


def case_primal_block(lib, randqp, n, ne, ni, B, box=False, hessian=int(HessianType.Dense), cond=False, diag_c=False,
                      threads=None, pair=None, forward=True, schur=True, need_r_above=None, early_stops=(), label=None,
                      report=None, gate_edited=True):
    """cold solve of B generator QPs, then every stage of every QP whose factor is valid; at least half of the batch
    must have been checked.  With n_in = 0 the Schur block has exactly n_eq rows and is never edited.
    `early_stops`: further solves stopped after so many outer iterations, whose Schur factors are checked as well
    (how a case reaches a block beyond `need_r_above` rows: the active set is largest early in a solve).
    `gate_edited=False`: the metric of an EDITED Schur factor is printed ("schur_edited_recorded", over 1e-11) and not
    asserted -- for the families outside the strongly convex QPs the 1e-11 of case_schur_factor_identity was set for."""
    # (PrimalDualLDLT forced: the automatic choice takes the other engine when n_eq + n_in is large against n; a
    # zero / diagonal Hessian with random constraints need not have a bounded solution: the factors do not care, the
    # solve is cut short)
    b = solve_batch(lib, randqp, B, n, ne, ni, box=box, hessian=hessian, cond=cond, diag_c=diag_c,
                    backend=int(DenseBackend.PrimalDualLDLT), max_iter=None if hessian == int(HessianType.Dense) else 20)
    assert_kernel(b, threads, pair)
    worst, checked, schur_checked, r_max = Worst(), 0, 0, 0
    for q in range(B):
        pf, sc, sf = b.primal_factor(q), b.scaled(q), b.schur_factor(q)
        G, meta = sf[2], sf[4]
        if not pf["meta"]["factor_valid"]:
            continue
        assert pf["meta"]["backend"] == int(DenseBackend.PrimalDualLDLT)
        checked += 1
        dm = bool(pf["meta"]["diag_mode"])
        assert dm == bool(diag_c and hessian != int(HessianType.Dense) and ne == 0 and not (ni and box)), dm
        if hessian == int(HessianType.Dense):
            check_structure_dense(pf, G, box, n, ne + ni)
            worst.take(check_primal_dense(pf, sc, G, box, forward=forward))
        else:
            worst.take(check_primal_identity_L(pf, sc, G, box, dm))
        if schur and not dm:
            r = take_schur(worst, sf, ne, gate_edited)
            if r:
                schur_checked += 1
                r_max = max(r_max, r)
                assert ni > 0 or (r == ne and not meta["ls_edited"])
    # (the primal block does not change from here on: the early stops add Schur factors only)
    for max_iter in early_stops:
        for i in range(B):
            b.settings(i).max_iter = max_iter
        b.solve()
        assert_kernel(b, threads, pair)
        for q in range(B):
            if b.primal_factor(q)["meta"]["factor_valid"]:
                r_max = max(r_max, take_schur(worst, b.schur_factor(q), ne, gate_edited))
    b.close()
    line = worst.line(label or "(%d,%d,%d)%s" % (n, ne, ni, " box" if box else ""))
    print(line)
    if report is not None:
        report.append(line)
    assert 2 * checked >= B, (checked, B)
    if schur and ne > 0 and not diag_c:
        assert 2 * schur_checked >= B, (schur_checked, B)
    if need_r_above is not None:
        assert r_max > need_r_above, (r_max, "no QP ended on a Schur block beyond %d rows" % need_r_above)
    bad = {k: v for k, v in worst.items() if not v <= 1.0 and not k.endswith("_recorded")}
    assert not bad, (bad, line)
    return worst


def case_schur_edited(lib, randqp, n, ne, ni, B, threads=None, pair=None, label=None, report=None):
    """the loop of parity_cases.case_schur_factor_identity (a converged solve, then solves stopped after 2 .. 6 outer
    iterations, which catch the factor in the middle of its life) with the identity evaluated in long double and the
    float64 comparator beside it; enough QPs must have ended on an edited factor"""
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)
    b = N.Batch(B, n, ne, ni, lib=lib)
    b.init(-1, m.H, m.g, m.A, m.b, m.C, m.l, m.u)
    worst, edited, checked, over64 = Worst(), 0, 0, 0.0
    for max_iter in (10000, 2, 3, 4, 5, 6):
        for i in range(B):
            s = b.settings(i)
            s.eps_abs, s.eps_rel, s.initial_guess, s.max_iter = EPS, 0, int(InitialGuess.NO_INITIAL_GUESS), max_iter
        b.solve()
        assert_kernel(b, threads, pair)
        for q in range(B):
            sf = b.schur_factor(q)
            meta = sf[4]
            if not meta["ls_valid"]:
                continue
            W, d, S, r = schur_block(sf, ne)
            rt, met, m64 = check_inverse_factor(W, d, S, bool(meta["ls_edited"]))
            worst.take({"schur_edited" if meta["ls_edited"] else "schur": rt})
            if meta["ls_edited"]:
                over64 = max(over64, met / max(m64, U))
            edited += int(meta["ls_edited"])
            checked += 1
    b.close()
    line = worst.line(label or "(%d,%d,%d) edited" % (n, ne, ni)) + "  edited/float64=%.3g  (%d edited of %d)" % (over64, edited, checked)
    print(line)
    if report is not None:
        report.append(line)
    assert 2 * edited >= B, (edited, "too few QPs ended on an edited factor for this check to mean anything")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (bad, line)
    return worst


def case_kernel_agreement(lib, randqp, monkeypatch, n, ne, ni, B):
    """PQP_DENSE_KERNEL=wave (prologue kernel + one-wavefront kernel) and =workgroup both run Solver::prologue /
    factor_primal_block on 256 threads: the same QPs must leave the same bits in F, dF, WL, Zr, G"""
    snaps = []
    for kernel in ("wave", "workgroup"):
        monkeypatch.setenv("PQP_DENSE_KERNEL", kernel)
        b = solve_batch(lib, randqp, B, n, ne, ni)
        assert_kernel(b, pair=(kernel == "wave"))
        snap = []
        for q in range(B):
            pf = b.primal_factor(q)
            snap.append((pf["meta"]["factor_valid"], pf["rho"], pf["F"], pf["dF"], pf["WL"], pf["Zr"], b.schur_factor(q)[2]))
        snaps.append(snap)
        b.close()
    compared = 0
    for q, (a, c) in enumerate(zip(*snaps)):
        if not (a[0] and c[0]):
            continue
        assert a[1] == c[1], ("rho_fact differs", q, a[1], c[1])
        compared += 1
        for name, u, v in zip(("F", "dF", "WL", "Zr", "G"), a[2:], c[2:]):
            assert np.array_equal(u, v), (name, q, float(np.max(np.abs(u - v))))
    assert 2 * compared >= B, compared


def primal_ldlt_models(randqp, dim, B, seed0=1):
    """the models of parity_cases.case_primal_ldlt: n_eq = n_in = 2 dim, box around a known feasible point"""
    ne = ni = 2 * dim
    H, g = np.zeros((B, dim, dim)), np.zeros((B, dim))
    A, bb = np.zeros((B, ne, dim)), np.zeros((B, ne))
    Cm, l, u = np.zeros((B, ni, dim)), np.zeros((B, ni)), np.zeros((B, ni))
    lb, ub = np.zeros((B, dim)), np.zeros((B, dim))
    for s in range(B):
        randqp.set_seed(seed0 + s)
        m = randqp.dense_strongly_convex_qp(dim, ne, ni, 0.75, 1e-2)
        x_sol = np.array([randqp.normal_rand() for _ in range(dim)])
        delta = np.array([randqp.uniform_rand() for _ in range(ni)])
        shift = np.array([randqp.uniform_rand() for _ in range(dim)])
        H[s], g[s], A[s], Cm[s], l[s] = m.H, m.g, m.A, m.C, m.l
        u[s] = m.C @ x_sol + delta
        bb[s] = m.A @ x_sol
        ub[s], lb[s] = x_sol + shift, x_sol - shift
    return H, g, A, bb, Cm, l, u, lb, ub


def case_primal_ldlt_factor(lib, randqp, dim, B, shape=None, need_edited=False, threads=None, label=None, report=None):
    """DenseBackend::PrimalLDLT: (W, D) of P_J after a cold solve and after solves stopped early, so that factors
    edited by rank-1 updates (pm_rank1) are seen.  `shape` = None: the models of case_primal_ldlt (n_eq = n_in =
    2 dim, box) -- their inequalities sit strictly inside at every stop, so the factor that is left has no active row
    and no edit; shape = (n_eq, n_in, box): the engine forced on generator QPs of that shape, whose active sets
    move, so that edited factors ARE left behind (need_edited)."""
    box = True
    if shape is None:
        ne = ni = 2 * dim
        mats = primal_ldlt_models(randqp, dim, B)
    else:
        ne, ni, box = shape
        m, H, kw = make_models(randqp, B, dim, ne, ni, box, int(HessianType.Dense), False)
        mats = (H, m.g, m.A if ne else None, m.b if ne else None, m.C, m.l, m.u, kw.get("l_box"), kw.get("u_box"))
    b = N.Batch(B, dim, ne, ni, box_constraints=box, dense_backend=int(DenseBackend.PrimalLDLT), lib=lib)
    assert b.dense_backend == int(DenseBackend.PrimalLDLT)
    b.init(-1, *mats)
    worst, edited, checked, over64 = Worst(), 0, 0, 0.0
    per_round = []
    for max_iter in (10000, 2, 3, 4, 5, 6):
        for i in range(B):
            s = b.settings(i)
            s.eps_abs, s.eps_rel, s.initial_guess, s.max_iter = EPS, 0, int(InitialGuess.NO_INITIAL_GUESS), max_iter
        b.solve()
        assert_kernel(b, threads, pair=False)
        n_round = 0
        for q in range(B):
            pf, sc, sf = b.primal_factor(q), b.scaled(q), b.schur_factor(q)
            meta = sf[4]
            assert pf["meta"]["backend"] == int(DenseBackend.PrimalLDLT)
            if not meta["ls_valid"]:
                continue
            W = np.tril(pf["WL"], -1) + np.eye(dim)
            assert np.all(np.diag(pf["WL"]) == 1.0) and np.all(pf["dF"] > 0)
            P = primal_ldlt_matrix(pf, sc, sf, box)
            rt, met, m64 = check_inverse_factor(W, pf["dF"], P, bool(meta["ls_edited"]))
            worst.take({"pldlt_edited" if meta["ls_edited"] else "pldlt": rt})
            if meta["ls_edited"]:
                over64 = max(over64, met / max(m64, U))
            edited += int(meta["ls_edited"])
            checked += 1
            n_round += 1
        per_round.append(n_round)
    b.close()
    line = worst.line(label or "PrimalLDLT dim %d" % dim) + "  edited/float64=%.3g  (%d edited of %d)" % (over64, edited, checked)
    print(line)
    if report is not None:
        report.append(line)
    assert 2 * checked >= B * len(per_round), (per_round, B)
    if need_edited:
        assert edited > 0, "no QP ended on an edited factor of P_J"
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (bad, line)
    return worst

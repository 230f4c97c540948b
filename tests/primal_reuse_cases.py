"""Reuse of the primal block (F, dF, WL, WU, Zr, Zc, G) across solves of an unchanged model -- State::primal_valid --
shared by tests/test_emu_primal_reuse.py and tests/test_gpu_primal_reuse.py, as factor_cases.py is shared by the factor
tests.

The comparator is a TWIN batch: built the same way, given the same commands, but every one of its launches runs under
PQP_PRIMAL_REUSE=0, where a solve factorises exactly as it did before the flag existed.  (Never a freshly initialised
batch: Ruiz on new vectors gives another scaling.)  After every step the two must agree bit for bit in x, y, z, se, si,
every Info field, the seven arrays of the primal block, rho_fact and the Schur factor.

Whether the factorisation ran is read from the instrumented build's cyc_factor_h (the emulator library and
libproxqp_hip_stats.so compile the counters in): 0 where the block is reused, > 0 where it is rebuilt.

A stale factor does not show in results -- refinement on the unfactorised operator absorbs it as extra steps -- so
wherever the block has to be rebuilt it is judged directly against the NEW scaled model with the gates of
factor_cases.py (ratios <= 1), besides the bit-equality with the twin."""
from dataclasses import dataclass, field, replace

import numpy as np

import factor_cases as fc
from proxsuite_amd import _native as N
from proxsuite_amd._ctypes_defs import DenseBackend, HessianType, InitialGuess

DENSE, DIAG = int(HessianType.Dense), int(HessianType.Diagonal)
NO_GUESS = int(InitialGuess.NO_INITIAL_GUESS)
ALL_GUESSES = [int(g) for g in (InitialGuess.NO_INITIAL_GUESS, InitialGuess.EQUALITY_CONSTRAINED_INITIAL_GUESS,
                                InitialGuess.WARM_START_WITH_PREVIOUS_RESULT, InitialGuess.WARM_START,
                                InitialGuess.COLD_START_WITH_PREVIOUS_RESULT)]
CYC_FACTOR_H = N.STAT_NAMES.index("cyc_factor_h")


@dataclass
class Family:
    """one kernel family at the smallest shape it runs at: what to set, what must have run"""
    n: int
    ne: int
    ni: int
    B: int
    env: dict = field(default_factory=dict)
    threads: int = None
    pair: bool = False
    hessian: int = DENSE
    box: bool = False
    backend: int = int(DenseBackend.PrimalDualLDLT)


FAMILIES = {
    "pair": Family(20, 10, 20, 64, env={"PQP_DENSE_KERNEL": "wave"}, pair=True),
    "workgroup": Family(20, 10, 20, 8, env={"PQP_DENSE_KERNEL": "workgroup"}, threads=256),
    "pair_n17": Family(17, 4, 8, 64, env={"PQP_DENSE_KERNEL": "wave"}, pair=True),
    "workgroup_n17": Family(17, 4, 8, 8, env={"PQP_DENSE_KERNEL": "workgroup"}, threads=256),
    "workgroup_box": Family(20, 5, 10, 8, env={"PQP_DENSE_KERNEL": "workgroup"}, threads=256, box=True),
    "threads512": Family(300, 40, 120, 2, threads=512),
    "threads1024": Family(512, 200, 400, 2, threads=1024),
    "hbm_vectors": Family(30, 7, 9, 2, env={"PQP_FORCE_HBM_VECTORS": "1"}, threads=1024),
    "identity_L": Family(40, 10, 30, 4, env={"PQP_DIAG_KERNEL": "workgroup"}, threads=256, hessian=DIAG),
}


def family(name, B=None):
    """`B`: another batch size (the emulator runs the one-wavefront pair, forced by PQP_DENSE_KERNEL=wave, on a handful
    of QPs; on the device the pair gets the 64 QPs from which its dispatch takes it)"""
    f = FAMILIES[name]
    return f if B is None else replace(f, B=B)


class Twins:
    """the batch under test (`a`, launches under PQP_PRIMAL_REUSE=1) and its twin (`t`, under =0)"""

    def __init__(self, lib, randqp, monkeypatch, fam, guess=NO_GUESS, seed0=0):
        self.fam, self.mp = fam, monkeypatch
        for k, v in fam.env.items():
            monkeypatch.setenv(k, v)
        self.m, self.H, self.kw = fc.make_models(randqp, fam.B, fam.n, fam.ne, fam.ni, fam.box, fam.hessian, False, seed0)
        self.a, self.t = self._make(lib, guess), self._make(lib, guess)

    def _make(self, lib, guess):
        f, m = self.fam, self.m
        b = N.Batch(f.B, f.n, f.ne, f.ni, box_constraints=f.box, hessian_type=f.hessian, dense_backend=f.backend, lib=lib)
        st = dict(eps_abs=fc.EPS, eps_rel=0, initial_guess=guess)
        if f.hessian != DENSE:  # (random constraints on a merely convex objective: the factors do not care, the solve is cut short)
            st["max_iter"] = 20
        b.set_all_settings(**st)
        b.init(-1, self.H, m.g, m.A if f.ne else None, m.b if f.ne else None, m.C if f.ni else None,
               m.l if f.ni else None, m.u if f.ni else None, **self.kw)
        return b

    def both(self, fn):
        """the same command on both batches"""
        fn(self.a)
        fn(self.t)

    def solve(self, launch=lambda b: b.solve(), kernel=None):
        """one launch each; returns the factorisation cycles per QP of the batch under test and of the twin"""
        if kernel is not None:
            self.mp.setenv("PQP_DENSE_KERNEL", kernel)
        out = []
        for b, reuse in ((self.a, "1"), (self.t, "0")):
            self.mp.setenv("PQP_PRIMAL_REUSE", reuse)
            launch(b)
            out.append(b.stats()[:, CYC_FACTOR_H].copy())
        self.mp.delenv("PQP_PRIMAL_REUSE")
        return out

    def assert_kernel(self, pair=None, threads=None):
        for b in (self.a, self.t):
            fc.assert_kernel(b, self.fam.threads if threads is None and pair is None else threads,
                             self.fam.pair if pair is None else pair)

    def assert_equal(self, what=""):
        a, t = self.a, self.t
        ra, rt = a.results(), t.results()
        for name, u, v in zip(("x", "y", "z", "se", "si"), ra[:5], rt[:5]):
            assert np.array_equal(u, v), (what, name, float(np.max(np.abs(u - v))))
        assert bytes(ra[5]) == bytes(rt[5]), (what, "Info records differ")
        for q in range(self.fam.B):
            pa, pt = a.primal_factor(q), t.primal_factor(q)
            assert pa["meta"] == pt["meta"] and pa["rho"] == pt["rho"], (what, q, pa["meta"], pt["meta"], pa["rho"], pt["rho"])
            for name in ("F", "dF", "WL", "WU", "Zr", "Zc"):
                assert np.array_equal(pa[name], pt[name]), (what, name, q)
            sa, st = a.schur_factor(q), t.schur_factor(q)
            assert sa[4] == st[4] and np.array_equal(sa[5], st[5]), (what, "Schur meta", q, sa[4], st[4])
            assert np.array_equal(sa[3], st[3]), (what, "slots", q)
            if self.fam.backend == int(DenseBackend.PrimalLDLT):
                continue  # (no dual Schur block in that engine: its factor is WL / dF above)
            r = self.fam.ne + sa[4]["n_slots"]  # (rows of the block: what lies beyond them in W_S and D_S is scratch)
            for name, u, v in (("WS", sa[0][:r, :r], st[0][:r, :r]), ("dS", sa[1][:r], st[1][:r]), ("G", sa[2], st[2])):
                assert np.array_equal(u, v), (what, name, q)

    def assert_factors(self, what=""):
        """the block the batch under test holds, against ITS OWN current scaled model (dense Hessian)"""
        f, worst = self.fam, fc.Worst()
        for q in range(f.B):
            pf, sc, G = self.a.primal_factor(q), self.a.scaled(q), self.a.schur_factor(q)[2]
            assert pf["meta"]["factor_valid"] == 1, (what, q)
            fc.check_structure_dense(pf, G, f.box, f.n, f.ne + f.ni)
            worst.take(fc.check_primal_dense(pf, sc, G, f.box))
        print(worst.line(what))
        bad = {k: v for k, v in worst.items() if not v <= 1.0}
        assert not bad, (what, bad)

    def close(self):
        self.a.close()
        self.t.close()


def expect(cyc, reused, what, counters=True):
    """cyc = (batch under test, twin): the twin always factorises; the batch under test exactly where `reused` is False.
    `reused`: one bool, or one per QP"""
    if not counters:
        return
    a, t = cyc
    assert np.all(t > 0), (what, "the twin did not factorise", t)
    r = np.broadcast_to(np.asarray(reused, dtype=bool), a.shape)
    assert np.all(a[r] == 0), (what, "factorised where the block in HBM was valid", a)
    assert np.all(a[~r] > 0), (what, "skipped a factorisation it needed", a)


# ---- 1. re-solve ---------------------------------------------------------------------------------------------------
def case_resolve(lib, randqp, monkeypatch, fam, counters=True, B=None):
    """solve twice with NO_INITIAL_GUESS, and again after cleanup(): only the first solve factorises"""
    tw = Twins(lib, randqp, monkeypatch, family(fam, B))
    expect(tw.solve(), False, "first solve", counters)
    tw.assert_kernel()
    tw.assert_equal("first solve")
    expect(tw.solve(), True, "second solve", counters)
    tw.assert_kernel()
    tw.assert_equal("second solve")
    tw.both(lambda b: b.cleanup())
    expect(tw.solve(), True, "solve after cleanup", counters)
    tw.assert_equal("solve after cleanup")
    if tw.fam.hessian == DENSE:
        tw.assert_factors("%s: the block three solves old" % fam)
    tw.close()


# ---- 2. vector-only update -----------------------------------------------------------------------------------------
def case_vector_update(lib, randqp, monkeypatch, fam, guess, counters=True, B=None):
    """update(g, b, l, u) on fixed H, A, C: the set-up kernel leaves the scaled matrices alone (same bits) and the next
    solve, whatever its initial guess, does not factorise the primal block"""
    f = family(fam, B)
    tw = Twins(lib, randqp, monkeypatch, f, guess=guess)
    expect(tw.solve(), False, "first solve", counters)
    before = [tw.a.scaled(q) for q in range(f.B)]
    rng = np.random.default_rng(5)
    m = tw.m
    g2 = m.g + 0.1 * rng.standard_normal(m.g.shape)
    b2 = m.b + 0.01 * rng.standard_normal(m.b.shape)
    l2, u2 = m.l - 0.05, m.u + 0.05
    x0 = [r.copy() for r in tw.a.results()[:3]]
    tw.both(lambda b: b.update(-1, g=g2, b=b2, l=l2, u=u2))
    if guess == int(InitialGuess.WARM_START):
        tw.both(lambda b: b.warm_start(-1, *x0))
    tw.both(lambda b: b.flush())
    for q in range(f.B):
        after = tw.a.scaled(q)
        for k in ("H", "A", "C", "delta"):
            assert np.array_equal(before[q][k], after[k]), ("scaled %s changed by a vector-only update" % k, q)
        assert before[q]["c"] == after["c"]
        assert not np.array_equal(before[q]["g"], after["g"]), "the update did not reach the scaled vectors"
    cyc = tw.solve()
    if guess == int(InitialGuess.WARM_START_WITH_PREVIOUS_RESULT):
        # (that mode restores the whole factorisation, primal block and Schur factor, on either batch: nothing to elide)
        assert not counters or (np.all(cyc[0] == 0) and np.all(cyc[1] == 0)), cyc
    else:
        expect(cyc, True, "solve after update(g, b, l, u)", counters)
    tw.assert_kernel()
    tw.assert_equal("solve after update(g, b, l, u), initial guess %d" % guess)
    tw.assert_factors("vector update, initial guess %d" % guess)
    tw.close()


# ---- 3. invalidation -----------------------------------------------------------------------------------------------
def _perturbed(tw, rng):
    m, f = tw.m, tw.fam
    E = 0.05 * rng.standard_normal(tw.H.shape)
    H2 = tw.H + E + np.swapaxes(E, 1, 2) + 0.5 * np.eye(f.n)
    A2 = m.A + 0.05 * rng.standard_normal(m.A.shape)
    C2 = m.C + 0.05 * rng.standard_normal(m.C.shape)
    return H2, A2, C2


INVALIDATIONS = ("update_H", "update_A", "update_C", "update_preconditioner", "update_rho", "default_rho", "backward",
                 "second_init")


def case_invalidation(lib, randqp, monkeypatch, fam, how, counters=True, B=None):
    """each of these changes a scaled matrix or rho: the next solve factorises, its factors pass the gates on the new
    model and equal the twin's"""
    f = family(fam, B)
    tw = Twins(lib, randqp, monkeypatch, f)
    expect(tw.solve(), False, "first solve", counters)
    expect(tw.solve(), True, "second solve", counters)
    rng = np.random.default_rng(11)
    H2, A2, C2 = _perturbed(tw, rng)
    m = tw.m
    rho_expected = 1e-6
    if how == "update_H":
        tw.both(lambda b: b.update(-1, H=H2))
    elif how == "update_A":
        tw.both(lambda b: b.update(-1, A=A2))
    elif how == "update_C":
        tw.both(lambda b: b.update(-1, C=C2))
    elif how == "update_preconditioner":
        g2 = m.g * (1.0 + rng.uniform(0.5, 2.0, m.g.shape))
        tw.both(lambda b: b.update(-1, g=g2, update_preconditioner=True))
    elif how == "update_rho":
        rho_expected = 1e-5
        tw.both(lambda b: b.update(-1, rho=1e-5))
    elif how == "default_rho":
        rho_expected = 3e-6
        tw.both(lambda b: b.set_all_settings(default_rho=3e-6))
    elif how == "backward":
        ld = rng.standard_normal((f.B, f.n + f.ne + f.ni))
        tw.both(lambda b: b.backward(ld))
    elif how == "second_init":
        tw.both(lambda b: b.init(-1, H2, m.g, A2, m.b, C2, m.l, m.u))
    else:
        raise ValueError(how)
    expect(tw.solve(), False, "solve after %s" % how, counters)
    tw.assert_kernel()
    tw.assert_equal("solve after %s" % how)
    tw.assert_factors("%s after %s" % (fam, how))
    assert tw.a.primal_factor(0)["rho"] == rho_expected, (tw.a.primal_factor(0)["rho"], rho_expected)
    # and the rebuilt block is reused in turn
    expect(tw.solve(), True, "re-solve after %s" % how, counters)
    tw.assert_equal("re-solve after %s" % how)
    tw.close()


# ---- 4. settings that do not invalidate -----------------------------------------------------------------------------
def case_settings_keep(lib, randqp, monkeypatch, fam, counters=True, B=None):
    tw = Twins(lib, randqp, monkeypatch, family(fam, B))
    expect(tw.solve(), False, "first solve", counters)
    for change in (dict(eps_abs=1e-6), dict(max_iter=3), dict(max_iter=10000, default_mu_eq=1e-2, default_mu_in=1e-2)):
        tw.both(lambda b: b.set_all_settings(**change))
        expect(tw.solve(), True, "solve under %s" % (change,), counters)
        tw.assert_equal("solve under %s" % (change,))
    tw.assert_factors("after changes of eps_abs, max_iter, default_mu_*")
    tw.close()


# ---- 5. hand-over between kernel families ---------------------------------------------------------------------------
def case_hand_over(lib, randqp, monkeypatch, first, counters=True, B=None):
    """the block one kernel family left is taken by the other: first solve by `first`, second by the other one, with
    PQP_DENSE_KERNEL toggled between the launches; the twin's second solve runs the second family with reuse off"""
    second = "workgroup" if first == "wave" else "wave"
    tw = Twins(lib, randqp, monkeypatch, family("pair", B))
    expect(tw.solve(kernel=first), False, "first solve (%s)" % first, counters)
    tw.assert_kernel(pair=(first == "wave"))
    tw.assert_equal("first solve (%s)" % first)
    expect(tw.solve(kernel=second), True, "second solve (%s)" % second, counters)
    tw.assert_kernel(pair=(second == "wave"))
    tw.assert_equal("second solve (%s)" % second)
    tw.assert_factors("hand-over %s -> %s" % (first, second))
    tw.close()


# ---- 6. mixed launch -----------------------------------------------------------------------------------------------
def case_mixed_launch(lib, randqp, monkeypatch, fam, counters=True, B=None):
    """update(H') on every other QP, nothing on the rest: one launch in which some workgroups factorise and some skip;
    then the same through a subset launch that covers QPs of both kinds"""
    f = family(fam, B)
    tw = Twins(lib, randqp, monkeypatch, f)
    expect(tw.solve(), False, "first solve", counters)
    H2 = _perturbed(tw, np.random.default_rng(13))[0]
    changed = np.arange(f.B) % 2 == 0
    for q in np.nonzero(changed)[0]:
        tw.both(lambda b: b.update(int(q), H=H2[q]))
    expect(tw.solve(), ~changed, "mixed launch", counters)
    tw.assert_kernel()
    tw.assert_equal("mixed launch")
    tw.assert_factors("%s mixed launch" % fam)
    # a subset launch: three quarters of the batch, the updated QPs among them updated once more
    sub = np.nonzero(np.arange(f.B) % 4 != 3)[0]
    H3 = H2 + 0.25 * np.eye(f.n)
    for q in np.nonzero(changed)[0]:
        tw.both(lambda b: b.update(int(q), H=H3[q]))
    cyc = tw.solve(launch=lambda b: b.solve_subset(sub))
    if counters:
        expect((cyc[0][sub], cyc[1][sub]), ~changed[sub], "subset launch", counters)
    tw.close()


# ---- 7. PrimalLDLT -------------------------------------------------------------------------------------------------
def case_primal_ldlt_never_skips(lib, randqp, monkeypatch, counters=True):
    """F holds P_J there and WU holds A_s^T A_s: the flag stays 0 and every solve rebuilds the model-only part"""
    fam = Family(20, 10, 20, 4, threads=256, backend=int(DenseBackend.PrimalLDLT))
    tw = Twins(lib, randqp, monkeypatch, fam)
    assert tw.a.dense_backend == int(DenseBackend.PrimalLDLT)
    for k in range(3):
        expect(tw.solve(), False, "PrimalLDLT solve %d" % k, counters)
        tw.assert_kernel()
        tw.assert_equal("PrimalLDLT solve %d" % k)
    tw.close()

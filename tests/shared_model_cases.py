"""Cases of the batches that share a model (csrc/pqp_shared.hpp: pqp_batch_init_shared / pqp_batch_update_shared,
pqp_batch_get_backward_sum, pqp_multi_init_shared, BatchQP.init_shared and the three torch layers), shared by
tests/test_emu_shared_model.py (CPU emulator) and tests/test_gpu_shared_model.py (MI355X).  `N` is proxsuite_amd._native
with the library under test loaded.

The gates are equalities of BITS: after init_shared / update_shared a handle holds what init / update with materialised
copies (np.broadcast_to(...).copy()) leave in a twin handle, so every getter and every later solve must agree bit for bit;
and the sum has a stated order (restated_sum below), so it is compared bit for bit with sequential `+` in a Python loop.
The one gate with a tolerance is the torch layers' gradient of a SHARED parameter against the fully expanded call's
sum(dim=0): two summation orders over the same B terms differ by at most (B - 1) u sum |term| per entry, u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), for each of them; the gate is B 2^-52 sum |term|.

The shapes are chosen for the two kernels, not for the workload: odd lengths (the 8-byte stores), even lengths (16-byte
stores), a length beyond one tile of 256 elements, absent blocks, box arrays, ranges that start inside the batch and
batches that cross a chunk of 64 QPs of the sum."""
import numpy as np
import pytest

NAMES = ("H", "g", "A", "b", "C", "l", "u", "l_box", "u_box")
JAC7 = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_du", "dL_dl")
JAC9 = JAC7 + ("dL_dl_box", "dL_du_box")
EPS = 1e-9
BW = (1e-5, 1e-7, 1e-7)
SUM_CHUNK = 64

# (n, n_eq, n_in, box): why
SHAPES = {"odd_lengths": (3, 1, 2, False),        # len 9, 3, 6: the 8-byte path
          "even_lengths": (4, 2, 2, False),       # the 16-byte path
          "beyond_a_tile": (17, 0, 3, False),     # len 289 > 256; no equalities: null arrays
          "no_inequalities": (5, 2, 0, False),
          "box": (4, 1, 2, True)}
MASKS = {"H_shared_A_per_qp": ("H",), "all_nine_shared": NAMES, "none_shared": (),
         "shared_l_box_per_qp_u_box": ("H", "A", "C", "l_box")}
ADDRESSING = [(s, m) for s in SHAPES for m in MASKS if m != "shared_l_box_per_qp_u_box" or SHAPES[s][3]]


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def on(device, a):
    """numpy for device None, else a tensor on `device`"""
    if a is None or device is None:
        return a
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def model(randqp, B, n, ne, ni, box, seed0=3):
    """dict name -> [B, ...] array, None for an absent block"""
    m = randqp.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.5, 1e-1, seed0=seed0)
    rng = np.random.default_rng(100 + seed0)
    out = dict(H=m.H, g=m.g, A=m.A if ne else None, b=m.b if ne else None, C=m.C if ni else None, l=m.l if ni else None,
               u=m.u if ni else None, l_box=None, u_box=None)
    if box:
        out["l_box"] = -1.0 - np.abs(rng.standard_normal((B, n)))
        out["u_box"] = 1.0 + np.abs(rng.standard_normal((B, n)))
    return out


def handle(N, B, n, ne, ni, box, **kw):
    b = N.Batch(B, n, ne, ni, box_constraints=box, **kw)
    b.set_all_settings(eps_abs=EPS, eps_rel=0.0)
    return b


def split(mod, first, count, shared):
    """(the arguments of init_shared over [first, first + count), the materialised [count, ...] arrays of the twin): a
    shared array is that of QP `first`"""
    args, twin = {}, {}
    for k, a in mod.items():
        if a is None:
            args[k] = twin[k] = None
        elif k in shared:
            args[k] = np.ascontiguousarray(a[first])
            twin[k] = np.broadcast_to(a[first], (count,) + a[first].shape).copy()
        else:
            args[k] = twin[k] = np.ascontiguousarray(a[first:first + count])
    return args, twin


def same_bits(a, b, what):
    a, b = host(a), host(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), \
        (what, int(np.count_nonzero(a != b)), a.size)


def same_scaled(h, t, slots, what):
    for q in slots:
        sa, sb = h.scaled(q), t.scaled(q)
        for k in sa:
            same_bits(np.asarray(sa[k]), np.asarray(sb[k]), "%s: scaled %s of slot %d" % (what, k, q))


def same_results(h, t, what):
    ra, rb = h.results(), t.results()
    for k, a, b in zip(("x", "y", "z"), ra, rb):
        same_bits(a, b, "%s: %s" % (what, k))
    for q in range(h.B):
        for f in ("iter", "iter_ext", "mu_updates", "status"):
            assert getattr(ra[5][q], f) == getattr(rb[5][q], f), (what, q, f)


# ---------------------------------------------------------------------------------------------------------------------
# broadcast addressing


def case_addressing(N, randqp, shape, mask, device=None):
    """B = 5, the range [1, 4), slots 0 and 4 initialised with other data before: every slot as in the twin"""
    n, ne, ni, box = SHAPES[shape]
    shared = MASKS[mask]
    B, first, count = 5, 1, 3
    mod = model(randqp, B, n, ne, ni, box)
    args, twin = split(mod, first, count, shared)
    h, t = handle(N, B, n, ne, ni, box), handle(N, B, n, ne, ni, box)
    one = lambda q: {k: (None if a is None else a[q]) for k, a in mod.items()}
    for q in (0, 4):
        h.init(q, **one(q))
    h.flush()
    before = {q: h.scaled(q) for q in (0, 4)}
    h.init_shared(first, count, shared=shared, **{k: on(device, a) for k, a in args.items()})
    full = {k: (None if a is None else np.concatenate([a[:1], twin[k], a[4:]])) for k, a in mod.items()}
    t.init(-1, **full)
    same_scaled(h, t, range(B), "%s %s" % (shape, mask))
    for q in (0, 4):
        after = h.scaled(q)
        for k in after:
            same_bits(np.asarray(after[k]), np.asarray(before[q][k]), "slot %d %s untouched" % (q, k))
    h.solve()
    t.solve()
    same_results(h, t, "%s %s after solve" % (shape, mask))
    h.close()
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# update


def case_update(N, randqp, device=None):
    """init_shared -> solve -> update_shared(H shared, g per QP) -> solve against init(-1) -> solve -> update(-1) -> solve"""
    n, ne, ni, box, B = 4, 2, 2, False, 4
    mod = model(randqp, B, n, ne, ni, box)
    args, twin = split(mod, 0, B, ("H", "A", "C"))
    h, t = handle(N, B, n, ne, ni, box), handle(N, B, n, ne, ni, box)
    h.init_shared(0, B, shared=("H", "A", "C"), **{k: on(device, a) for k, a in args.items()})
    t.init(-1, **twin)
    h.solve()
    t.solve()
    same_results(h, t, "first solve")
    H2 = 1.25 * mod["H"][1] + 0.5 * np.eye(n)
    g2 = mod["g"][::-1].copy()
    h.update_shared(0, B, H=on(device, H2), g=on(device, g2), shared=("H",))
    t.update(-1, H=np.broadcast_to(H2, (B, n, n)).copy(), g=g2)
    same_scaled(h, t, range(B), "after update")
    h.solve()
    t.solve()
    same_results(h, t, "second solve")
    h.close()
    t.close()


def case_update_of_a_fresh_qp(N, randqp):
    """update_shared over a range with one never-initialised QP: that QP is initialised, as update does"""
    n, ne, ni, box, B = 3, 1, 2, False, 3
    mod = model(randqp, B, n, ne, ni, box)
    args, twin = split(mod, 0, B, ("H", "C"))
    h, t = handle(N, B, n, ne, ni, box), handle(N, B, n, ne, ni, box)
    for b in (h, t):
        for q in (0, 1):
            b.init(q, **{k: (None if a is None else a[q]) for k, a in mod.items()})
        b.solve(0, 2)
    h.update_shared(0, B, shared=("H", "C"), update_preconditioner=True, **args)
    t.update(-1, update_preconditioner=True, **twin)
    same_scaled(h, t, range(B), "update with a fresh QP")
    h.solve()
    t.solve()
    same_results(h, t, "update with a fresh QP, solved")
    for q in range(B):
        for f in ("compute_preconditioner", "update_preconditioner", "default_rho"):
            assert getattr(h.settings(q), f) == getattr(t.settings(q), f), (q, f)
    h.close()
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# errors and edge cases


def case_errors(N, randqp):
    n, ne, ni, box, B = 3, 1, 2, False, 5
    mod = model(randqp, B, n, ne, ni, box)
    args, twin = split(mod, 0, B, ("H",))
    h, t = handle(N, B, n, ne, ni, box), handle(N, B, n, ne, ni, box)
    h.init(-1, **twin)
    t.init(-1, **twin)
    # count == 0: nothing happens, whatever the arrays say
    other, _ = split(model(randqp, B, n, ne, ni, box, seed0=9), 0, 0, ("H",))
    h.init_shared(2, 0, shared=("H",), **other)
    h.update_shared(5, 0, shared=("H",), **other)
    same_scaled(h, t, range(B), "count == 0")
    # the range sticks out of the batch
    part, _ = split(mod, 0, 3, ("H",))
    for first in (3, -1, 6):
        with pytest.raises(ValueError, match="range"):
            h.init_shared(first, 3, shared=("H",), **part)
        with pytest.raises(ValueError, match="range"):
            h.update_shared(first, 3, shared=("H",), **part)
    # box arrays on a handle without box constraints: the message of init / update
    for fn in (h.init_shared, h.update_shared):
        with pytest.raises(ValueError, match="wrong model setup"):
            fn(0, 3, shared=("H", "l_box"), l_box=np.zeros(n), **{k: v for k, v in part.items() if k != "l_box"})
    same_scaled(h, t, range(B), "after the errors")
    # a set mask bit of a null array is ignored
    n2, B2 = 5, 3
    mod2 = model(randqp, B2, n2, 0, 2, False)
    args2, twin2 = split(mod2, 0, B2, ("H", "C"))
    h2, t2 = handle(N, B2, n2, 0, 2, False), handle(N, B2, n2, 0, 2, False)
    h2.init_shared(0, B2, shared=1 | 4 | 8 | 16 | 128 | 256, **args2)  # (A, b, l_box, u_box are null)
    t2.init(-1, **twin2)
    same_scaled(h2, t2, range(B2), "bits of null arrays")
    with pytest.raises(ValueError):
        h2.init_shared(0, B2, shared=("Q",), **args2)
    for b in (h, t, h2, t2):
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# the sum


def restated_sum(a, first, count):
    """the order of csrc/pqp_shared.hpp with sequential `+`: chunks of 64 QPs from `first`, each added up in index order
    starting from its first term; the partials added in chunk order"""
    partials = []
    for c0 in range(first, first + count, SUM_CHUNK):
        acc = a[c0].copy()
        for q in range(c0 + 1, min(c0 + SUM_CHUNK, first + count)):
            acc = acc + a[q]
        partials.append(acc)
    tot = partials[0]
    for p in partials[1:]:
        tot = tot + p
    return tot


def check_sum(b, per_qp, first, count, names, device=None):
    got = b.backward_sum(first, count)
    assert sorted(got) == sorted(names)
    for k in names:
        if k in ("dL_dH", "dL_dg") or (count >= 60 and k in JAC7[:6]):  # (the generator's QPs have no active lower bound)
            assert np.any(per_qp[k][first:first + count]), k  # (a sum of zeros would prove nothing)
        same_bits(got[k], restated_sum(per_qp[k], first, count), "sum of %s over [%d, %d)" % (k, first, first + count))
    again = b.backward_sum(first, count)
    for k in names:
        same_bits(again[k], got[k], "second call, %s" % k)
    if device is not None:  # device output pointers: the same bits
        import torch
        into = {k: torch.full(got[k].shape, float("nan"), dtype=torch.float64, device=device) for k in names}
        b.backward_sum(first, count, into=into)
        for k in names:
            same_bits(into[k], got[k], "device output, %s" % k)
    # only what `into` names is written
    some = {names[0]: np.full_like(got[names[0]], np.nan)}
    b.backward_sum(first, count, into=some)
    same_bits(some[names[0]], got[names[0]], "a single output")


SUMS = {"crosses_a_chunk": (67, 0, 67), "one_qp": (1, 0, 1), "range_inside_the_batch": (70, 2, 65)}


def case_sum(N, randqp, which, device=None):
    """after pqp_batch_backward at (3, 1, 2)"""
    B, first, count = SUMS[which]
    n, ne, ni = 3, 1, 2
    mod = model(randqp, B, n, ne, ni, False)
    b = handle(N, B, n, ne, ni, False)
    b.init(-1, **mod)
    b.solve()
    with pytest.raises(ValueError):
        b.backward_sum()  # no backward pass yet
    ld = np.random.default_rng(5).standard_normal((B, n + ne + ni))
    b.backward(on(device, ld), *BW)
    check_sum(b, b.backward_results(-1), first, count, JAC7, device)
    with pytest.raises(ValueError, match="box"):
        b.backward_sum(first, count, into=dict(dL_dl_box=np.zeros(n)))
    with pytest.raises(ValueError, match="range"):
        b.backward_sum(first + 1, B - first)
    b.close()


def case_sum_box(N, randqp, device=None):
    """after pqp_batch_backward_box at (4, 1, 2) with box: nine sums"""
    n, ne, ni, B = 4, 1, 2, 6
    mod = model(randqp, B, n, ne, ni, True)
    # (bounds tight enough that some are active: dL_dl_box / dL_du_box are not all zero)
    mod["u_box"] = np.full((B, n), 0.05)
    mod["l_box"] = np.full((B, n), -0.05)
    b = handle(N, B, n, ne, ni, True)
    b.init(-1, **mod)
    b.solve()
    ld = np.random.default_rng(6).standard_normal((B, 1, n + ne + ni + n))
    b.backward_box(on(device, ld), *BW)
    per_qp = b.backward_box_results(-1)
    assert np.any(per_qp["dL_dl_box"][1:5]) and np.any(per_qp["dL_du_box"][1:5])
    check_sum(b, per_qp, 1, 4, JAC9, device)
    b.close()


def case_sum_closest_feasible(N, randqp, device=None):
    """after pqp_batch_backward_closest_feasible at (4, 1, 3), B = 3 (single-sided rows: l = -1e20)"""
    n, ne, ni, B = 4, 1, 3, 3
    mod = model(randqp, B, n, ne, ni, False)
    mod["l"] = np.full((B, ni), -1.0e20)
    b = N.Batch(B, n, ne, ni)
    b.set_all_settings(primal_infeasibility_solving=1, eps_abs=EPS, eps_rel=0.0)
    b.init(-1, **mod)
    b.solve()
    ld = np.random.default_rng(7).standard_normal((B, n + 2 * ne + 2 * ni))
    b.backward_closest_feasible(on(device, ld), 1e-9)
    per_qp = b.backward_results(-1)
    got = b.backward_sum()
    for k in JAC7:
        same_bits(got[k], restated_sum(per_qp[k], 0, B), "sum of %s" % k)
    for k in ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC"):  # (single-sided: dL_dl is identically zero)
        assert np.any(per_qp[k]), k
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# several shards


def case_multi(N, randqp, devices=(0, 0, 0)):
    """pqp_multi_init_shared over three (logical) shards, B = 7 at (3, 1, 2): the single handle's bits"""
    n, ne, ni, B = 3, 1, 2, 7
    mod = model(randqp, B, n, ne, ni, False)
    shared = ("H", "A", "C")
    args, twin = split(mod, 0, B, shared)
    m = N.MultiBatch(B, n, ne, ni, list(devices))
    t = handle(N, B, n, ne, ni, False)
    for q in range(B):
        s = m.settings(q)
        s.eps_abs, s.eps_rel = EPS, 0.0
    m.init_shared(0, B, shared=shared, **args)
    t.init(-1, **twin)
    m.solve()
    t.solve()
    same_results(m, t, "multi")
    # a range that starts inside the second shard and ends inside the third, H shared, the rest per QP
    first, count = 4, 3
    H2 = mod["H"][0] + np.eye(n)
    g2 = -mod["g"][first:first + count]
    m.update_shared(first, count, H=H2, g=g2, shared=("H",))
    for i in range(count):
        t.update(first + i, H=H2, g=g2[i])
    m.solve()
    t.solve()
    same_results(m, t, "multi, range update")
    with pytest.raises(ValueError, match="range"):
        m.init_shared(5, 3, shared=shared, **split(mod, 0, 3, shared)[0])
    m.close()
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# proxqp.dense.BatchQP


def case_batchqp(N, randqp):
    from proxsuite_amd.proxqp import dense
    n, ne, ni, B = 4, 2, 3, 5
    mod = model(randqp, B, n, ne, ni, False)
    shared = ("H", "A", "C")
    args, twin = split(mod, 0, B, shared)
    a, r = dense.BatchQP(B, device=0), dense.BatchQP(B, device=0)
    qps = a.init_shared(B, args["H"], args["g"], args["A"], args["b"], args["C"], args["l"], args["u"])
    assert len(qps) == B and a.size() == B
    for q in range(B):
        qp = r.init_qp_in_place(n, ne, ni)
        qp.init(*[twin[k][q] for k in NAMES[:7]])
    for batch in (a, r):
        for qp in batch:
            qp.settings.eps_abs, qp.settings.eps_rel = EPS, 0.0
    dense.solve_in_parallel(qps=a)
    dense.solve_in_parallel(qps=r)
    for q in range(B):
        for k in ("x", "y", "z"):
            same_bits(getattr(a[q].results, k), getattr(r[q].results, k), "BatchQP qp %d %s" % (q, k))
        assert a[q].results.info.iter == r[q].results.info.iter
    for k in shared:
        assert getattr(qps[0].model, k) is getattr(qps[3].model, k), k
        same_bits(getattr(qps[0].model, k), args[k], "model.%s" % k)
    assert qps[0].model.g is not qps[3].model.g
    same_bits(qps[3].model.g, mod["g"][3], "model.g")
    # a single update afterwards replaces that QP's entry alone
    g_new = mod["g"][0] * 2.0
    qps[2].update(g=g_new)
    r[2].update(g=g_new)
    same_bits(qps[2].model.g, g_new, "model.g after update")
    same_bits(qps[1].model.g, mod["g"][1], "the neighbour's model.g")
    # update_shared of all of them: a new shared H, per-QP u
    H2 = mod["H"][2] + 0.25 * np.eye(n)
    u2 = mod["u"] + 0.5
    a.update_shared(H=H2, u=u2)
    for q in range(B):
        r[q].update(H=H2, u=u2[q])
    assert qps[0].model.H is qps[4].model.H
    dense.solve_in_parallel(qps=a)
    dense.solve_in_parallel(qps=r)
    for q in range(B):
        for k in ("x", "y", "z"):
            same_bits(getattr(a[q].results, k), getattr(r[q].results, k), "BatchQP after update_shared, qp %d %s" % (q, k))


# ---------------------------------------------------------------------------------------------------------------------
# the torch layers


LAYERS = ("feasible", "closest_feasible", "box")


def _layer(which):
    from proxsuite_amd.torch import qplayer
    if which == "box":
        return qplayer.QPFunctionBox(eps=EPS, maxIter=1000, eps_backward=1e-9)
    # (closest-feasible forwards stall short of eps on an infeasible QP and then only repeat outer iterations -- minutes on
    # the emulator, see tests/infeas_backward_cases.py: 50 of them; the comparisons are between two runs of the same forward)
    return qplayer.QPFunction(eps=EPS, maxIter=1000 if which == "feasible" else 50, eps_backward=1e-9,
                              structural_feasibility=which == "feasible")


def _layer_run(which, mod, shared, device, seed=11):
    """loss = fixed random weights times every output; (outputs, gradients by name) as numpy"""
    import torch
    names = NAMES if which == "box" else NAMES[:7]
    params = {k: torch.tensor(mod[k][0] if k in shared else mod[k], dtype=torch.float64, device=device, requires_grad=True)
              for k in names}
    outs = _layer(which)(*[params[k] for k in names])
    rng = np.random.default_rng(seed)
    loss = sum((torch.tensor(rng.standard_normal(tuple(o.shape)), device=device) * o).sum() for o in outs)
    loss.backward()
    return [host(o) for o in outs], {k: host(params[k].grad) for k in names}


def layer_model(randqp, which, B, n, ne, ni):
    """Q, A, G the same in every QP; p, b, l, u (and the box) of the QP's own"""
    mod = model(randqp, B, n, ne, ni, which == "box", seed0=21)
    for k in ("H", "A", "C"):
        mod[k] = np.broadcast_to(mod[k][0], mod[k].shape).copy()
    if which == "box":
        mod["l_box"], mod["u_box"] = np.full((B, n), -0.05), np.full((B, n), 0.05)
    return mod


def case_layer(which, randqp, device="cpu"):
    """Q, A, G shared, the vectors batched, at (6, 2, 4), B = 5, against the fully expanded call"""
    n, ne, ni, B = 6, 2, 4, 5
    mod = layer_model(randqp, which, B, n, ne, ni)
    outs_f, full = _layer_run(which, mod, (), device)
    outs_s, shared = _layer_run(which, mod, ("H", "A", "C"), device)
    for i, (a, b) in enumerate(zip(outs_s, outs_f)):
        same_bits(a, b, "%s: output %d" % (which, i))
    for k in full:
        if k in ("H", "A", "C"):
            assert shared[k].shape == full[k].shape[1:], k
            bound = B * 2.0 ** -52 * np.sum(np.abs(full[k]), axis=0)
            err = np.abs(shared[k] - full[k].sum(axis=0))
            print("%s d%s: max error %.3e, max bound %.3e" % (which, k, err.max(), bound.max()))
            assert np.any(full[k]), k
            assert np.all(err <= bound), (which, k, float(np.max(err - bound)))
        else:
            same_bits(shared[k], full[k], "%s: gradient of %s" % (which, k))


def case_layer_everything_shared(which, randqp, device="cpu"):
    """every parameter without a batch dimension: one QP"""
    n, ne, ni = 6, 2, 4
    mod = layer_model(randqp, which, 1, n, ne, ni)
    names = NAMES if which == "box" else NAMES[:7]
    outs_f, full = _layer_run(which, mod, (), device)
    outs_s, shared = _layer_run(which, mod, names, device)
    for i, (a, b) in enumerate(zip(outs_s, outs_f)):
        same_bits(a, b, "%s: output %d" % (which, i))
    for k in names:
        same_bits(shared[k], full[k][0], "%s: gradient of %s" % (which, k))


def case_layer_allocates_no_expanded_copy(randqp, device="cuda"):
    """forward + backward of QPFunction at B = 256, (20, 5, 10) with Q, A, G shared: the peak of the allocator over its
    baseline stays under the B n n doubles of ONE expanded Q"""
    import torch
    n, ne, ni, B = 20, 5, 10, 256
    mod = layer_model(randqp, "feasible", B, n, ne, ni)
    names = NAMES[:7]
    params = {k: torch.tensor(mod[k][0] if k in ("H", "A", "C") else mod[k], dtype=torch.float64, device=device,
                              requires_grad=True) for k in names}
    w = torch.tensor(np.random.default_rng(3).standard_normal((B, n)), device=device)
    f = _layer("feasible")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    x, _, _ = f(*[params[k] for k in names])
    (w * x).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak over the baseline: %d bytes; B n n doubles: %d bytes" % (peak, B * n * n * 8))
    assert params["H"].grad is not None and tuple(params["H"].grad.shape) == (n, n)
    assert peak < B * n * n * 8, (peak, B * n * n * 8)

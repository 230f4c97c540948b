"""QPFunction: the forward of `proxsuite.torch.qplayer.QPFunction` on MI355X.

Mirrors reference bindings/python/proxsuite/torch/qplayer.py:12-167 (feasible QPs) and
:255-369 (closest-feasible QPs, `structural_feasibility=False`): same factory arguments,
same solver settings (max_iter = maxIter, max_iter_in = 100, rho = 5e-5 with
refactor_rho_threshold = rho, eps_abs = eps), same outputs.  The reference loops over the
batch in Python, copies every matrix to numpy, and calls init/solve per QP; here the whole
batch goes through ONE pqp_batch_init (pointers of the torch tensors, host or ROCm, are
handed to the C-ABI as they are), ONE solve launch with one workgroup per QP, and the
results are copied device-to-device into the output tensors.

The backward pass (reference qplayer.py:172-253) is ONE pqp_batch_backward launch (the device
form of dense/compute_ECJ.hpp's compute_backward for every QP of the batch) whose seven jacobians
are copied device-to-device into the gradient tensors.

Parameters WITHOUT a batch dimension (2-D Q, A, G; 1-D vectors: a layer's weights) are shared by the batch and stay as
they are: they go through ONE pqp_batch_init_shared, which gives them to every QP on the device, and their gradients are the
per-QP jacobians summed on the device (pqp_batch_get_backward_sum, csrc/pqp_shared.hpp); no [B, ...] tensor is made for them.

Forward mode: `solution_tangents` (one forward, one pqp_batch_tangent_multi call) and a `jvp` on the feasible layer's
Function, so that torch.autograd.forward_ad works through QPFunction(structural_feasibility=True): the tangents of
(x, y, z) for the tangents of the seven parameters, one refined KKT solve on the factorisation of the backward pass
(csrc/pqp_tangent.hpp).  The closest-feasible layer and QPFunctionBox have no jvp.

The closest-feasible variant (`structural_feasibility=False`) differentiates through its sparse backend in the
reference (qplayer.py:371-610): per QP a rectangular linear system K w = r, solved as a QP with zero Hessian, K as
equality constraints and primal_infeasibility_solving.  That QP is dense and of the kind this engine solves, so here the
backward is ONE pqp_batch_backward_closest_feasible call: a kernel assembles K and r of every QP in the model arrays of
an inner batch handle, the engine solves them, a second kernel forms the jacobians (csrc/pqp_infeas.hpp, DESIGN.md
section 3g).  Three departures from the reference's Python, decided by the chain rule and by finite differences:
dG = dG1[n_in:] - dG1[:n_in] of the single-sided G1 = [-G; G] (the reference keeps one half), parameters shared by the
batch receive the SUM of the per-QP gradients (the reference: the mean), and everything stays in fp64.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from .. import _native
from .._ctypes_defs import DenseBackend, HessianType, InitialGuess


def _extract_nbatch(*params_and_dims):
    for param, dim in params_and_dims:
        if param.ndimension() == dim:
            return param.size(0)
    return 1


def _expand(X, nbatch, ndim):
    # reference bindings/python/proxsuite/torch/utils.py:57-63
    if X.ndimension() in (0, ndim) or X.nelement() == 0:
        return X
    if X.ndimension() == ndim - 1:
        return X.unsqueeze(0).expand(*([nbatch] + list(X.size())))
    raise RuntimeError("Unexpected number of dimensions.")


def _dense64(t):
    return t.detach().to(torch.float64).contiguous()


# Native batch handles are kept per (batch, dim, n_eq, n_in, device, box_constraints) signature: creating one costs
# ~45 device allocations + memsets (25 ms at 2048 x (100, 50, 100), against 10 ms for the solve).  A
# forward checks a handle out; it goes back when the autograd context that owns it dies (after the
# backward, or with the graph), so two layers of one shape in the same graph never share a handle.
_FREE = {}
_KEEP = 4


def _checkout(key):
    free = _FREE.setdefault(key, [])
    if free:
        batch = free.pop()
        # a reused handle must look like the fresh QP objects the reference builds at every forward:
        # QP::cleanup() resets results and the proximal parameters (the previous backward left
        # rho = rho_backward, mu = mu_backward in results.info, and init(..., rho=...) keeps mu)
        batch.cleanup(-1)
        return batch
    nbatch, nz, neq, nineq, index, box = key
    return _native.Batch(nbatch, nz, neq, nineq, box_constraints=box, hessian_type=int(HessianType.Dense),
                         dense_backend=int(DenseBackend.Automatic), device=index)


def _give_back(key, batch):
    free = _FREE.setdefault(key, [])
    if len(free) < _KEEP:
        free.append(batch)
    else:
        batch.close()


class _Lease:
    """ties a checked-out handle to the lifetime of its autograd context"""

    def __init__(self, key, batch):
        self.key, self.batch = key, batch

    def __del__(self):
        try:
            _give_back(self.key, self.batch)
        except Exception:
            pass


def _solve_batch(Q, p, A, b, G, l, u, eps, max_iter, infeasible, l_box=None, u_box=None, nbatch=None):
    """The parameters as the caller holds them: a matrix with 2 dimensions / a vector with 1 is SHARED by the `nbatch` QPs
    and goes through Batch.init_shared as it is -- one copy of it reaches the handle and is given to every QP on the
    device (csrc/pqp_shared.hpp); nothing of nbatch times its size is materialised.  `nbatch` None: every parameter
    carries the batch dimension (pqp_batch_init).  `l_box` / `u_box` ([nbatch, nz] or [nz]): the handle has box
    constraints (QPFunctionBox); G may then be empty and z is [nbatch, nineq + nz] = [z_in | z_box]"""
    box = l_box is not None
    nbatch, nz = p.size(0) if nbatch is None else nbatch, p.size(-1)
    nineq = G.size(-2) if G.nelement() > 0 else 0
    neq = A.size(-2) if A.nelement() > 0 else 0
    assert neq > 0 or nineq > 0 or box
    dev = Q.device
    index = dev.index if dev.type == "cuda" and dev.index is not None else 0
    key = (int(nbatch), int(nz), int(neq), int(nineq), int(index), box)
    batch = _checkout(key)
    lease = _Lease(key, batch)
    rho = 5.0e-5
    # (one vectorised write per field over the handle's settings table: the per-QP Python loop cost ~5 ms at 2048 QPs)
    batch.set_all_settings(primal_infeasibility_solving=int(infeasible), max_iter=max_iter, max_iter_in=100,
                           default_rho=rho, refactor_rho_threshold=rho,  # no refactorization
                           eps_abs=eps,
                           initial_guess=int(InitialGuess.EQUALITY_CONSTRAINED_INITIAL_GUESS))  # (restated for reused handles)
    if dev.type == "cuda":
        # kernels go to the caller's stream; the model copies of init are blocking copies on the
        # null stream, which are ordered after torch's default stream -- only a side stream with
        # inputs still in flight needs an explicit wait
        cur = torch.cuda.current_stream(dev)
        batch.set_stream(cur.cuda_stream)
        if cur != torch.cuda.default_stream(dev):
            cur.synchronize()
    model = dict(H=_dense64(Q), g=_dense64(p), A=_dense64(A) if neq else None, b=_dense64(b) if neq else None,
                 C=_dense64(G) if nineq else None, l=_dense64(l) if nineq else None, u=_dense64(u) if nineq else None,
                 l_box=_dense64(l_box) if box else None, u_box=_dense64(u_box) if box else None)
    shared = [k for k, t in model.items() if t is not None and t.ndimension() == (2 if k in ("H", "A", "C") else 1)]
    if shared:
        batch.init_shared(0, nbatch, shared=shared, rho=rho, **model)
    else:
        batch.init(-1, rho=rho, **model)
    batch.solve()
    opts = dict(dtype=torch.float64, device=dev)
    x = torch.empty((nbatch, nz), **opts)
    y = torch.empty((nbatch, neq), **opts)
    z = torch.empty((nbatch, batch.n_c), **opts)
    se = torch.empty((nbatch, neq), **opts)
    si = torch.empty((nbatch, batch.n_c), **opts)
    batch.results_into(x, y, z, se, si)
    return lease, x, y, z, se, si


def _gradients(batch, names, batched, shapes, dev, dtype, box=False):
    """The gradient of every parameter of a layer from the jacobians the backward launch left in the handle.  names[i]:
    the jacobian of parameter i; batched[i]: it carries the batch dimension and receives the per-QP jacobians
    (Batch.backward_results); a parameter shared by the batch receives their SUM, formed on the device
    (Batch.backward_sum): no [B, ...] tensor is allocated or fetched for it.  shapes[i] == (): the parameter is absent."""
    B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in
    one = dict(dL_dH=(n, n), dL_dg=(n,), dL_dA=(ne, n), dL_db=(ne,), dL_dC=(ni, n), dL_du=(ni,), dL_dl=(ni,),
               dL_dl_box=(n,), dL_du_box=(n,))
    opts = dict(dtype=torch.float64, device=dev)
    per = {k: torch.empty((B,) + one[k], **opts) for i, k in enumerate(names) if len(shapes[i]) and batched[i]}
    tot = {k: torch.empty(one[k], **opts) for i, k in enumerate(names) if len(shapes[i]) and not batched[i]}
    if per:
        (batch.backward_box_results if box else batch.backward_results)(-1, into=per)
    if tot:
        batch.backward_sum(0, B, into=tot)
    return per, tot


def solution_jacobians(Q, p, A, b, G, l, u, eps=1e-9, maxIter=1000, eps_backward=1.0e-4, rho_backward=1.0e-6,
                       mu_backward=1.0e-6):
    """The solution of a batch of QPs and its jacobians wrt the vectors of the model: one forward solve with the settings
    of QPFunction, then ONE backward launch with K = n loss derivatives per QP ([I_n | 0]: one factorisation per QP
    instead of the n that a loop of autograd.grad calls over the components of x pays).  Returns
    (x [B, n], dx/dp [B, n, n], dx/db [B, n, n_eq], dx/dl [B, n, n_in], dx/du [B, n, n_in]) on the inputs' device."""
    nbatch = _extract_nbatch((Q, 3), (p, 2), (A, 3), (b, 2), (G, 3), (l, 2), (u, 2))
    Q_, p_, G_ = _expand(Q, nbatch, 3), _expand(p, nbatch, 2), _expand(G, nbatch, 3)
    u_, l_ = _expand(u, nbatch, 2), _expand(l, nbatch, 2)
    A_, b_ = _expand(A, nbatch, 3), _expand(b, nbatch, 2)
    lease, x, _, _, _, _ = _solve_batch(Q_, p_, A_, b_, G_, l_, u_, eps, maxIter, infeasible=False)
    batch, dev = lease.batch, Q_.device
    B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in
    ld = torch.zeros((B, n, n + ne + ni), dtype=torch.float64, device=dev)
    ld[:, :, :n] = torch.eye(n, dtype=torch.float64, device=dev)
    V, act = batch.backward_multi(ld, eps_backward, rho_backward, mu_backward)
    Vz, zero = V[:, :, n + ne:], torch.zeros((), dtype=torch.float64, device=dev)
    up, low = ((act & 1) != 0).unsqueeze(1), ((act & 2) != 0).unsqueeze(1)
    t = Q.dtype
    return (x.to(t), V[:, :, :n].to(t), (-V[:, :, n:n + ne]).to(t), torch.where(low, -Vz, zero).to(t),
            torch.where(up, -Vz, zero).to(t))


def _tangents(batch, dev, shapes, batched, tangents, eps_backward, rho_backward, mu_backward):
    """(dx, dy, dz) in fp64 for ONE direction.  shapes[i] / batched[i]: the shape of parameter i (() when it is absent) and
    whether it carries the batch dimension; tangents[i] (None: zero) has that shape.  A parameter without batch dimension
    is shared by the batch and its tangent goes in as it is, with its shared bit"""
    B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in
    names = ("H", "g", "A", "b", "C", "l", "u")
    args, shared = {}, []
    for name, shape, bt, t in zip(names, shapes, batched, tangents):
        if t is None or not len(shape):
            continue
        if tuple(t.shape) != tuple(shape):
            raise ValueError("the tangent of %s has shape %s, its parameter %s" % (name, tuple(t.shape), tuple(shape)))
        t = _dense64(t).to(dev)
        if bt:
            args["d" + name] = t.unsqueeze(1)  # [B, 1, ...]
        else:
            args["d" + name] = t.unsqueeze(0)  # [1, ...]: one block for every QP
            shared.append(name)
    if not args:
        zero = lambda k: torch.zeros((B, k), dtype=torch.float64, device=dev)
        return zero(n), zero(ne), zero(ni)
    T, _ = batch.tangent_multi(eps_backward, rho_backward, mu_backward, shared=shared, **args)
    return T[:, 0, :n].clone(), T[:, 0, n:n + ne].clone(), T[:, 0, n + ne:].clone()


def _shapes_and_batched(params):
    """what QPFunction keeps of its seven parameters: the shape (() for an absent one) and whether it carries the batch dimension"""
    dims = (3, 2, 3, 2, 3, 2, 2)
    return (tuple(tuple(t_.shape) if t_.numel() else () for t_ in params),
            tuple(t_.ndimension() == d for t_, d in zip(params, dims)))


def solution_tangents(Q, p, A, b, G, l, u, dQ=None, dp=None, dA=None, db=None, dG=None, dl=None, du=None, eps=1e-9,
                      maxIter=1000, eps_backward=1.0e-4, rho_backward=1.0e-6, mu_backward=1.0e-6):
    """The solution of a batch of QPs and its directional derivative: one forward solve with the settings of QPFunction,
    then ONE tangent call (pqp_batch_tangent_multi).  A tangent has the shape of its parameter (a parameter without batch
    dimension is shared by the batch, and so is its tangent); None is a zero tangent.  Returns (x, y, z, dx, dy, dz) on
    the inputs' device, in the inputs' dtype."""
    nbatch = _extract_nbatch((Q, 3), (p, 2), (A, 3), (b, 2), (G, 3), (l, 2), (u, 2))
    lease, x, y, z, _, _ = _solve_batch(Q, p, A, b, G, l, u, eps, maxIter, infeasible=False, nbatch=nbatch)
    shapes, batched = _shapes_and_batched((Q, p, A, b, G, l, u))
    d = _tangents(lease.batch, Q.device, shapes, batched, (dQ, dp, dA, db, dG, dl, du), eps_backward, rho_backward,
                  mu_backward)
    t = Q.dtype
    return (x.to(t), y.to(t), z.to(t)) + tuple(v.to(t) for v in d)


def QPFunction(eps=1e-9, maxIter=1000, eps_backward=1.0e-4, rho_backward=1.0e-6, mu_backward=1.0e-6,
               omp_parallel=False, structural_feasibility=True):
    """Factory with the reference's signature (qplayer.py:12-20).  `omp_parallel` is accepted and
    ignored: the batch is always solved in one launch.  The feasible layer (`structural_feasibility=True`) also has a
    `jvp`: torch.autograd.forward_ad works through it.  The closest-feasible layer and QPFunctionBox have none."""

    class QPFunctionFn(Function):
        @staticmethod
        def forward(ctx, Q_, p_, A_, b_, G_, l_, u_):
            nbatch = _extract_nbatch((Q_, 3), (p_, 2), (A_, 3), (b_, 2), (G_, 3), (l_, 2), (u_, 2))
            # (parameters shared by the batch stay as they are: _solve_batch hands them to init_shared)
            lease, x, y, z, _, _ = _solve_batch(Q_, p_, A_, b_, G_, l_, u_, eps, maxIter, infeasible=False, nbatch=nbatch)
            ctx.lease = lease  # the handle returns to the cache when this context is collected
            ctx.batch = lease.batch
            ctx.dev = Q_.device
            ctx.dtype = Q_.dtype
            ctx.shapes = tuple(tuple(t_.shape) if t_.numel() else () for t_ in (Q_, p_, A_, b_, G_, l_, u_))
            ctx.batched = (Q_.ndimension() == 3, p_.ndimension() == 2, A_.ndimension() == 3, b_.ndimension() == 2,
                           G_.ndimension() == 3, l_.ndimension() == 2, u_.ndimension() == 2)
            return x.to(Q_.dtype), y.to(Q_.dtype), z.to(Q_.dtype)

        @staticmethod
        def jvp(ctx, *tangents):
            # forward mode (torch.autograd.forward_ad): one tangent call on the handle the forward left solved.  An input
            # without a tangent arrives as None and reaches the library as a null pointer.  The call reads (x, y, z) and
            # the scaled model and rewrites only what backward() rewrites, so a later backward() finds what it needs.
            d = _tangents(ctx.batch, ctx.dev, ctx.shapes, ctx.batched, tangents, eps_backward, rho_backward, mu_backward)
            return tuple(v.to(ctx.dtype) for v in d)

        @staticmethod
        def backward(ctx, dl_dzhat, dl_dlams, dl_dnus):
            batch, dev = ctx.batch, ctx.dev
            B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in
            ld = torch.zeros((B, n + ne + ni), dtype=torch.float64, device=dev)
            ld[:, :n] = dl_dzhat
            if dl_dlams is not None and ne:
                ld[:, n:n + ne] = dl_dlams
            if dl_dnus is not None and ni:
                ld[:, n + ne:] = dl_dnus
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
            batch.backward(ld, eps_backward, rho_backward, mu_backward)
            bt, sh, t = ctx.batched, ctx.shapes, ctx.dtype
            names = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_dl", "dL_du")
            # parameters shared by the batch receive the sum of the per-QP gradients
            per, tot = _gradients(batch, names, bt, sh, dev, t)
            return tuple((per[k] if bt[i] else tot[k]).to(t).reshape(sh[i]) if len(sh[i]) else None
                         for i, k in enumerate(names))

    class QPFunctionFn_infeas(Function):
        @staticmethod
        def forward(ctx, Q_, p_, A_, b_, G_, l_, u_):
            n_in, nz = G_.size()[-2:]
            nbatch = _extract_nbatch((Q_, 3), (p_, 2), (A_, 3), (b_, 2), (G_, 3), (l_, 2), (u_, 2))
            # single-sided restatement, as the reference does (qplayer.py:270-271), of the parameters as they are: G1 of
            # a shared G is shared; h is shared when both l and u are (else the shared one of the two vectors is expanded)
            if l_.ndimension() != u_.ndimension():
                l, u = _expand(l_, nbatch, 2), _expand(u_, nbatch, 2)
            else:
                l, u = l_, u_
            h = torch.cat((-l, u), dim=-1)
            G1 = torch.cat((-G_, G_), dim=-2)
            lo = torch.full((2 * int(n_in),), -1.0e20, dtype=h.dtype, device=h.device)  # (the same for every QP)
            lease, x, y, z, se, si = _solve_batch(Q_, p_, A_, b_, G1, lo, h, eps, maxIter, infeasible=True, nbatch=nbatch)
            Q = Q_
            ctx.lease = lease
            ctx.batch = lease.batch  # (its result arrays are the inputs of the backward)
            ctx.n_in = int(n_in)
            ctx.dev = Q.device
            ctx.dtype = Q.dtype
            ctx.shapes = tuple(tuple(t_.shape) if t_.numel() else () for t_ in (Q_, p_, A_, b_, G_, l_, u_))
            ctx.batched = (Q_.ndimension() == 3, p_.ndimension() == 2, A_.ndimension() == 3, b_.ndimension() == 2,
                           G_.ndimension() == 3, l_.ndimension() == 2, u_.ndimension() == 2)
            # the active half of every double-sided row (reference qplayer.py:480)
            ctx.active = (-z[:, :n_in] + z[:, n_in:]) >= 0
            nus_sol = -z[:, :n_in] + z[:, n_in:]
            s_i = -si[:, :n_in] + si[:, n_in:]
            t = Q.dtype
            return x.to(t), y.to(t), nus_sol.to(t), se.to(t), s_i.to(t)

        @staticmethod
        def backward(ctx, dl_dzhat, dl_dlams, dl_dnus, dl_ds_e, dl_ds_i):
            batch, dev, ns = ctx.batch, ctx.dev, ctx.n_in
            B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in  # (ni = 2 ns: the single-sided QP)
            # rows (dl/dx | dl/dlam | dl/dnu | dl/dse | dl/dsi) of the single-sided QP; the kernel negates them into the
            # right-hand side, which then equals the reference's (qplayer.py:473-503): a double-sided derivative goes to
            # the first half (-G) where the row is not active from above, negated, and to the second half where it is
            ld = torch.zeros((B, n + 2 * ne + 2 * ni), dtype=torch.float64, device=dev)
            act = ctx.active

            def halves(at, v):
                v = v.to(torch.float64)
                zero = torch.zeros((), dtype=torch.float64, device=dev)
                ld[:, at:at + ns] = torch.where(act, zero, -v)
                ld[:, at + ns:at + ni] = torch.where(act, v, zero)

            if dl_dzhat is not None:
                ld[:, :n] = dl_dzhat
            if dl_dlams is not None and ne:
                ld[:, n:n + ne] = dl_dlams
            if dl_dnus is not None and ni:
                halves(n + ne, dl_dnus)
            if dl_ds_e is not None and ne:
                ld[:, n + ne + ni:n + 2 * ne + ni] = dl_ds_e
            if dl_ds_i is not None and ni:
                halves(n + 2 * ne + ni, dl_ds_i)
            batch.backward_closest_feasible(ld, eps_backward)
            bt, sh, t = ctx.batched, ctx.shapes, ctx.dtype
            # the jacobians of the single-sided QP: l and u both come from dL_du of h = [-l; u], per QP for the batched
            # one of the two and summed for the shared one.  dL_dC is fetched per QP even for a shared G: its two halves
            # are the jacobians of -G and G, which cancel in the fold below (1e8 against 1e2 at eps_backward = 1e-9), so
            # the fold has to come BEFORE the sum
            names = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_du", "dL_du")
            fetch = tuple(b or i == 4 for i, b in enumerate(bt))
            per, tot = _gradients(batch, names, fetch, sh, dev, t)
            pick = lambda i: per[names[i]] if fetch[i] else tot[names[i]]
            # back to the double-sided parameters: G1 = [-G; G], h = [-l; u]
            fold = (lambda g: g, lambda g: g, lambda g: g, lambda g: g, lambda g: g[:, ns:] - g[:, :ns],
                    lambda g: -g[..., :ns], lambda g: g[..., ns:])
            # parameters shared by the batch receive the sum of the per-QP gradients
            grads = [fold[i](pick(i)) if len(sh[i]) else None for i in range(7)]
            if grads[4] is not None and not bt[4]:
                grads[4] = grads[4].sum(dim=0)
            return tuple(g.to(t).reshape(sh[i]) if g is not None else None for i, g in enumerate(grads))

    return QPFunctionFn.apply if structural_feasibility else QPFunctionFn_infeas.apply


def QPFunctionBox(eps=1e-9, maxIter=1000, eps_backward=1.0e-4, rho_backward=1.0e-6, mu_backward=1.0e-6):
    """QPFunction for QPs with variable bounds l_box <= x <= u_box: the function takes (Q, p, A, b, G, l, u, l_box, u_box)
    and returns (x, y, z, z_box).  The bounds are box constraints of the engine (a handle created with box_constraints:
    one scaled column per bound instead of a dense identity row under G), and the backward is ONE pqp_batch_backward_box
    call with one loss derivative per QP, whose nine jacobians are copied device-to-device into the gradient tensors.
    Parameters shared by the batch are handled as in QPFunction and receive the sum of the per-QP gradients.  G (with l
    and u) may be empty."""

    class QPFunctionBoxFn(Function):
        @staticmethod
        def forward(ctx, Q_, p_, A_, b_, G_, l_, u_, lb_, ub_):
            nbatch = _extract_nbatch((Q_, 3), (p_, 2), (A_, 3), (b_, 2), (G_, 3), (l_, 2), (u_, 2), (lb_, 2), (ub_, 2))
            lease, x, y, z, _, _ = _solve_batch(Q_, p_, A_, b_, G_, l_, u_, eps, maxIter, infeasible=False, l_box=lb_,
                                                u_box=ub_, nbatch=nbatch)
            Q = Q_
            ctx.lease = lease  # the handle returns to the cache when this context is collected
            ctx.batch = lease.batch
            ctx.dev = Q.device
            ctx.dtype = Q.dtype
            ins = (Q_, p_, A_, b_, G_, l_, u_, lb_, ub_)
            ctx.shapes = tuple(tuple(t_.shape) if t_.numel() else () for t_ in ins)
            ctx.batched = tuple(t_.ndimension() == d for t_, d in zip(ins, (3, 2, 3, 2, 3, 2, 2, 2, 2)))
            ni = lease.batch.n_in
            t = Q.dtype
            return x.to(t), y.to(t), z[:, :ni].to(t), z[:, ni:].to(t)

        @staticmethod
        def backward(ctx, dl_dx, dl_dy, dl_dz, dl_dzbox):
            batch, dev = ctx.batch, ctx.dev
            B, n, ne, ni = batch.B, batch.n, batch.n_eq, batch.n_in
            ld = torch.zeros((B, 1, n + ne + ni + n), dtype=torch.float64, device=dev)
            if dl_dx is not None:
                ld[:, 0, :n] = dl_dx
            if dl_dy is not None and ne:
                ld[:, 0, n:n + ne] = dl_dy
            if dl_dz is not None and ni:
                ld[:, 0, n + ne:n + ne + ni] = dl_dz
            if dl_dzbox is not None:
                ld[:, 0, n + ne + ni:] = dl_dzbox
            batch.backward_box(ld, eps_backward, rho_backward, mu_backward)  # (synchronises the caller's stream itself)
            bt, sh, t = ctx.batched, ctx.shapes, ctx.dtype
            names = ("dL_dH", "dL_dg", "dL_dA", "dL_db", "dL_dC", "dL_dl", "dL_du", "dL_dl_box", "dL_du_box")
            # parameters shared by the batch receive the sum of the per-QP gradients
            per, tot = _gradients(batch, names, bt, sh, dev, t, box=True)
            return tuple((per[k] if bt[i] else tot[k]).to(t).reshape(sh[i]) if len(sh[i]) else None
                         for i, k in enumerate(names))

    return QPFunctionBoxFn.apply

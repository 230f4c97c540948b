#!/usr/bin/env python
"""Batches that share a model (csrc/pqp_shared.hpp) against the same batches with materialised copies.  Stand-alone:
bench.py and its flagship workload are not involved.

    python scripts/shared_model_bench.py [--out profiles/shared_model.txt] [--repeats 20] [--quick] [--lib PATH]

Case (a), host buffers, 2048 x (100, 50, 100): pqp_batch_init(-1) with B materialised copies of H, A, C against
pqp_batch_init_shared with H, A, C shared (g, b, l, u per QP in both).  Figures: host wall time of init + flush, and
the inclusive rate init + flush + solve + results to the host, in QPs/s.

Case (b), ROCm tensors: QPFunction forward + backward with Q, A, G shared (2-D) and p, b, l, u batched, B in {256, 2048},
at (100, 50, 100).  "shared": the layer as it is (init_shared, backward_sum).  "expanded": the same call with Q, A, G
expanded to [B, ...] views beforehand, which is the parent commit's path through the layer (B contiguous copies handed to
init, B per-QP jacobians fetched and summed).  --lib PATH adds "expanded, other library": that path on another build
of libproxqp_hip.so (the parent commit's).

Every figure is the median [min .. max] of `--repeats` rounds after one warm-up round, the contenders of a case
alternating within a round."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shared_model(R, B, n, ne, ni, seed=0):
    """H, A, C of one QP; g of each QP; b, l, u around a point of each QP (every QP is feasible)"""
    m = R.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2, seed0=seed)
    H, A, C = m.H[0].copy(), m.A[0].copy(), m.C[0].copy()
    x0 = np.random.default_rng(seed).standard_normal((B, n))
    Cx = x0 @ C.T
    return dict(H=H, A=A, C=C, g=m.g.copy(), b=x0 @ A.T, l=Cx - 1.0, u=Cx + 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_model.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--lib", default=None, help="another build of libproxqp_hip.so (the parent commit's) for case (b)")
    a = ap.parse_args()

    import torch
    from proxsuite_amd import _native as N
    from proxsuite_amd.torch import qplayer
    from proxsuite_amd.utils import random_qp as R
    lib = N.load()  # (fails loudly without the library or a device: no fall-back, no number)
    other = N.NativeLib(a.lib, legacy=True) if a.lib else None
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: "%9.3f [%9.3f .. %9.3f]" % (statistics.median(v), min(v), max(v))
    n, ne, ni = (100, 50, 100) if not a.quick else (10, 4, 7)
    rel = lambda p: os.path.relpath(os.path.abspath(p), ROOT)
    say("# library: %s%s" % (rel(lib.path), "; other library: %s" % rel(other.path) if other else ""))
    say("# scripts/shared_model_bench.py: shape (%d, %d, %d), %d rounds per figure after one warm-up round, median [min .. max], "
        "host wall ms; device %s" % (n, ne, ni, a.repeats, torch.cuda.get_device_name(0)))
    say("# box before: %s" % N.box_calibration())

    # -- case (a)
    B = 2048 if not a.quick else 16
    md = shared_model(R, B, n, ne, ni)
    full = {k: (np.broadcast_to(v, (B,) + v.shape).copy() if k in ("H", "A", "C") else v) for k, v in md.items()}
    mb = lambda d: sum(v.nbytes for v in d.values()) / 1e6
    say()
    say("(a) host buffers, B = %d: %.1f MB of model arrays materialised, %.1f MB with H, A, C shared" % (B, mb(full), mb(md)))
    handles = {}
    for name in ("init(-1), materialised", "init_shared, H A C shared"):
        handles[name] = N.Batch(B, n, ne, ni, lib=lib)
        handles[name].set_all_settings(eps_abs=1e-9, eps_rel=0.0)
    t_init, t_all = {k: [] for k in handles}, {k: [] for k in handles}
    for rep in range(a.repeats + 1):
        for name, b in handles.items():
            t0 = time.perf_counter()
            if name.startswith("init_shared"):
                b.init_shared(0, B, shared=("H", "A", "C"), **md)
            else:
                b.init(-1, **full)
            b.flush()
            t1 = time.perf_counter()
            b.solve()
            res = b.results()
            t2 = time.perf_counter()
            if rep:
                t_init[name].append(1e3 * (t1 - t0))
                t_all[name].append(1e3 * (t2 - t0))
            assert all(res[5][i].status == 0 for i in range(B)), name
    for name in handles:
        say("%-28s | init + flush %s ms | init + flush + solve + results %s ms = %8.0f QPs/s inclusive"
            % (name, fmt(t_init[name]), fmt(t_all[name]), B / (1e-3 * statistics.median(t_all[name]))))
    ra, rb = (h.results() for h in handles.values())
    say("    x, y, z of the two handles bit-identical: %s" % all(np.array_equal(p, q) for p, q in zip(ra[:3], rb[:3])))
    for b in handles.values():
        b.close()

    # -- case (b)
    say()
    say("(b) ROCm tensors: QPFunction forward + backward, Q, A, G shared, p, b, l, u batched")
    f = qplayer.QPFunction(eps=1e-9, maxIter=1000)
    contenders = ["shared", "expanded"] + (["expanded, other library"] if other else [])
    pools = {c: {} for c in contenders}  # (the layer's cache of handles, one per contender: a handle belongs to its library)
    for B in ((256, 2048) if not a.quick else (8,)):
        md = shared_model(R, B, n, ne, ni, seed=1)
        names = ("H", "g", "A", "b", "C", "l", "u")
        w = torch.as_tensor(np.random.default_rng(2).standard_normal((B, n)), device="cuda")
        times, grads = {c: [] for c in contenders}, {}
        for rep in range(a.repeats + 1):
            for c in contenders:
                N._lib = other if c.endswith("other library") else lib
                qplayer._FREE = pools[c]
                params = {k: torch.tensor(md[k], dtype=torch.float64, device="cuda", requires_grad=True) for k in names}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                args = [params[k] if c == "shared" or k not in ("H", "A", "C") else params[k].unsqueeze(0).expand(B, *params[k].shape)
                        for k in names]
                out = f(*args)
                (w * out[0]).sum().backward()
                torch.cuda.synchronize()
                if rep:
                    times[c].append(1e3 * (time.perf_counter() - t0))
                grads[c] = params["H"].grad.detach().cpu().numpy()
                del out, args, params  # (the handle goes back to THIS contender's pool: before the next one's is installed)
        N._lib = lib
        for c in contenders:
            say("B %4d | %-24s %s ms" % (B, c, fmt(times[c])))
        for c in contenders[1:]:
            ref = grads[c]
            say("    dL/dQ, shared against %s: max |difference| %.3e (max |entry| %.3e)"
                % (c, float(np.max(np.abs(grads["shared"] - ref))), float(np.max(np.abs(ref)))))
    say("# box after:  %s" % N.box_calibration())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""One pqp_batch_backward_multi call with K loss derivatives per QP against K calls of pqp_batch_backward_range on the same
solved batch.  Stand-alone: bench.py and its flagship workload are not involved.

    python scripts/backward_multi_bench.py [--out profiles/backward_multi.txt] [--repeats 5] [--quick] [--single-only] [--lib PATH]

Shape (100, 50, 100) (BASELINE.json configs[1] / [2]), B in {1, 256, 2048}, K in {1, 8, 100}; forward eps_abs = 1e-9,
backward (eps, rho, mu) = (1e-5, 1e-7, 1e-7).  Loss derivatives and outputs are ROCm tensors (no staging copy in either
path); both entries are synchronous, so a figure is the host wall time of the call(s): median [min .. max] of `--repeats`
rounds, the two paths alternating, one forward solve in front of every timed backward (outside the timed region: a backward
pass leaves the QP to be solved again).  The K single calls are timed without the read-back of their seven jacobians
(pqp_batch_get_backward), i.e. in their favour.  --single-only times the K single calls alone: that path is the parent
commit's, so the same command on a parent build says whether the two builds agree on it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BW = (1e-5, 1e-7, 1e-7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backward_multi.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libproxqp_hip.so (with --single-only: the parent commit's)")
    a = ap.parse_args()

    import torch
    from proxsuite_amd import _native as N
    from proxsuite_amd.utils import random_qp as R
    lib = N.load()  # (fails loudly without the library or a device: no fall-back, no number)
    if a.lib:
        lib = N.NativeLib(a.lib, legacy=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, ne, ni = (100, 50, 100) if not a.quick else (10, 4, 7)
    ntot = n + ne + ni
    batches, rows = ((1, 256, 2048), (1, 8, 100)) if not a.quick else ((1, 8), (1, 3))
    say("# library: %s" % lib.path)
    say("# scripts/backward_multi_bench.py: shape (%d, %d, %d), %d rounds per figure, median [min .. max], host wall ms; device %s"
        % (n, ne, ni, a.repeats, torch.cuda.get_device_name(0)))
    say("# box before: %s" % N.box_calibration())
    for B in batches:
        m = R.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)
        b = N.Batch(B, n, ne, ni, lib=lib)
        b.set_all_settings(eps_abs=1e-9, eps_rel=0.0)
        b.init(-1, m.H, m.g, m.A, m.b, m.C, m.l, m.u)
        for K in rows:
            rng = np.random.default_rng(K)
            ld = torch.as_tensor(rng.standard_normal((B, K, ntot)), device="cuda")
            single_rows = [ld[:, k].contiguous() for k in range(K)]
            V = torch.zeros_like(ld)
            act = torch.zeros((B, ni), dtype=torch.int32, device="cuda")
            t_multi, t_single = [], []
            for rep in range(a.repeats + 1):  # (round 0 is the warm-up)
                if not a.single_only:
                    b.solve()
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    b.backward_multi(ld, *BW, into=(V, act))
                    t_multi.append(1e3 * (time.perf_counter() - t))
                spent = 0.0
                for k in range(K):
                    b.solve()
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    b.backward(single_rows[k], *BW, first=0, count=B)
                    spent += 1e3 * (time.perf_counter() - t)
                t_single.append(spent)
            fmt = lambda v: "%10.3f [%10.3f .. %10.3f]" % (statistics.median(v[1:]), min(v[1:]), max(v[1:]))
            if a.single_only:
                say("B %4d K %3d | %d single calls %s" % (B, K, K, fmt(t_single)))
            else:
                say("B %4d K %3d | backward_multi %s | %d single calls %s | ratio %.2f"
                    % (B, K, fmt(t_multi), K, fmt(t_single), statistics.median(t_single[1:]) / statistics.median(t_multi[1:])))
        b.close()
    say("# box after:  %s" % N.box_calibration())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

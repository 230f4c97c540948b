#!/usr/bin/env python
"""One pqp_batch_tangent_multi call with K directions per QP against the only route without it: pqp_batch_backward_multi with
n + n_eq + n_in identity rows (the full Jacobian of (x, y, z)) followed by the contraction with the right-hand sides.
Stand-alone: bench.py and its flagship workload are not involved.

    python scripts/tangent_bench.py [--out profiles/tangent_multi.txt] [--repeats 5] [--quick]

Shape (100, 50, 100), B in {1, 256, 2048}, K in {1, 8}; forward eps_abs = 1e-9, backward (eps, rho, mu) = (1e-5, 1e-7,
1e-7).  Two runs per (B, K): all seven tangents, and the vector tangents alone (no matrix is read).  Tangents and outputs
are ROCm tensors (no staging copy in either path); both entries are synchronous, so a figure is the host wall time: median
[min .. max] of `--repeats` rounds, the two paths alternating, one forward solve in front of every timed call (outside the
timed region).  The Jacobian route is timed in its favour: its right-hand sides (r_x | r_y | r_z) and its contraction are
torch einsums on the device, and its z rows -- which backward_multi's repeated scaling gets wrong under equilibration
 -- are not checked."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BW = (1e-5, 1e-7, 1e-7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_multi.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()

    import torch
    from proxsuite_amd import _native as N
    from proxsuite_amd.utils import random_qp as R
    lib = N.load()  # (fails loudly without the library or a device: no fall-back, no number)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, ne, ni = (100, 50, 100) if not a.quick else (10, 4, 7)
    ntot = n + ne + ni
    batches, dirs = ((1, 256, 2048), (1, 8)) if not a.quick else ((1, 8), (1, 3))
    tails = dict(H=(n, n), g=(n,), A=(ne, n), b=(ne,), C=(ni, n), l=(ni,), u=(ni,))
    say("# library: %s" % lib.path)
    say("# scripts/tangent_bench.py: shape (%d, %d, %d), %d rounds per figure, median [min .. max], host wall ms; device %s"
        % (n, ne, ni, a.repeats, torch.cuda.get_device_name(0)))
    say("# box before: %s" % N.box_calibration())
    opts = dict(dtype=torch.float64, device="cuda")
    for B in batches:
        m = R.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)
        b = N.Batch(B, n, ne, ni, lib=lib)
        b.set_all_settings(eps_abs=1e-9, eps_rel=0.0)
        b.init(-1, m.H, m.g, m.A, m.b, m.C, m.l, m.u)
        eye = torch.eye(ntot, **opts).expand(B, ntot, ntot).contiguous()
        J, jact = torch.zeros_like(eye), torch.zeros((B, ni), dtype=torch.int32, device="cuda")
        x, y, z = (torch.empty((B, k), **opts) for k in (n, ne, ni))
        for K in dirs:
            gen = torch.Generator(device="cuda").manual_seed(K)
            full = {k: torch.randn((B, K) + v, generator=gen, **opts) for k, v in tails.items()}
            T, act = torch.zeros((B, K, ntot), **opts), torch.zeros((B, ni), dtype=torch.int32, device="cuda")
            for what, names in (("all seven", "HgAbClu"), ("vectors", "gblu")):
                t = {"d" + k: v for k, v in full.items() if k in names}
                mat = "H" in names
                t_new, t_old = [], []
                for rep in range(a.repeats + 1):  # (round 0 is the warm-up)
                    b.solve()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    b.tangent_multi(*BW, into=(T, act), **t)
                    t_new.append(1e3 * (time.perf_counter() - t0))
                    b.solve()
                    b.results_into(x, y, z)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    b.backward_multi(eye, *BW, into=(J, jact))
                    rx = t["dg"].clone()
                    ry, rz = -t["db"], torch.zeros((B, K, ni), **opts)
                    if mat:
                        rx += 0.5 * (torch.einsum("bkij,bj->bki", t["dH"], x) + torch.einsum("bkij,bi->bkj", t["dH"], x))
                        rx += torch.einsum("bkij,bi->bkj", t["dA"], y) + torch.einsum("bkij,bi->bkj", t["dC"], z)
                        ry = ry + torch.einsum("bkij,bj->bki", t["dA"], x)
                        rz = rz + torch.einsum("bkij,bj->bki", t["dC"], x)
                    up, low = ((jact & 1) != 0)[:, None, :], ((jact & 2) != 0)[:, None, :]
                    rz = torch.where((jact != 0)[:, None, :], rz - up * t["du"] - low * t["dl"], torch.zeros((), **opts))
                    old = torch.einsum("bij,bkj->bki", J, torch.cat([rx, ry, rz], dim=2))
                    torch.cuda.synchronize()
                    t_old.append(1e3 * (time.perf_counter() - t0))
                err = float((old[:, :, :n + ne] - T[:, :, :n + ne]).abs().max() / (1 + T[:, :, :n + ne].abs().max()))
                fmt = lambda v: "%10.3f [%10.3f .. %10.3f]" % (statistics.median(v[1:]), min(v[1:]), max(v[1:]))
                say("B %4d K %2d %-9s | tangent_multi %s | backward_multi(%d rows) + contraction %s | ratio %.2f | x, y rows agree to %.1e"
                    % (B, K, what, fmt(t_new), ntot, fmt(t_old), statistics.median(t_old[1:]) / statistics.median(t_new[1:]), err))
            del full
        b.close()
    say("# box after:  %s" % N.box_calibration())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

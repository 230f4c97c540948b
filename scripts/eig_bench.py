#!/usr/bin/env python
"""Batched minimal-eigenvalue estimates on the device (pqp_estimate_min_eigenvalues, csrc/pqp_eig.hpp) against the host
helper looped over the same matrices.  Stand-alone: bench.py and its flagship workload are not involved.

    python scripts/eig_bench.py [--out profiles/eig_batch.txt] [--repeats 7] [--quick]

Per shape (B matrices of order n, random symmetric indefinite (M + M^T) / 2, seeded) and method:
  * device: the matrices already on the device (a ROCm tensor, read in place), events of the launch stream around
    the call -- the kernel plus the read-back of B results; warm-up launches first, then the median and the spread
    of `--repeats` launches.  The same from a host array (one staging copy of B n^2 doubles in front) as a host wall time.
  * host: dense.estimate_minimal_eigen_value_of_symmetric_matrix called matrix by matrix on the host of the same machine,
    timed on the first `sample` matrices and scaled to B (the sample size is printed).
PowerIteration runs at its defaults (accuracy 1e-3, 1000 iterations).  At order 100 the LDS-resident and the streamed
form of the power iteration (PQP_EIG_RESIDENT=1 / 0) are timed alternately.  The box state (pqp_box_calibrate) is
recorded before and after."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def matrices(B, n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((B, n, n))
    return (M + M.transpose(0, 2, 1)) / 2


def device_ms(N, torch, Hd, method, repeats, warmup=2):
    """event span of one call per launch, milliseconds: (median, min, max), and the values of the last launch"""
    out = None
    for _ in range(warmup):
        out = N.estimate_min_eigenvalues(Hd, method)
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = N.estimate_min_eigenvalues(Hd, method)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), out.cpu().numpy()


def host_call_ms(N, H, method, repeats):
    """host wall time of the call on a HOST array (staging copy + kernel + read-back), milliseconds: median"""
    N.estimate_min_eigenvalues(H, method)
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        N.estimate_min_eigenvalues(H, method)
        ms.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ms)


def host_helper_ms(dense, H, method, sample):
    sample = min(sample, len(H))
    dense.estimate_minimal_eigen_value_of_symmetric_matrix(H[0], method)
    t = time.perf_counter()
    vals = [dense.estimate_minimal_eigen_value_of_symmetric_matrix(H[i], method) for i in range(sample)]
    per = 1e3 * (time.perf_counter() - t) / sample
    return per, sample, np.array(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_batch.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()

    import torch
    from proxsuite_amd import _native as N
    from proxsuite_amd.proxqp import dense
    Opt = dense.EigenValueEstimateMethodOption
    N.load()  # (fails loudly without the library or a device: no fall-back, no number)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    shapes = [(2048, 100, 64, 16), (2048, 50, 128, 32), (512, 512, 4, 2)]  # B, n, host sample exact, host sample power
    if a.quick:
        shapes = [(32, 20, 4, 4)]
    say("# scripts/eig_bench.py: %d repeats per figure, median [min .. max]; device %s" % (a.repeats, torch.cuda.get_device_name(0)))
    say("# box before: %s" % N.box_calibration())
    for B, n, s_exact, s_power in shapes:
        H = matrices(B, n, seed=n)
        Hd = torch.as_tensor(H, device="cuda")
        for method, sample in ((Opt.ExactMethod, s_exact), (Opt.PowerIteration, s_power)):
            med, lo, hi, vals = device_ms(N, torch, Hd, method, a.repeats)
            staged = host_call_ms(N, H, method, max(3, a.repeats // 2))
            per, used, hvals = host_helper_ms(dense, H, method, sample)
            dev = np.max(np.abs(vals[:used] - hvals))
            say("%4d x order %3d  %-14s device %9.3f ms [%9.3f .. %9.3f] per launch | from a host array %9.3f ms (wall) | "
                "host helper %9.3f ms per matrix on %d matrices = %10.1f ms per %d | max |device - host| on them %.3g"
                % (B, n, method.name, med, lo, hi, staged, per, used, per * B, B, dev))
        if n == 100 or a.quick:
            # LDS-resident against streamed H in the power iteration, alternating
            res = {"1": [], "0": []}
            for _ in range(3):
                for flag in ("1", "0"):
                    os.environ["PQP_EIG_RESIDENT"] = flag
                    res[flag].append(device_ms(N, torch, Hd, Opt.PowerIteration, max(3, a.repeats // 2), warmup=1)[0])
            os.environ.pop("PQP_EIG_RESIDENT")
            say("%4d x order %3d  PowerIteration  H in LDS %s ms | H streamed from HBM %s ms (medians of alternating rounds)"
                % (B, n, ["%.3f" % v for v in res["1"]], ["%.3f" % v for v in res["0"]]))
        del Hd
    say("# box after:  %s" % N.box_calibration())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

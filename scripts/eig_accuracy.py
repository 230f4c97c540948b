#!/usr/bin/env python
"""Worst error of the device's ExactMethod per order, in units of n u ||H||_2 (the gate of tests/eig_cases.py is 8), over
the kinds of matrix of that file; and of the converged PowerIteration in units of sqrt(n) accuracy (gate 2).

    python scripts/eig_accuracy.py [--out profiles/eig_accuracy.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_accuracy.txt"))
    a = ap.parse_args()
    import eig_cases as ec
    from proxsuite_amd import _native as N
    lib = N.load()
    lines = ["# scripts/eig_accuracy.py on %s" % lib.path.replace(ROOT + os.sep, ""),
             "# ExactMethod: worst |device - truth| / (n u ||H||_2) per order (gate 8), kinds: " + ", ".join(ec.KINDS)]
    for n in ec.EXACT_ORDERS + (ec.EXACT_ORDER_GPU_ONLY,):
        cases = [ec.exact_kind(k, n) for k in ec.KINDS]
        got = N.estimate_min_eigenvalues(np.stack([H for H, _ in cases]), ec.Opt.ExactMethod, lib=lib)
        ratios = [abs(g - t) / (ec.exact_gate(H) / 8) if ec.exact_gate(H) > 0 else abs(g - t) for g, (H, t) in zip(got, cases)]
        lines.append("order %4d  worst %.3f  (%s)" % (n, max(ratios), " ".join("%.3f" % r for r in ratios)))
    cases = ec.mixed_70()
    got = N.estimate_min_eigenvalues(np.stack([H for H, _ in cases]), ec.Opt.ExactMethod, lib=lib)
    lines.append("70 mixed matrices of order 65  worst %.3f" % max(
        abs(g - t) / (ec.exact_gate(H) / 8) if ec.exact_gate(H) > 0 else abs(g - t) for g, (H, t) in zip(got, cases)))
    lines.append("# PowerIteration, converged: worst |device - lambda_min| / (sqrt(n) accuracy) per order (gate 2)")
    for accuracy, nb in ec.POWER_SETTINGS:
        for n in ec.POWER_ORDERS:
            cases = ec.power_pair(n)
            got = N.estimate_min_eigenvalues(np.stack([H for H, _ in cases]), ec.Opt.PowerIteration, accuracy, nb, lib=lib)
            lines.append("accuracy %g order %4d  worst %.3g" % (accuracy, n, max(
                abs(g - t) / (np.sqrt(n) * accuracy) for g, (_, t) in zip(got, cases))))
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

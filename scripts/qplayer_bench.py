"""QPLayer forward + backward throughput on MI355X at the C2 shape (2048 QPs, n=100, n_eq=50,
n_in=100): proxsuite_amd.torch.QPFunction on ROCm tensors, loss = sum(x).

--infeas [OUT]: forward + backward of the closest-feasible layer (structural_feasibility=False; 100 double-sided rows, so
the single-sided QP has 200 and the inner QP of its backward is 750 x 600) beside the feasible
layer's on the same run, B in {1, 256, 2048}; the lines also go to OUT (default profiles/infeas_backward.txt)."""
import sys, time
import numpy as np
import torch
sys.path.insert(0, ".")
from proxsuite_amd.torch import QPFunction
from proxsuite_amd.utils import random_qp as R

n, ne, ni = 100, 50, 100
dev = "cuda"
t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)


def run(B, feasible, reps, emit):
    m = R.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)
    Q, p, A, b, G, u = t(m.H), t(m.g).requires_grad_(True), t(m.A), t(m.b), t(m.C), t(m.u)
    l = torch.full_like(u, -1e20) if feasible else t(m.l)
    f = QPFunction(eps=1e-9, maxIter=1000, structural_feasibility=feasible)
    for rep in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x = f(Q, p, A, b, G, l, u)[0]
        torch.cuda.synchronize(); t1 = time.perf_counter()
        x.sum().backward()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        emit("%s B %4d rep %d: forward %.2f ms (%.0f QPs/s incl. batch create + init + Ruiz), backward %.2f ms (%.0f QPs/s)"
             % ("feasible        " if feasible else "closest-feasible", B, rep, 1e3 * (t1 - t0), B / (t1 - t0), 1e3 * (t2 - t1),
                B / (t2 - t1)))
        p.grad = None


if "--infeas" in sys.argv:
    i = sys.argv.index("--infeas")
    out = open(sys.argv[i + 1] if len(sys.argv) > i + 1 else "profiles/infeas_backward.txt", "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit("# scripts/qplayer_bench.py --infeas: QPFunction forward + backward at (n, n_eq, n_in) = (%d, %d, %d), fp64, %s"
         % (n, ne, ni, torch.cuda.get_device_name(0)))
    for B in (1, 256, 2048):
        run(B, True, 2, emit)
        run(B, False, 2, emit)
else:
    run(2048, True, 3, lambda s: print(s, flush=True))

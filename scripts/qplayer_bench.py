"""QPLayer forward + backward throughput on MI355X at the C2 shape (2048 QPs, n=100, n_eq=50,
n_in=100): proxsuite_amd.torch.QPFunction on ROCm tensors, loss = sum(x).

--infeas [OUT]: forward + backward of the closest-feasible layer (structural_feasibility=False; 100 double-sided rows, so
the single-sided QP has 200 and the inner QP of its backward is 750 x 600) beside the feasible
layer's on the same run, B in {1, 256, 2048}; the lines also go to OUT (default profiles/infeas_backward.txt).

--box [OUT] [--commit ID]: forward + backward of 2048 QPs at that shape with n variable bounds, in two forms: (a)
QPFunctionBox (the bounds as box constraints of the engine) and (b) QPFunction with the bounds stacked under G as n
identity rows.  3 warm-up and 20 timed repetitions each, interleaved; medians, the ratio (a) / (b), the kernels that ran
and the box calibration line go to OUT (default profiles/backward_box.txt)."""
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


def run_box(out_path, commit):
    from proxsuite_amd import _native
    from proxsuite_amd.torch import QPFunctionBox
    B, warm, reps = 2048, 3, 20
    m = R.dense_strongly_convex_qp_batch(B, n, ne, ni, 0.15, 1e-2)
    Q, A, b, G, l, u = t(m.H), t(m.A), t(m.b), t(m.C), t(m.l), t(m.u)
    # bounds around the solution of the QP without them: a quarter of the variables pushed down, a quarter pushed up
    x0 = QPFunction(eps=1e-9, maxIter=1000)(Q, t(m.g), A, b, G, l, u)[0]
    kind = torch.arange(n, device=dev) % 4
    ub = torch.where(kind == 0, x0 - 0.1, x0 + 1.0).contiguous()
    lb = torch.where(kind == 1, x0 + 0.1, x0 - 1.0).contiguous()
    eye = torch.eye(n, dtype=torch.float64, device=dev).expand(B, n, n)
    G2, l2, u2 = torch.cat((G, eye), dim=1).contiguous(), torch.cat((l, lb), dim=1), torch.cat((u, ub), dim=1)
    fa, fb = QPFunctionBox(eps=1e-9, maxIter=1000), QPFunction(eps=1e-9, maxIter=1000)
    times = {"a": ([], []), "b": ([], [])}
    kernels, grads = {}, {}
    for rep in range(warm + reps):
        for form in ("a", "b"):
            p = t(m.g).requires_grad_(True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            x = fa(Q, p, A, b, G, l, u, lb, ub)[0] if form == "a" else fb(Q, p, A, b, G2, l2, u2)[0]
            torch.cuda.synchronize(); t1 = time.perf_counter()
            kernels[form] = x.grad_fn.batch.last_kernel
            x.sum().backward()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            grads[form] = p.grad
            if rep >= warm:
                times[form][0].append(1e3 * (t1 - t0))
                times[form][1].append(1e3 * (t2 - t1))
    med = {k: (float(np.median(v[0])), float(np.median(v[1]))) for k, v in times.items()}
    spread = {k: (min(v[0]), max(v[0]), min(v[1]), max(v[1])) for k, v in times.items()}
    diff = float((grads["a"] - grads["b"]).abs().max())
    lines = ["# scripts/qplayer_bench.py --box: forward + backward of %d QPs at (n, n_eq, n_in) = (%d, %d, %d) with n variable bounds,"
             % (B, n, ne, ni),
             "# fp64, loss = sum(x), %d warm-up + %d timed repetitions per form, interleaved; host wall clock around synchronised calls"
             % (warm, reps),
             "# (a forward includes checking out the handle, init with Ruiz and the solve; a backward the launch and the copies)",
             "commit: %s" % commit, "device: %s" % torch.cuda.get_device_name(0),
             "box calibration: %s" % (_native.box_calibration(),),
             "(a) QPFunctionBox            : forward %.3f ms (min %.3f, max %.3f)  backward %.3f ms (min %.3f, max %.3f)  solve kernel %s"
             % (med["a"][0], spread["a"][0], spread["a"][1], med["a"][1], spread["a"][2], spread["a"][3], kernels["a"]),
             "(b) QPFunction, bounds as rows: forward %.3f ms (min %.3f, max %.3f)  backward %.3f ms (min %.3f, max %.3f)  solve kernel %s"
             % (med["b"][0], spread["b"][0], spread["b"][1], med["b"][1], spread["b"][2], spread["b"][3], kernels["b"]),
             "backward kernels: (a) pqp_bwbox_kernel<256> + pqp_bwbox_outer_kernel<256>, %d constraint rows of which %d are dense rows"
             " of G; (b) pqp_backward_kernel<256>, %d dense rows" % (ni + n, ni, ni + n),
             "ratio (a) / (b): forward %.3f  backward %.3f  forward + backward %.3f"
             % (med["a"][0] / med["b"][0], med["a"][1] / med["b"][1], sum(med["a"]) / sum(med["b"])),
             "max |dL/dp (a) - dL/dp (b)|: %.3e" % diff,
             "(a) is %s than (b) forward + backward" % ("FASTER" if sum(med["a"]) < sum(med["b"]) else "NOT faster")]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if "--box" in sys.argv:
    i = sys.argv.index("--box")
    nxt = sys.argv[i + 1] if len(sys.argv) > i + 1 and not sys.argv[i + 1].startswith("--") else "profiles/backward_box.txt"
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    run_box(nxt, commit)
elif "--infeas" in sys.argv:
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

"""In-tree native builds (no JIT cache: the .so files travel with the repo snapshot).

* ``libproxqp_hip.so``  -- the product: HIP kernels (gfx950) + the C-ABI, built with hipcc.
* ``libpqp_randqp.so``  -- host-only synthetic QP generator (g++).

The CPU oracle (``oracle/liboracle.so``) and the kernel-logic emulator
(``tests/emu/libpqp_emu.so``) are test infrastructure; they are built by
``__graft_entry__.build()`` / the test fixtures, never loaded from this package.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "proxsuite_amd" / "csrc"
INCLUDE = ROOT / "include"

HIP_LIB = CSRC / "libproxqp_hip.so"
# the same library with the per-phase device timers and event counters compiled in (-DPQP_STATS):
# used by bench.py OUTSIDE its timed region and by the profiling scripts, never by the product path
HIP_STATS_LIB = CSRC / "libproxqp_hip_stats.so"
RANDQP_LIB = CSRC / "libpqp_randqp.so"

HOST_CXXFLAGS = ["-O3", "-march=x86-64-v3", "-mtune=generic", "-std=gnu++17", "-fPIC", "-fopenmp"]


def _newer(target: Path, sources) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(Path(s).stat().st_mtime <= t for s in sources)


def _run(cmd, cwd=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: %s\n%s\n%s" % (" ".join(map(str, cmd)), r.stdout, r.stderr))
    return r


def build_randqp(force: bool = False) -> Path:
    src = [CSRC / "random_qp.cpp"]
    if not force and _newer(RANDQP_LIB, src):
        return RANDQP_LIB
    _run(["g++", *HOST_CXXFLAGS, "-shared", "-o", str(RANDQP_LIB), *map(str, src)])
    return RANDQP_LIB


# pqp_kernels.hip is compiled once per kernel family (see its header): every solve kernel is
# ~350 KB of inlined code and takes about a minute of hipcc time, so the objects are built in
# parallel and linked into one shared library.
KERNEL_TUS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27)
# families outside the solver (19: the eigenvalue estimates of pqp_eig.hpp): built and linked like the others, their
# resources frozen in a record of their own (tests/golden/eig_kernel_resources_expected.json) -- the solver's frozen record
# names the solver's kernels and no others
AUXILIARY_TUS = (19,)
# ... and further groups of that kind, each with a frozen record of its own and selected by name
# (kernel_resources(auxiliary="backward_multi")): 20 / 21, the backward pass for K loss derivatives per QP, in LDS and on
# an HBM slice (tests/golden/backward_multi_kernel_resources_expected.json)
# 22, the closest-feasible QPLayer's backward pass: the assembly of its linear systems and its jacobians (csrc/pqp_infeas.hpp,
# tests/golden/infeas_backward_kernel_resources_expected.json)
# 23 / 24, the backward pass of QPs with box constraints, in LDS and on an HBM slice, and the kernel that forms its nine
# jacobians (tests/golden/bwbox_kernel_resources_expected.json, written by --freeze under the name below)
# 25, batches that share a model: the broadcast of one model array to the QPs of a range and the ordered sum of a per-QP
# array (csrc/pqp_shared.hpp, tests/golden/shared_model_kernel_resources_expected.json)
# 26 / 27, forward-mode sensitivities: the K-tangent solve in LDS and on an HBM slice, and the assembly of its right-hand
# sides from the parameter tangents (csrc/pqp_tangent.hpp, tests/golden/tangent_kernel_resources_expected.json)
NAMED_TUS = {"backward_multi": (20, 21), "infeas_backward": (22,), "backward_box": (23, 24), "shared_model": (25,),
             "tangent": (26, 27)}
# (the frozen record of a group is <RECORD_NAMES.get(group, group)>_kernel_resources_expected.json)
RECORD_NAMES = {"backward_box": "bwbox"}
OBJ_DIR = ROOT / "build" / "obj"


def hip_sources():
    return [CSRC / "pqp_capi.hip", CSRC / "pqp_multi.hip", CSRC / "pqp_kernels.hip", CSRC / "pqp_calib.hip"]


def hip_headers():
    return sorted(CSRC.glob("*.hpp")) + sorted(INCLUDE.glob("*.h"))


# Register allocation of the one-kernel solver is the lever: sinking
# instructions into the loops that use them and NOT hoisting loop invariants out of them cuts the
# VGPR spills of the C2 kernel from 517 to 163 (+9 % QPs/s, profiles/r02_ab_compiler_flags.txt); without
# loop strength reduction the mat-vec loops recompute their addresses from one index instead of
# carrying a pointer per load in flight (128-VGPR kernel: 319 -> 206 spilled VGPRs, +4.5 % QPs/s).
CODEGEN_FLAGS = ["-mllvm", "-sink-insts-to-avoid-spills", "-mllvm", "-disable-machine-licm"]
# per translation unit (kernel family, csrc/pqp_kernels.hip): measured on the workload each one serves --
# C2 +4.3 %, C1 +3.4 %, C4 +2 % with -disable-lsr; the structured / boxed 256-thread kernel (C5: -17 %) and the
# 512-thread kernels (dense-backend shape: -7 %) keep loop strength reduction
TU_FLAGS = {17: ["-mllvm", "-disable-lsr"],  # the one-wavefront dense kernel: 7.65 -> 7.37 ms per 2048 C2 QPs (profiles/r06_ab_dwave.txt section 13)
            18: ["-mllvm", "-disable-lsr", "-DPQP_ZG_DEPTH=4"],  # the prologue kernel: 4 k-steps of operand loads in flight per lane in its Z / G build (8 elsewhere): 1.026 -> 0.985 ms per 2048 C2 QPs; 2 / 3 / 5 / 6 / 12: 1.000 / 1.003 / 0.986 / 1.020 / 1.467 ms
            1: ["-mllvm", "-disable-lsr"], 4: ["-mllvm", "-disable-lsr"], 7: ["-mllvm", "-disable-lsr"], 13: ["-mllvm", "-disable-lsr"], 15: ["-mllvm", "-disable-lsr"]}


def hip_flags(extra_flags=()):
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", *CODEGEN_FLAGS,
            "-Rpass-analysis=kernel-resource-usage",  # per-kernel registers / spills / scratch, parsed below
            "-I", str(INCLUDE), "-I", str(CSRC), *extra_flags]


def parse_kernel_resources(stderr: str) -> dict:
    """The AMDGPU backend's kernel-resource-usage remarks -> {demangled-ish kernel name: {field: value}}.
    The register allocation of the one-kernel solver decides its speed, and three
    internal -mllvm switches shape it: every build records what it got (build/kernel_resources.json,
    copied to profiles/ by __graft_entry__.build) so that a toolchain change cannot shift it silently."""
    import re
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?:\[[^\]]*\])?):\s*(\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            key = re.sub(r"\s*\[.*\]", "", key).strip().replace(" ", "_")
            try:
                cur[key] = int(val)
            except ValueError:
                cur[key] = val
    return out


def kernel_label(mangled: str) -> str:
    """_Z16pqp_solve_kernelILi256ELi4ELi1EEv... -> pqp_solve_kernel<256,4,1>"""
    import re
    m = re.match(r"_Z\d+([A-Za-z_0-9]+?)I((?:Li\d+E)+)E", mangled)
    if not m:
        return mangled
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"Li(\d+)E", m.group(2))))


def flags_tag(extra_flags) -> str:
    """stable name of a flag set (object directory / object suffix of a variant build)"""
    import hashlib
    return "v" + hashlib.sha1(" ".join(extra_flags).encode()).hexdigest()[:8]


def hipcc() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


HOST_OBJECTS = {"capi.o": "pqp_capi.hip", "multi.o": "pqp_multi.hip", "calib.o": "pqp_calib.hip"}


def hip_objects(odir: Path, tus=KERNEL_TUS):
    """the objects libproxqp_hip.so is linked from: the host translation units and one per kernel family"""
    return [odir / o for o in HOST_OBJECTS] + [odir / ("kernels_%d.o" % k) for k in tus]


def compile_tu(k: int, obj: Path, extra_flags=()):
    """kernel family `k` of pqp_kernels.hip -> `obj`; returns the finished process (stderr: the resource remarks)"""
    return _run([hipcc(), *hip_flags(extra_flags), *TU_FLAGS.get(k, []), "-DPQP_TU=%d" % k, "-c",
                 str(CSRC / "pqp_kernels.hip"), "-o", str(obj)])


def link_hip(lib: Path, odir: Path = None, replaced=None, tus=KERNEL_TUS) -> Path:
    """`lib` <- the objects of the build in `odir` (default: the product's), those named in `replaced`
    ({object name: another object}) swapped: how a variant that differs in one kernel family is made in seconds"""
    odir, replaced = odir or OBJ_DIR / "default", replaced or {}
    Path(lib).parent.mkdir(parents=True, exist_ok=True)
    _run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(lib),
          *[str(replaced.get(o.name, o)) for o in hip_objects(odir, tus)]])
    return Path(lib)


def build_hip(force: bool = False, extra_flags=(), out: Path = None, tus=KERNEL_TUS) -> Path:
    """Cross-compiles for gfx950 (works without a GPU).  `out` / `extra_flags` build a variant
    of the library somewhere else (A/B runs: scripts/gpu_ab.sh); `tus` restricts the kernel
    families that are compiled (development only: the launchers of the others are then missing
    and the link fails unless the variant is never asked for them... so keep the default)."""
    from concurrent.futures import ThreadPoolExecutor
    lib = Path(out) if out else HIP_LIB
    deps = list(hip_sources()) + hip_headers() + [Path(__file__)]
    if not force and _newer(lib, deps):
        return lib
    tag = "default" if not extra_flags else flags_tag(extra_flags)
    odir = OBJ_DIR / tag
    odir.mkdir(parents=True, exist_ok=True)
    # an object is stale when ITS source, a header or this recipe is newer (an edit of pqp_multi.hip does not recompile
    # sixteen kernel families)
    common = hip_headers() + [Path(__file__)]
    # (pqp_dwave.hpp is parsed by every kernel family; family 17 instantiates its kernel, and family 6 compiles the host
    # side of its dispatch -- pqp_plan_solve reads dwave_signature / dwave_lds_bytes: inline templates, no code elsewhere)
    # (pqp_eig.hpp: family 19 alone includes it; pqp_capi.hip reads its host half)
    # (pqp_shared.hpp: family 25 alone includes it; pqp_capi.hip reads its constants)
    only = {"pqp_dwave.hpp": ("kernels_17.o", "kernels_6.o"), "pqp_eig.hpp": ("kernels_19.o", "capi.o"),
            "pqp_shared.hpp": ("kernels_25.o", "capi.o"),
            # (pqp_tangent.hpp: families 26 and 27 alone include it; pqp_capi.hip reads its argument records)
            "pqp_tangent.hpp": ("kernels_26.o", "kernels_27.o", "capi.o")}
    def deps_of(o):
        return [h for h in common if h.name not in only or o.name in only[h.name]] + [CSRC / HOST_OBJECTS.get(o.name, "pqp_kernels.hip")]
    def compile_object(o):
        if o.name in HOST_OBJECTS:
            return _run([hipcc(), *hip_flags(extra_flags), "-c", str(CSRC / HOST_OBJECTS[o.name]), "-o", str(o)])
        return compile_tu(int(o.stem.split("_")[1]), o, extra_flags)
    todo = [o for o in hip_objects(odir, tus) if force or not _newer(o, deps_of(o))]
    with ThreadPoolExecutor(max_workers=max(1, min(len(todo), os.cpu_count() or 1))) as ex:
        results = list(ex.map(compile_object, todo))
    link_hip(lib, odir, tus=tus)
    # registers / spills / scratch of every kernel that was (re)compiled, merged into the record of this build tag
    import json
    rec_path = odir / "kernel_resources.json"
    rec = json.loads(rec_path.read_text()) if rec_path.exists() else {}
    for o, r in zip(todo, results):
        rec = {k: v for k, v in rec.items() if v.get("object") != o.name}  # (what that object held before this compile)
        for name, fields in parse_kernel_resources(r.stderr).items():
            rec[kernel_label(name)] = dict(fields, object=o.name)
    rec_path.write_text(json.dumps(rec, indent=1, sort_keys=True))
    return lib


def kernel_resources(tag: str = "default", auxiliary=False) -> dict:
    """what the last build of `tag` recorded (see parse_kernel_resources) for the solver's kernel families, or
    (`auxiliary` True) for the families of AUXILIARY_TUS, or (`auxiliary` a name) for that group of NAMED_TUS"""
    import json
    p = OBJ_DIR / tag / "kernel_resources.json"
    rec = json.loads(p.read_text()) if p.exists() else {}
    # (the record accumulates over builds: entries of translation units that no longer exist are dropped)
    named = {k for tus in NAMED_TUS.values() for k in tus}
    if isinstance(auxiliary, str):
        live = {"kernels_%d.o" % k for k in NAMED_TUS[auxiliary]}
    else:
        live = {"kernels_%d.o" % k for k in KERNEL_TUS if k not in named and (k in AUXILIARY_TUS) == auxiliary}
    return {k: v for k, v in rec.items() if v.get("object") in live}


def build_hip_stats(force: bool = False) -> Path:
    lib = HIP_STATS_LIB
    deps = list(hip_sources()) + hip_headers() + [Path(__file__)]
    if not force and _newer(lib, deps):
        return lib
    return build_hip(extra_flags=("-DPQP_STATS",), out=lib)  # (stale objects only)


VARIANT_DIR = CSRC / "variants"


def build_hip_variants(force: bool = False):
    """A/B partners that travel with the tree.  Register-budget variants of the 512-thread latency kernel (PQP_WPS_512 = 3 and 4; the product
    uses 2), for the GPU regression test that sweeps them (tests/test_gpu_parity.py): round 1 saw
    NaNs at (512, 4) with a kernel that has since been rewritten; the sweep keeps watch.  Only the
    translation unit of that kernel is recompiled; the other objects are the product's."""
    out = []
    deps = list(hip_sources()) + hip_headers() + [Path(__file__)]
    build_hip()  # the product objects the variants link against
    for w in (3, 4):
        lib = VARIANT_DIR / ("libproxqp_hip_wps512_%d.so" % w)
        if force or not _newer(lib, deps):
            o3 = OBJ_DIR / "default" / ("kernels_3_wps%d.o" % w)
            compile_tu(3, o3, ("-DPQP_WPS_512=%d" % w,))
            link_hip(lib, replaced={"kernels_3.o": o3})
        out.append(lib)
    # the one-wavefront dense kernel with the two-pass dual Schur solve / row append everywhere (PQP_DW_SCHUR_ONE_PASS=0,
    # csrc/pqp_dwave.hpp): the A/B twin of the one-pass form, bit for bit the same results (tests/test_gpu_schur_one_pass.py)
    lib = VARIANT_DIR / "libproxqp_hip_schur2pass.so"
    if force or not _newer(lib, deps):
        import json
        _, res = build_tu_variant(17, ("-DPQP_DW_SCHUR_ONE_PASS=0",), lib)
        (OBJ_DIR / "default" / "kernel_resources_schur2pass.json").write_text(json.dumps(res, indent=1, sort_keys=True))
    out.append(lib)
    return out


def build_tu_variant(tu, extra_flags, out: Path):
    """A/B partner that differs from the product in ONE kernel family: translation unit `tu` recompiled with
    `extra_flags`, every other object taken from the product build (seconds instead of minutes).  Returns (library path,
    {kernel: resources})."""
    build_hip()
    repl, res = {}, {}
    for t in ([tu] if isinstance(tu, int) else list(tu)):
        o = OBJ_DIR / "default" / ("kernels_%d_%s.o" % (t, flags_tag(extra_flags)))
        r = compile_tu(t, o, tuple(extra_flags))
        repl["kernels_%d.o" % t] = o
        res.update({kernel_label(k): v for k, v in parse_kernel_resources(r.stderr).items()})
    return link_hip(out, replaced=repl), res


def build_oracle(force: bool = False) -> Path:
    odir = ROOT / "oracle"
    lib = odir / "liboracle.so"
    srcs = [odir / "proxqp_oracle.cpp", odir / "oracle_capi.cpp", odir / "proxqp_oracle.hpp",
            odir / "ldlt_oracle.hpp", INCLUDE / "pqp_types.h", odir / "Makefile"]
    if not force and _newer(lib, srcs):
        return lib
    if force and lib.exists():
        os.remove(lib)
    _run(["make", "-C", str(odir), "-B" if force else "-s", "liboracle.so"])
    return lib


def kernel_sources_sha(diag: bool = False, dwave: bool = False) -> str:
    """sha256 (first 16 hex digits) of the device sources a solve kernel is compiled from: what a PMC traffic figure in
    profiles/pmc_traffic.json was measured on (scripts/merge_pmc_traffic.py stamps it, bench.py compares)"""
    import hashlib
    files = ["pqp_solver.hpp", "pqp_block.hpp"] + (["pqp_diag.hpp"] if diag or dwave else []) + (["pqp_dwave.hpp"] if dwave else [])
    import re
    h = hashlib.sha256()
    for f in files:
        # the CODE: comments and blank lines do not make a measurement stale
        text = (CSRC / f).read_text()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        lines = [re.sub(r"//.*$", "", ln).rstrip() for ln in text.splitlines()]
        h.update("\n".join(ln for ln in lines if ln.strip()).encode())
    return h.hexdigest()[:16]


def freeze_kernel_resources():
    """tests/golden/kernel_resources_expected.json <- the record of the current product build (run after a kernel
    change has been measured on the GPU and accepted: tests/test_kernel_resources.py then guards it)"""
    import json
    build_hip()
    rec = kernel_resources()
    keep = ("VGPRs", "AGPRs", "VGPRs_Spill", "SGPRs_Spill", "ScratchSize", "Occupancy")
    out = {k: {f: v[f] for f in keep if f in v} for k, v in sorted(rec.items()) if k.startswith("pqp_")}
    p = ROOT / "tests" / "golden" / "kernel_resources_expected.json"
    p.write_text(json.dumps(out, indent=1, sort_keys=True))
    aux = {k: {f: v[f] for f in keep if f in v} for k, v in sorted(kernel_resources(auxiliary=True).items()) if k.startswith("pqp_")}
    (p.parent / "eig_kernel_resources_expected.json").write_text(json.dumps(aux, indent=1, sort_keys=True))
    for name in NAMED_TUS:
        grp = {k: {f: v[f] for f in keep if f in v} for k, v in sorted(kernel_resources(auxiliary=name).items()) if k.startswith("pqp_")}
        (p.parent / ("%s_kernel_resources_expected.json" % RECORD_NAMES.get(name, name))).write_text(json.dumps(grp, indent=1, sort_keys=True))
    return p


if __name__ == "__main__":
    import sys
    if "--freeze" in sys.argv:
        print(freeze_kernel_resources())

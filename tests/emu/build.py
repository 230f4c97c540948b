"""TEST INFRASTRUCTURE ONLY.

Builds tests/emu/libpqp_emu.so: the *unmodified* HIP sources of the product
(proxsuite_amd/csrc/pqp_capi.hip, pqp_kernels.hip + headers) compiled with g++ against the fiber-based
SIMT emulator (hip_emu.hpp/.cpp), exposing the same C-ABI as libproxqp_hip.so.
It exists so that kernel logic can be validated against the oracle on a box without a
GPU.  The product package never loads it (proxsuite_amd._native only ever opens
proxsuite_amd/csrc/libproxqp_hip.so).
"""
import os
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
LIB = HERE / "libpqp_emu.so"


CSRC = ROOT / "proxsuite_amd" / "csrc"


def _compile(out, flags, force=False):
    """the one g++ recipe: every product source in ONE translation-unit set against the emulator's hip_runtime.h; `out`
    is rebuilt when a source, ANY header of csrc/, include/ or the emulator, or this file is newer"""
    srcs = [CSRC / "pqp_capi.hip", CSRC / "pqp_multi.hip", CSRC / "pqp_kernels.hip", CSRC / "pqp_calib.hip", HERE / "hip_emu.cpp"]
    deps = srcs + sorted(CSRC.glob("*.hpp")) + sorted((ROOT / "include").glob("*.h")) + \
        [HERE / "hip_emu.hpp", HERE / "include" / "hip" / "hip_runtime.h", Path(__file__)]
    if not force and out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    tmp = str(out) + ".tmp%d" % os.getpid()
    cmd = ["g++", "-std=gnu++17", "-fPIC", "-shared", *flags, "-pthread", "-fno-strict-aliasing", "-DPQP_STATS",
           "-Wno-unknown-pragmas", "-Wno-attributes",
           "-I", str(HERE / "include"), "-I", str(ROOT / "include"), "-I", str(CSRC),
           "-x", "c++", *map(str, srcs), "-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("emulator build of %s failed:\n" % out.name + r.stdout + r.stderr)
    os.replace(tmp, out)  # (atomic: parallel test workers may build at the same time)
    return out


def build_variant(tag, defines):
    """A second emulator library with extra -D switches (A/B of a code path on the CPU: tests/test_emu_parity.py)."""
    return _compile(HERE / ("libpqp_emu_%s.so" % tag), ["-O2", *["-D" + d for d in defines]])


def build(force=False, debug=False):
    # PQP_EMU_LIBRARY=<path>: the emulator tests load that build of the emulator library instead (scripts/dev/emu_asan.sh: the
    # AddressSanitizer build, with LD_PRELOAD=libasan.so in front of python)
    if os.environ.get("PQP_EMU_LIBRARY"):
        return Path(os.environ["PQP_EMU_LIBRARY"])
    return _compile(LIB, ["-O0", "-g"] if debug else ["-O2"], force)


if __name__ == "__main__":
    print(build(force=True, debug="--debug" in sys.argv))

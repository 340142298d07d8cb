"""Build libsc_amd.so (hipcc, gfx950) in-tree.  Used by __graft_entry__.build() and by hand.

The library is seventeen translation units: the host side in four of them, none with device code (csrc/sc_lib.hip and HOST_UNITS below:
families, schemes, top-m network; what they share is declared in csrc/sc_host.h, their set-up-time integers are the HIP-free
csrc/sc_bigint.h), the instances of the two interpreter
kernels in three parts each (csrc/sc_launch_vm.hip / sc_launch_pvm.hip with -DSC_PART=0/1/2, each part expanding its rows of the
instance list in csrc/sc_route.h and exporting one look-up of them) and the remaining kernels
(csrc/sc_launch_misc.hip with csrc/sc_kernel_plain.h and, from the subdirectory csrc/div/, the division's k_divmod_words; each of these defined in the unit that launches it, over the bit-field helpers of csrc/sc_plain_words.h: the secure multiplication's two in csrc/sc_launch_mul.hip, the inner product's two in csrc/sc_launch_dot.hip, the one-hot encoding's three in csrc/sc_launch_lookup.hip, the product along an axis in csrc/sc_launch_reduce.hip, the running product in csrc/sc_launch_scan.hip, the linear map with public weights in csrc/sc_launch_lin.hip).  The parts compile in parallel; an object is rebuilt only when one of the files it includes changed,
so a change of host logic costs the seconds of the host units it touches and a kernel change only the parts that hold that kernel.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
OUT = os.path.join(HERE, "libsc_amd.so")
INCLUDE = os.path.join(HERE, "..", "..", "include")
# -pragma-unroll-threshold: the L = 27 limb-step loops (1458 multiply-adds per block) must be fully unrolled, otherwise
# the column registers are indexed dynamically and land in scratch memory (50x slower)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-pragma-unroll-threshold=1000000"]
# (object name, source, extra flags)
UNITS = [("sc_lib", "sc_lib.hip", [])] + \
        [(f"sc_launch_vm{p}", "sc_launch_vm.hip", [f"-DSC_PART={p}"]) for p in range(3)] + \
        [(f"sc_launch_pvm{p}", "sc_launch_pvm.hip", [f"-DSC_PART={p}"]) for p in range(3)] + \
        [("sc_launch_misc", "sc_launch_misc.hip", []), ("sc_launch_mul", "sc_launch_mul.hip", []),
         ("sc_launch_dot", "sc_launch_dot.hip", []), ("sc_launch_lookup", "sc_launch_lookup.hip", []),
         ("sc_launch_reduce", "sc_launch_reduce.hip", []), ("sc_launch_scan", "sc_launch_scan.hip", [])]
# The fourteenth unit, the linear map with public weights, is listed apart: tests/test_scan_cpu.py holds UNITS at the
# thirteen above, whose objects this unit leaves byte for byte what they were.  The library is built from ALL_UNITS.
LINEAR_UNITS = [("sc_launch_lin", "sc_launch_lin.hip", [])]
# The host units beside sc_lib.hip; each begins with its own includes and compiles on its own.
HOST_UNITS = [(n, n + ".hip", []) for n in ("sc_families", "sc_schemes", "sc_topk")]
ALL_UNITS = UNITS + LINEAR_UNITS + HOST_UNITS
# every source under csrc/, its subdirectories included (csrc/div/ holds k_divmod_words, which sc_launch_misc.hip includes; _closure
# follows an include into a subdirectory as it follows any other)
DEPS = sorted(os.path.join(d, f) for d, _, fs in os.walk(CSRC) for f in fs if f.endswith((".hip", ".h"))) + [
    os.path.join(INCLUDE, "sc_amd.h"), os.path.join(INCLUDE, "sc_amd_dev.h")]
_INC = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _closure(path: str, seen: set[str] | None = None) -> set[str]:
    """`path` and every file it includes with quotes, transitively."""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in _INC.findall(open(path).read()):
        _closure(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def _stale(obj: str, src: str) -> bool:
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in _closure(src) | {os.path.abspath(__file__)})


def needs_build() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build_lib(force: bool = False, verbose: bool = True, extra_flags: tuple[str, ...] = ()) -> str:
    if not force and not extra_flags and not needs_build():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    jobs = []
    for name, src, flags in ALL_UNITS:
        obj, path = os.path.join(OBJ, name + ".o"), os.path.join(CSRC, src)
        if force or extra_flags or _stale(obj, path):
            jobs.append((obj, [hipcc, *FLAGS, *flags, *extra_flags, "-c", path, "-o", obj]))

    def run(job):
        obj, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if proc.returncode == 0 and "loop not unrolled" in proc.stderr:
            # a partially unrolled limb loop indexes the column registers dynamically -> scratch memory -> ~50x slower
            os.remove(obj)
            return obj, 1, proc.stderr + "\nhipcc did not fully unroll a limb loop (see -pragma-unroll-threshold in build.py)"
        return obj, proc.returncode, proc.stderr

    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1, 8))) as pool:
        results = list(pool.map(run, jobs))
    failed = [(o, err) for o, rc, err in results if rc != 0]
    if failed:
        for o, err in failed:
            sys.stderr.write(f"--- {os.path.basename(o)}\n{err}\n")
            if os.path.exists(o):
                os.remove(o)
        raise RuntimeError("hipcc failed for " + ", ".join(os.path.basename(o) for o, _ in failed))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *(os.path.join(OBJ, n + ".o") for n, _, _ in ALL_UNITS), "-o", OUT, "-ldl"]
    if verbose:
        print(" ".join(link), flush=True)
    proc = subprocess.run(link, stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stderr)
        raise subprocess.CalledProcessError(proc.returncode, link)
    return OUT


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)

"""Plain-Python reference of the product along an axis (sc_modprod_axis) and of its level plan, and the table of compiled k_prod_axis
and k_scan_axis instances the GPU tier runs.  No torch at import."""
from __future__ import annotations

import os
import re

# every k_prod_axis<G, L> and k_scan_axis<G, L> that csrc/sc_launch_reduce.hip and csrc/sc_launch_scan.hip compile, from the one list in
# csrc/sc_launch_axis.h; tests/test_gpu_aggregate.py and tests/test_gpu_scan.py run one parametrised case per row and
# tests/test_aggregate_cpu.py and tests/test_scan_cpu.py compare this table with the source
INSTANCES = [(2, 18), (2, 27), (4, 14), (4, 18), (4, 27), (8, 14), (8, 18), (8, 27), (16, 14), (16, 18)]

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "protocols", "secure_comparison_amd", "csrc")
SOURCE = os.path.join(CSRC, "sc_launch_axis.h")
UNITS = [os.path.join(CSRC, "sc_launch_reduce.hip"), os.path.join(CSRC, "sc_launch_scan.hip")]


def compiled_instances(text: str) -> list[tuple[int, int]]:
    """The (G, L) pairs of the SC_AXIS_INSTANCES list of the launchers' shared header."""
    m = re.search(r"#define\s+SC_AXIS_INSTANCES\(X\)(.*)", text)
    if not m:
        raise ValueError("SC_AXIS_INSTANCES not found")
    return [(int(g), int(l)) for g, l in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]


def units_share_the_list() -> bool:
    """Both launch units include the shared header and neither defines an instance list of its own."""
    texts = [open(u).read() for u in UNITS]
    return all('#include "sc_launch_axis.h"' in t and not re.search(r"#define\s+SC_\w*INSTANCES", t) for t in texts)


def missing_rows(text: str, table=None) -> list[tuple[int, int]]:
    """Compiled instances without a row in `table` (default: INSTANCES)."""
    table = INSTANCES if table is None else table
    return [c for c in compiled_instances(text) if c not in table]


def prod_axis(n: int, x: list[int], outer: int, K: int, inner: int) -> list[int]:
    """out[o][i] = prod_j x[o][j][i] mod n for x flat in [outer][K][inner] order; flat [outer][inner]."""
    assert len(x) == outer * K * inner
    out = []
    for o in range(outer):
        for i in range(inner):
            v = 1
            for j in range(K):
                v = v * x[(o * K + j) * inner + i] % n
            out.append(v % n)
    return out


def chains_per_level(K: int, chunk_of) -> list[int]:
    """Chains per output at every level of a tree over K members: a level with chunk length c = chunk_of(level, K) (cut to K) groups its
    members c at a time, counted one by one here, and hands one partial per chain to the next level; the last level has one chain."""
    out, level = [], 0
    while True:
        c = min(chunk_of(level, K), K)
        chains, left = 0, K
        while left > 0:
            left -= min(c, left)
            chains += 1
        out.append(chains)
        if chains == 1:
            return out
        K, level = chains, level + 1

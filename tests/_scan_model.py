"""Plain-Python reference of the running product along an axis (sc_modscan_axis), a launch-by-launch count of its plan that walks the
members one by one; the table of compiled k_scan_axis instances is k_prod_axis' (tests/_reduce_model.py).  No torch at import."""
from __future__ import annotations

from _reduce_model import INSTANCES, SOURCE, compiled_instances, missing_rows, units_share_the_list  # noqa: F401


def scan_axis(n: int, x: list[int], outer: int, K: int, inner: int) -> list[int]:
    """out[o][j][i] = prod_{j' <= j} x[o][j'][i] mod n for x flat in [outer][K][inner] order; flat in the same order."""
    assert len(x) == outer * K * inner
    out = [0] * len(x)
    for o in range(outer):
        for i in range(inner):
            v = 1
            for j in range(K):
                at = (o * K + j) * inner + i
                v = v * x[at] % n
                out[at] = v % n
    return out


def launches(outer: int, K: int, inner: int, resident_groups: int, forced: int = 0) -> list[tuple[str, int, int, int]]:
    """The launches (kind, K, chunk, chains) of one call, counted member by member: a level is direct when its scans fill the resident
    group slots by themselves (automatic chunks only) or fit one chunk; otherwise its members are dealt into chunks one at a time, every
    chunk that another follows gets a total, the totals are scanned by the same rule and the level is scanned again with a chain per
    chunk."""
    if forced:
        c = forced
    else:
        c = -(-(outer * K * inner) // resident_groups)
        c = 4 if c < 4 else 32 if c > 32 else c
    if (not forced and outer * inner >= resident_groups) or K <= c:
        return [("scan", K, K, outer * inner)]
    chunks, fill = 0, 0
    for _ in range(K):                       # one member at a time
        if fill == 0:
            chunks += 1
        fill = (fill + 1) % c
    followed = chunks - 1                    # every chunk but the last is followed by another, and is full
    return ([("totals", K, c, outer * followed * inner)] + launches(outer, followed, inner, resident_groups, forced) +
            [("scan", K, c, outer * chunks * inner)])


def count(plan, kind: str) -> int:
    return sum(1 for p in plan if p[0] == kind)


def products(plan) -> int:
    """Montgomery products of a plan: two per member of every scan launch, one per member past the first of every totalled chunk."""
    total = 0
    for kind, K, c, chains in plan:
        if kind == "scan":
            per_scan = chains // max(1, -(-K // c))          # outer * inner
            total += 2 * K * per_scan
        else:
            total += chains * (c - 1)
    return total

"""Pure-Python model of the secure top-m on Python values: the plaintext network with keep flags and the package's tie rule, on the
conventions of tests/_sort_model.py's apply, and the bookkeeping of dead outputs.

A comparator is (i, j, keep_i, keep_j), i < j.  F is the element compared first (i for the smallest, j for the largest) and G the
other; delta = key(F) <= key(G), lo = F if delta else G, hi = G if delta else F; lo belongs at F's position and hi at G's, and each
is written only when that position's keep flag is set.  Equal keys are never exchanged.
"""
from __future__ import annotations


def apply(layers, rows, largest=False, key=lambda t: t[0]):
    """The rows after the network; a dead output leaves its position as it was."""
    out = [list(r) for r in rows]
    for layer in layers:
        for r in out:
            for i, j, keep_i, keep_j in layer:
                (fi, fk), (gi, gk) = ((j, keep_j), (i, keep_i)) if largest else ((i, keep_i), (j, keep_j))
                F, G = r[fi], r[gi]
                d = key(F) <= key(G)
                lo, hi = (F, G) if d else (G, F)
                if fk:
                    r[fi] = lo
                if gk:
                    r[gi] = hi
    return out


def written(layers, k):
    """The positions some comparator writes (a live output); every other position keeps its input to the end."""
    out = set()
    for layer in layers:
        for i, j, keep_i, keep_j in layer:
            if keep_i:
                out.add(i)
            if keep_j:
                out.add(j)
    assert all(0 <= p < k for p in out)
    return out


def stale_reads(layers, k, outputs):
    """Comparators and final outputs that read a position after a dead output was left there: must be empty.  A dead output makes
    its position stale; only a live write to it would make it fresh again, and a comparator reads both of its positions."""
    stale, bad = set(), []
    for t, layer in enumerate(layers):
        for i, j, keep_i, keep_j in layer:
            bad += [(t, i, j, p) for p in (i, j) if p in stale]
            for p, keep in ((i, keep_i), (j, keep_j)):
                if keep:
                    stale.discard(p)
                else:
                    stale.add(p)
    return bad + [("output", p) for p in outputs if p in stale]

"""Pure-Python model of the secure sort on Python ints: Batcher's network, the plaintext network with the package's tie rule, and
the compare-exchange (a selection with sigma = delta whose finish shares one inversion between both outputs), with injected draws.

Independent of the package: the network is built here by the recursive odd-even merge, and the selection steps come from
tests/_select_model.py.  Keys are oracle/sc_oracle.py PaillierKey objects (g = N + 1).
"""
from __future__ import annotations

import _select_model as sm


def _merge(lo, hi, r):
    """Comparators of the odd-even merge of the sorted halves of [lo, hi] (inclusive) at stride r."""
    step = 2 * r
    if step < hi - lo:
        yield from _merge(lo, hi, step)
        yield from _merge(lo + r, hi, step)
        yield from ((i, i + r) for i in range(lo + r, hi - r, step))
    else:
        yield (lo, lo + r)


def _sort(lo, hi):
    if hi - lo >= 1:
        mid = lo + (hi - lo) // 2
        yield from _sort(lo, mid)
        yield from _sort(mid + 1, hi)
        yield from _merge(lo, hi, 1)


def comparators(k):
    """Batcher's odd-even merge sort for k inputs: the power-of-two network for 2^ceil(log2 k) without the comparators that touch an
    index >= k, in sequential order."""
    n = 1 << (k - 1).bit_length()
    return [(i, j) for i, j in (_sort(0, n - 1) if n > 1 else ()) if j < k]


def batcher_counts(m):
    """(layers, comparators) of the network for n = 2^m: m (m + 1) / 2 and (m^2 - m + 4) 2^(m - 2) - 1."""
    return m * (m + 1) // 2, ((m * m - m + 4) << m) // 4 - 1


def apply(layers, rows, descending=False, key=lambda t: t[0]):
    """The plaintext network on rows of tuples (key first, then payload / index): per comparator (i, j), F is the element compared
    first (i ascending, j descending) and G the other; delta = key(F) <= key(G), lo = F if delta else G, hi = G if delta else F; lo
    goes to F's position and hi to G's.  Equal keys are never exchanged."""
    out = [list(r) for r in rows]
    for layer in layers:
        for r in out:
            for i, j in layer:
                fi, gi = (j, i) if descending else (i, j)
                F, G = r[fi], r[gi]
                d = key(F) <= key(G)
                r[fi], r[gi] = (F, G) if d else (G, F)
    return out


def compare_exchange(sk, kappa, widths, delta, f_cs, g_cs, draws, shared_inversion=True, d_key=None, trace=None):
    """([[lo_j]], [[hi_j]]) of one compare-exchange from [[delta]] and the operand ciphertexts of every column: the selection with
    sigma = delta, base F_j and d_j = G_j F_j^-1 (1 + 2^w_j N), then hi = F ab^2 U^-1 and lo = G T^2 U^-1 with U = T ab (one
    inversion), or -- shared_inversion=False -- S = ab T^-1, hi = F S, lo = G S^-1 (two).  d_key: the key column's [[d]] when it is
    the comparison's own (the same plaintext under the randomizer of the sent [[z]]); trace: receives P and Bob's products."""
    n, n2 = sk.n, sk.n2
    r_a, r_bs, rho_p, rhos = draws
    d_cs = [g * pow(f, -1, n2) % n2 * (1 + (1 << w) * n) % n2 for f, g, w in zip(f_cs, g_cs, widths)]
    if d_key is not None:
        d_cs[0] = d_key
    P = sm.pack(sk, kappa, widths, delta, d_cs, r_a, r_bs, rho_p)
    ab_cs, _, bad = sm.mult(sk, kappa, widths, P, rhos)
    assert not bad
    if trace is not None:
        trace.update(P=P, products=ab_cs)
    lo, hi = [], []
    for w, f, g, d, ab, r_b in zip(widths, f_cs, g_cs, d_cs, ab_cs, r_bs):
        T = pow(delta, r_b + (1 << w), n2) * pow(d, r_a, n2) % n2 * sm.enc(sk, r_a * r_b) % n2
        if shared_inversion:
            u_inv = pow(T * ab % n2, -1, n2)
            hi.append(f * ab % n2 * ab % n2 * u_inv % n2)
            lo.append(g * T % n2 * T % n2 * u_inv % n2)
        else:
            s = ab * pow(T, -1, n2) % n2
            hi.append(f * s % n2)
            lo.append(g * pow(s, -1, n2) % n2)
    return lo, hi

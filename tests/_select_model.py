"""Pure-Python model of the secure selection (pack -> mult -> finish) on Python ints, with injected draws.

Independent of the package: the field layout is recomputed here from the protocol's definition ("Secure selection").
Keys are oracle/sc_oracle.py PaillierKey objects (g = N + 1).
"""
from __future__ import annotations

import random


def layout(kappa, widths, nbits):
    """(s, offsets, field bits, end); ValueError when the packed fields or one product do not fit below N."""
    s = kappa + 1
    fb = [w + kappa + 2 for w in widths]
    offs, off = [], s
    for f in fb:
        offs.append(off)
        off += f
    if off >= nbits - 1 or any(s + f >= nbits - 1 for f in fb):
        raise ValueError("layout does not fit")
    return s, offs, fb, off


def enc(sk, m, rho=None):
    c = (1 + (m % sk.n) * sk.n) % sk.n2
    return c if rho is None else c * pow(rho, sk.n, sk.n2) % sk.n2


def dec(sk, c):
    return (pow(c, sk.lam, sk.n2) - 1) // sk.n * sk.mu % sk.n


def draw(rng, kappa, widths, n):
    """Alice's r_a, r_b (one per column), rho_p and Bob's randomizers (one per column)."""
    return (rng.getrandbits(kappa), [rng.getrandbits(w + 1 + kappa) for w in widths], rng.randrange(1, n),
            [rng.randrange(1, n) for _ in widths])


def pack(sk, kappa, widths, sigma_c, d_cs, r_a, r_bs, rho_p):
    n, n2 = sk.n, sk.n2
    _, offs, _, _ = layout(kappa, widths, n.bit_length())
    R = r_a + sum(r_b << o for r_b, o in zip(r_bs, offs))
    P = sigma_c * enc(sk, R) % n2 * pow(rho_p, n, n2) % n2
    for d, o in zip(d_cs, offs):
        P = P * pow(d, 1 << o, n2) % n2
    return P


def mult(sk, kappa, widths, P, rhos):
    """Bob: ([[a b_j]] freshly randomized, the products a b_j, whether P exceeded the layout)."""
    s, offs, fb, end = layout(kappa, widths, sk.n.bit_length())
    p = dec(sk, P)
    a = p & ((1 << s) - 1)
    prods = [a * ((p >> o) & ((1 << f) - 1)) for o, f in zip(offs, fb)]
    return [enc(sk, m, rho) for m, rho in zip(prods, rhos)], prods, (p >> end) != 0


def finish(sk, kappa, widths, sigma_c, d_cs, b_cs, prod_cs, r_a, r_bs):
    n, n2 = sk.n, sk.n2
    out = []
    for w, d, b, pc, r_b in zip(widths, d_cs, b_cs, prod_cs, r_bs):
        T = pow(sigma_c, r_b + (1 << w), n2) * pow(d, r_a, n2) % n2 * enc(sk, r_a * r_b) % n2
        out.append(b * pc % n2 * pow(T, -1, n2) % n2)
    return out


def select(sk, kappa, widths, sigma_c, d_cs, b_cs, draws):
    r_a, r_bs, rho_p, rhos = draws
    P = pack(sk, kappa, widths, sigma_c, d_cs, r_a, r_bs, rho_p)
    prod_cs, _, bad = mult(sk, kappa, widths, P, rhos)
    assert not bad
    return finish(sk, kappa, widths, sigma_c, d_cs, b_cs, prod_cs, r_a, r_bs)


def _select_plain(sk, kappa, rng, sigma, cols):
    """cols: [(a, b, w)]: encrypt, select b + sigma (a - b) through the protocol, decrypt."""
    widths = [w for _, _, w in cols]
    n = sk.n
    sigma_c = enc(sk, sigma, rng.randrange(1, n))
    d_cs = [enc(sk, a - b + (1 << w), rng.randrange(1, n)) for a, b, w in cols]
    b_cs = [enc(sk, b, rng.randrange(1, n)) for _, b, _ in cols]
    outs = select(sk, kappa, widths, sigma_c, d_cs, b_cs, draw(rng, kappa, widths, n))
    return [dec(sk, c) for c in outs]


def minimum(sk, x, y, l, rng, kappa=40):
    return _select_plain(sk, kappa, rng, int(x <= y), [(x, y, l)])[0]


def maximum(sk, x, y, l, rng, kappa=40):
    return _select_plain(sk, kappa, rng, 1 - int(x <= y), [(x, y, l)])[0]


def index_bits(k):
    return max(1, (k - 1).bit_length())


def argext(sk, values, l, rng, kappa=40, want_max=False):
    """(value, index) of the tournament the package runs: pairs (2t, 2t + 1), the odd element carried over, ties to the left."""
    k = len(values)
    wi = index_bits(k)
    cur = [(v, i) for i, v in enumerate(values)]
    while len(cur) > 1:
        nxt = []
        for t in range(len(cur) // 2):
            (lv, li), (rv, ri) = cur[2 * t], cur[2 * t + 1]
            sigma = int(rv <= lv) if want_max else int(lv <= rv)     # the left one wins
            nxt.append(tuple(_select_plain(sk, kappa, rng, sigma, [(lv, rv, l), (li, ri, wi)])))
        if len(cur) % 2:
            nxt.append(cur[-1])
        cur = nxt
    return cur[0]


if __name__ == "__main__":      # pragma: no cover
    from oracle import sc_oracle as o

    sk = o.PaillierKey.generate(512, random.Random(1))
    print(minimum(sk, 3, 5, 8, random.Random(2)), argext(sk, [4, 1, 1, 7], 8, random.Random(3)))

"""Pure-Python model of the secure multiplication (pack -> mult -> finish) on Python ints, with injected draws.

Independent of the package: the field layout is recomputed here from the protocol's definition.  Keys are
oracle/sc_oracle.py PaillierKey objects (g = N + 1).  Draws of one row: (r_a, [r_b_j], rho_p, [rho_j]).
"""
from __future__ import annotations

import random


def layout(kappa, wx, wy, nbits):
    """(s, offsets, field bits, end, exponent bits); ValueError when the packed fields or one product do not fit below N, or an
    argument is out of range."""
    if not 1 <= kappa <= 62 or not 1 <= wx <= 255 or not 1 <= len(wy) <= 4 or any(not 1 <= w <= 255 for w in wy):
        raise ValueError("bad multiplication parameters")
    s = wx + kappa + 1
    fb = [w + kappa + 1 for w in wy]
    offs, off = [], s
    for f in fb:
        offs.append(off)
        off += f
    if not off < nbits - 1 or any(not s + f < nbits - 1 for f in fb):
        raise ValueError("layout does not fit")
    return s, offs, fb, off, max([s] + fb)


def enc(sk, m, rho=None):
    c = (1 + (m % sk.n) * sk.n) % sk.n2
    return c if rho is None else c * pow(rho, sk.n, sk.n2) % sk.n2


def dec(sk, c):
    return (pow(c, sk.lam, sk.n2) - 1) // sk.n * sk.mu % sk.n


def offsets(wx, wy, signed):
    return (1 << (wx - 1) if signed else 0), [(1 << (w - 1) if signed else 0) for w in wy]


def draw(rng, kappa, wx, wy, n):
    """Alice's r_a, r_b (one per column), rho_p and Bob's randomizers (one per column)."""
    return (rng.getrandbits(wx + kappa), [rng.getrandbits(w + kappa) for w in wy], rng.randrange(1, n), [rng.randrange(1, n) for _ in wy])


def plain(kappa, wx, wy, signed, r_a, r_bs):
    """Alice's plaintext values (e_y, [e_x_j], [e_x_j e_y])."""
    ox, oys = offsets(wx, wy, signed)
    e_y = r_a + ox
    e_xs = [r_b + oy for r_b, oy in zip(r_bs, oys)]
    return e_y, e_xs, [e_x * e_y for e_x in e_xs]


def pack(sk, kappa, wx, wy, signed, x_c, y_cs, r_a, r_bs, rho_p):
    n, n2 = sk.n, sk.n2
    _, offs, _, _, _ = layout(kappa, wx, wy, n.bit_length())
    e_y, e_xs, _ = plain(kappa, wx, wy, signed, r_a, r_bs)
    R = e_y + sum(e_x << o for e_x, o in zip(e_xs, offs))
    P = x_c * enc(sk, R) % n2 * pow(rho_p, n, n2) % n2
    for y, o in zip(y_cs, offs):
        P = P * pow(y, 1 << o, n2) % n2
    return P


def mult(sk, kappa, wx, wy, P, rhos):
    """Bob: ([[A B_j]] freshly randomized, the products A B_j, whether P exceeded the layout)."""
    s, offs, fb, end, _ = layout(kappa, wx, wy, sk.n.bit_length())
    p = dec(sk, P)
    a = p & ((1 << s) - 1)
    prods = [a * ((p >> o) & ((1 << f) - 1)) for o, f in zip(offs, fb)]
    return [enc(sk, m, rho) for m, rho in zip(prods, rhos)], prods, (p >> end) != 0


def finish(sk, kappa, wx, wy, signed, x_c, y_cs, prod_cs, r_a, r_bs, bases=None, coef=1):
    """base_j [[x y_j]]^coef, coef in {+1, -1, -2}."""
    n2 = sk.n2
    e_y, e_xs, rabs = plain(kappa, wx, wy, signed, r_a, r_bs)
    out = []
    for j, (y, pc, e_x, rab) in enumerate(zip(y_cs, prod_cs, e_xs, rabs)):
        T = pow(x_c, e_x, n2) * pow(y, e_y, n2) % n2 * enc(sk, rab) % n2
        xy = pc * pow(T, -1, n2) % n2
        r = pow(xy, coef, n2)
        out.append(r if bases is None else bases[j] * r % n2)
    return out


def multiply_enc(sk, kappa, wx, wy, signed, x_c, y_cs, draws, bases=None, coef=1):
    r_a, r_bs, rho_p, rhos = draws
    P = pack(sk, kappa, wx, wy, signed, x_c, y_cs, r_a, r_bs, rho_p)
    prod_cs, _, bad = mult(sk, kappa, wx, wy, P, rhos)
    assert not bad
    return finish(sk, kappa, wx, wy, signed, x_c, y_cs, prod_cs, r_a, r_bs, bases, coef)


def multiply(sk, x, ys, wx, wy, rng, signed=False, kappa=40, draws=None):
    """Plaintexts in, plaintext residues x * y_j mod N out, through the protocol."""
    n = sk.n
    x_c = enc(sk, x, rng.randrange(1, n))
    y_cs = [enc(sk, y, rng.randrange(1, n)) for y in ys]
    draws = draws if draws is not None else draw(rng, kappa, wx, wy, n)
    return [dec(sk, c) for c in multiply_enc(sk, kappa, wx, wy, signed, x_c, y_cs, draws)]


def bit_op(sk, a, b, op, rng, kappa=40):
    """a AND / OR / XOR b on bits through the protocol: OR and XOR pass base = [[a]] [[b]] and coef = -1 / -2."""
    n = sk.n
    a_c, b_c = enc(sk, a, rng.randrange(1, n)), enc(sk, b, rng.randrange(1, n))
    coef = {"and": 1, "or": -1, "xor": -2}[op]
    bases = None if coef == 1 else [a_c * b_c % sk.n2]
    return dec(sk, multiply_enc(sk, kappa, 1, [1], False, a_c, [b_c], draw(rng, kappa, 1, [1], n), bases, coef)[0])


def equal(sk, x, y, rng, kappa=40):
    """([x == y], [x <= y], [y <= x]): the two comparison bits are taken as given (the comparison has its own model), the AND runs
    through the protocol."""
    le, ge = int(x <= y), int(y <= x)
    return bit_op(sk, le, ge, "and", rng, kappa), le, ge


def in_range(sk, x, lo, hi, rng, kappa=40):
    return bit_op(sk, int(lo <= x), int(x <= hi), "and", rng, kappa)


if __name__ == "__main__":      # pragma: no cover
    from oracle import sc_oracle as o

    sk = o.PaillierKey.generate(512, random.Random(1))
    print(multiply(sk, 3, [5, 7], 8, [8, 8], random.Random(2)), equal(sk, 4, 4, random.Random(3)))

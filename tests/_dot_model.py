"""Pure-Python model of the secure inner product (pack -> answer -> finish) on Python ints, with injected draws.

Independent of the package: the layout and the pair-to-message mapping are recomputed here from the protocol's definition (DESIGN.md
§8g).  Keys are oracle/sc_oracle.py PaillierKey objects (g = N + 1).  Draws of one row: (r_as [k], r_bs [k] or None for a square,
rho_ps [M], rho_d).
"""
from __future__ import annotations

import random


def layout(kappa, wx, wy, square, k, nbits):
    """(sa, sb, pb, g, M, ebits); ValueError when a quantity is out of range, when no pair fits or when the sum of k products does
    not stay below N."""
    if not 1 <= kappa <= 62 or not 1 <= wx <= 255 or not 1 <= k <= 1024 or (not square and not 1 <= wy <= 255):
        raise ValueError("bad inner-product parameters")
    sa = wx + kappa + 1
    sb = 0 if square else wy + kappa + 1
    pb = sa + sb
    g = 0
    while (g + 1) * pb < nbits - 1:          # the largest g with g pb < bits(N) - 1, by the definition
        g += 1
    if g < 1:
        raise ValueError("one pair does not fit")
    prod = 2 * sa if square else sa + sb
    lg = 0
    while (1 << lg) < k:                     # ceil(log2 k)
        lg += 1
    if not prod + lg < nbits - 1:
        raise ValueError("the sum does not fit")
    return sa, sb, pb, g, (k + g - 1) // g, (sa + 1 if square else max(sa, sb))


def position(j, M):
    """(message, position) of pair j."""
    return j % M, j // M


def members(m, k, M):
    """The pairs of message m, by ascending position."""
    return [j for j in range(k) if j % M == m]


def enc(sk, m, rho=None):
    c = (1 + (m % sk.n) * sk.n) % sk.n2
    return c if rho is None else c * pow(rho, sk.n, sk.n2) % sk.n2


def dec(sk, c):
    return (pow(c, sk.lam, sk.n2) - 1) // sk.n * sk.mu % sk.n


def masks(kappa, wx, wy, signed, square, r_as, r_bs):
    """Alice's (a_j, b_j): the draws plus the offsets; b is None for a square."""
    ox = 1 << (wx - 1) if signed else 0
    a = [r + ox for r in r_as]
    if square:
        return a, None
    oy = 1 << (wy - 1) if signed else 0
    return a, [r + oy for r in r_bs]


def draw(rng, kappa, wx, wy, square, k, n):
    _, _, _, _, M, _ = layout(kappa, wx, wy, square, k, n.bit_length())
    return ([rng.getrandbits(wx + kappa) for _ in range(k)], None if square else [rng.getrandbits(wy + kappa) for _ in range(k)],
            [rng.randrange(1, n) for _ in range(M)], rng.randrange(1, n))


def plain(kappa, wx, wy, signed, square, k, nbits, r_as, r_bs):
    """Alice's plaintext values: (exponent planes e, packed masks R [M], S)."""
    sa, sb, pb, g, M, _ = layout(kappa, wx, wy, square, k, nbits)
    a, b = masks(kappa, wx, wy, signed, square, r_as, r_bs)
    R = [0] * M
    for j in range(k):
        m, t = position(j, M)
        R[m] += a[j] << (t * pb)
        if not square:
            R[m] += b[j] << (t * pb + sa)
    if square:
        return [2 * v for v in a], R, sum(v * v for v in a)
    return b + a, R, sum(u * v for u, v in zip(a, b))


def pack(sk, kappa, wx, wy, signed, square, x_cs, y_cs, r_as, r_bs, rho_ps):
    """The M messages of one row: P_m = prod_t [[x_(tM+m)]]^(2^(t pb)) [[y_(tM+m)]]^(2^(t pb + sa)) (1 + R_m N) rho_p_m^N.  The product
    over the positions is evaluated from the top one down, F_t = [[x]] [[y]]^(2^sa) and acc = acc^(2^pb) F_t, which is the same
    residue for one exponentiation's worth of squarings per message instead of one per pair."""
    n, n2, k = sk.n, sk.n2, len(x_cs)
    sa, sb, pb, g, M, _ = layout(kappa, wx, wy, square, k, n.bit_length())
    _, R, _ = plain(kappa, wx, wy, signed, square, k, n.bit_length(), r_as, r_bs)
    out = []
    for m in range(M):
        acc = 1
        for j in reversed(members(m, k, M)):
            f = x_cs[j] if square else x_cs[j] * pow(y_cs[j], 1 << sa, n2) % n2
            acc = pow(acc, 1 << pb, n2) * f % n2
        out.append(acc * enc(sk, R[m]) % n2 * pow(rho_ps[m], n, n2) % n2)
    return out


def answer(sk, kappa, wx, wy, square, k, Ps, rho_d):
    """Bob: ([[D]] freshly randomized, D, whether a message exceeded its own end)."""
    sa, sb, pb, g, M, _ = layout(kappa, wx, wy, square, k, sk.n.bit_length())
    assert len(Ps) == M
    D, bad = 0, False
    for m, P in enumerate(Ps):
        p = dec(sk, P)
        n_m = len(members(m, k, M))
        bad |= (p >> (n_m * pb)) != 0
        for t in range(n_m):
            A = (p >> (t * pb)) & ((1 << sa) - 1)
            D += A * A if square else A * ((p >> (t * pb + sa)) & ((1 << sb) - 1))
    return enc(sk, D, rho_d), D, bad


def finish(sk, kappa, wx, wy, signed, square, x_cs, y_cs, d_c, r_as, r_bs, base=None, coef=1):
    """base [[sum_j x_j y_j]]^coef, coef in {+1, -1, -2}."""
    n2, k = sk.n2, len(x_cs)
    e, _, S = plain(kappa, wx, wy, signed, square, k, sk.n.bit_length(), r_as, r_bs)
    T = enc(sk, S)
    for j in range(k):
        T = T * pow(x_cs[j], e[j], n2) % n2
        if not square:
            T = T * pow(y_cs[j], e[k + j], n2) % n2
    r = pow(d_c * pow(T, -1, n2) % n2, coef, n2)
    return r if base is None else base * r % n2


def dot_enc(sk, kappa, wx, wy, signed, square, x_cs, y_cs, draws, base=None, coef=1):
    r_as, r_bs, rho_ps, rho_d = draws
    Ps = pack(sk, kappa, wx, wy, signed, square, x_cs, y_cs, r_as, r_bs, rho_ps)
    d_c, _, bad = answer(sk, kappa, wx, wy, square, len(x_cs), Ps, rho_d)
    assert not bad
    return finish(sk, kappa, wx, wy, signed, square, x_cs, y_cs, d_c, r_as, r_bs, base, coef)


def dot(sk, xs, ys, wx, wy, rng, signed=False, kappa=40, draws=None):
    """Plaintexts in, the plaintext residue sum_j x_j y_j mod N out, through the protocol; ys None: the sum of squares."""
    n, square = sk.n, ys is None
    x_cs = [enc(sk, x, rng.randrange(1, n)) for x in xs]
    y_cs = None if square else [enc(sk, y, rng.randrange(1, n)) for y in ys]
    draws = draws if draws is not None else draw(rng, kappa, wx, wy, square, len(xs), n)
    return dec(sk, dot_enc(sk, kappa, wx, wy, signed, square, x_cs, y_cs, draws))


if __name__ == "__main__":      # pragma: no cover
    from oracle import sc_oracle as o

    sk = o.PaillierKey.generate(512, random.Random(1))
    print(dot(sk, [3, 5, 7], [2, 4, 6], 8, 8, random.Random(2)), dot(sk, [3, 5, 7], None, 8, 0, random.Random(3)))

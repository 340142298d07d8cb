"""Pure-Python model of the secure one-hot encoding (pack -> answer -> rotate) on Python ints, with injected draws.

Independent of the package: the layout, the placement of the fields, the remainders and the rotation are recomputed here from the
protocol's definition.  Keys are oracle/sc_oracle.py PaillierKey objects (g = N + 1).  Draws of one row: (rs [m],
rho_ps [M], rho_es [m][k]).
"""
from __future__ import annotations

import random


def layout(kappa, ib, k, m, nbits):
    """(f, g, M, rw); ValueError when a quantity is out of range or when one field does not fit below N."""
    if not 1 <= kappa <= 62 or not 1 <= ib <= 32 or not 1 <= k <= 1024 or not 1 <= m <= 65536:
        raise ValueError("bad one-hot parameters")
    f = ib + kappa + 1
    if not f < nbits - 1:
        raise ValueError("one field does not fit")
    g = 0
    while (g + 1) * f < nbits - 1:           # the largest g with g f < bits(N) - 1, by the definition
        g += 1
    rw = 1
    while 32 * rw < ib + kappa:              # the words of a mask
        rw += 1
    return f, g, (m + g - 1) // g, rw


def position(q, g):
    """(message, position) of index q."""
    return q // g, q % g


def members(mm, m, g):
    """The indices of message mm, by ascending position."""
    return [q for q in range(m) if q // g == mm]


def enc(sk, v, rho=None):
    c = (1 + (v % sk.n) * sk.n) % sk.n2
    return c if rho is None else c * pow(rho, sk.n, sk.n2) % sk.n2


def dec(sk, c):
    return (pow(c, sk.lam, sk.n2) - 1) // sk.n * sk.mu % sk.n


def draw(rng, kappa, ib, k, m, n, with_bob=True):
    _, _, M, _ = layout(kappa, ib, k, m, n.bit_length())
    return ([rng.getrandbits(ib + kappa) for _ in range(m)], [rng.randrange(1, n) for _ in range(M)],
            [[rng.randrange(1, n) for _ in range(k)] for _ in range(m)] if with_bob else None)


def plain(kappa, ib, k, m, nbits, rs):
    """Alice's plaintext values: (the packed masks R [M], the rotations rot [m])."""
    f, g, M, _ = layout(kappa, ib, k, m, nbits)
    R = [0] * M
    for q in range(m):
        mm, t = position(q, g)
        R[mm] += rs[q] << (t * f)
    return R, [r % k for r in rs]


def pack(sk, kappa, ib, k, i_cs, rs, rho_ps):
    """The M messages of one row: P_mm = prod_j [[i_(mm g + j)]]^(2^(j f)) (1 + R_mm N) rho_p_mm^N."""
    n, n2, m = sk.n, sk.n2, len(i_cs)
    f, g, M, _ = layout(kappa, ib, k, m, n.bit_length())
    R, _ = plain(kappa, ib, k, m, n.bit_length(), rs)
    out = []
    for mm in range(M):
        acc = 1
        for q in members(mm, m, g):
            acc = acc * pow(i_cs[q], 1 << ((q % g) * f), n2) % n2
        out.append(acc * enc(sk, R[mm]) % n2 * pow(rho_ps[mm], n, n2) % n2)
    return out


def split(kappa, ib, k, m, nbits, ps):
    """Bob's plaintext half from the decrypted messages ps [M]: (the fields d [m], the hot positions j [m], whether a message has a bit at
    or above its own end)."""
    f, g, M, _ = layout(kappa, ib, k, m, nbits)
    assert len(ps) == M
    d, bad = [], False
    for mm, p in enumerate(ps):
        qs = members(mm, m, g)
        bad |= (p >> (len(qs) * f)) != 0
        d += [(p >> ((q % g) * f)) & ((1 << f) - 1) for q in qs]
    return d, [v % k for v in d], bad


def answer(sk, kappa, ib, k, m, Ps, rho_es, only=None):
    """Bob: (E {(q, t): [[ [t == j_q] ]] freshly randomized}, d [m], j [m], bad); `only`: the (q, t) to encrypt (None: all of them)."""
    d, j, bad = split(kappa, ib, k, m, sk.n.bit_length(), [dec(sk, P) for P in Ps])
    want = [(q, t) for q in range(m) for t in range(k)] if only is None else only
    return {(q, t): enc(sk, 1 if t == j[q] else 0, rho_es[q][t]) for q, t in want}, d, j, bad


def rotate(E, rot, k, m):
    """out[q][t] = E[q][(t + rot_q) mod k] for rows E [m][k]."""
    return [[E[q][(t + rot[q]) % k] for t in range(k)] for q in range(m)]


def onehot_enc(sk, kappa, ib, k, i_cs, draws):
    """The whole protocol on ciphertexts: out [m][k]."""
    rs, rho_ps, rho_es = draws
    m = len(i_cs)
    Ps = pack(sk, kappa, ib, k, i_cs, rs, rho_ps)
    E, _, _, bad = answer(sk, kappa, ib, k, m, Ps, rho_es)
    assert not bad
    _, rot = plain(kappa, ib, k, m, sk.n.bit_length(), rs)
    return rotate([[E[(q, t)] for t in range(k)] for q in range(m)], rot, k, m)


def onehot(sk, idx, k, ib, rng, kappa=40, draws=None):
    """Plaintext indices in, the decrypted planes [m][k] out, through the protocol."""
    n = sk.n
    i_cs = [enc(sk, i, rng.randrange(1, n)) for i in idx]
    draws = draws if draws is not None else draw(rng, kappa, ib, k, len(idx), n)
    return [[dec(sk, c) for c in row] for row in onehot_enc(sk, kappa, ib, k, i_cs, draws)]


if __name__ == "__main__":      # pragma: no cover
    from oracle import sc_oracle as o

    sk = o.PaillierKey.generate(512, random.Random(1))
    print(onehot(sk, [0, 2, 6], 5, 3, random.Random(2)))

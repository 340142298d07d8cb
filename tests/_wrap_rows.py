"""Whole comparisons as data, at the rows a uniform draw of r never reaches: the region where the blinded sum
2^l + r + y - x wraps around N.  A row is (x, y, r, delta_a) for a given (N, l); every condition below is derived from the row alone.

Pure Python (no torch, nothing from the package under test, no oracle): tests/test_wrap_rows_cpu.py holds the table against the
oracle and the stand-in engine on a machine without a GPU, tests/test_gpu_wrap_rows.py runs it through the library.

The decision table of the protocol (steps as in oracle/sc_oracle.py), with half = (N - 1) // 2, T = 2^l + r + y - x (an integer,
0 < T < N + 2^(l+1)) and z = T mod N:

    rsmall = [r < half]   d = [z < half]
       1          1        no wrap (T < half + 2^(l+1) < N); step 4c replaces [d] by [0]; zeta_1
       1          0        the same, r just below half
       0          0        no wrap (a wrapped z is below 2^(l+1) < half); [d] = Enc(0); zeta_2 = z >> l
       0          1        THE WRAP CELL: T >= N (an unwrapped z would be >= r >= half), r in [N - 2^(l+1), N); [d] = Enc(1) survives
                           step 4c, alpha~ = (r - N) mod 2^l decides, w_i in {-1, 0, 1}, zeta_2 = (z + N) >> l

Outside the wrap cell the steps compute [x <= y] = (T >> l) - (r >> l) - [T mod 2^l < r mod 2^l] literally, and the result is right
for every row.  Inside it, with n0 = N mod 2^l, beta = z mod 2^l, alpha = r mod 2^l and alpha~ = (alpha - n0) mod 2^l:

* zeta_2 = (z + N) >> l = T >> l is right, and the bit still owed is t = [T mod 2^l < alpha] = [(beta + n0) mod 2^l < alpha];
* steps 4d-4j decide [beta < alpha~] instead.  The two agree when the carries c_beta = [beta + n0 >= 2^l] and
  c_alpha = [alpha~ + n0 >= 2^l] agree (add n0 to both sides; both overflow or neither does).  When c_beta = 1 and c_alpha = 0,
  (beta + n0) mod 2^l < n0 <= alpha while beta >= 2^l - n0 > alpha~: t = 1 but [beta < alpha~] = 0; when c_beta = 0 and
  c_alpha = 1 the other way round.  So t = [beta < alpha~] xor [c_beta != c_alpha];
* w_i = alpha_i xor beta_i - d is -(alpha~_i xor beta_i) where alpha_i != alpha~_i: the sum over 2^j w_j keeps its highest non-zero
  term's magnitude, so c_i for i >= 0 is zero exactly where it should be (|3 sum| >= 6 > |s + alpha~_i - beta_i|, and
  |c_i| < 3 2^l < u).  But c_{-1} = delta_a + sum 2^j w_j is zero also when delta_a = 1 and the sum is -1.  N is odd, so
  alpha_0 != alpha~_0 always and w_0 is 0 or -1, never +1: the sum is -1 exactly when alpha~ and beta differ at bit 0 alone with
  w_0 = -1.  With alpha~ > beta that row has delta_B = 1 anyway; with beta = alpha~ + 1 (alpha~ even) delta_B = 1 is wrong.  Call
  that the `glitch`: delta_a = 1, beta = alpha~ + 1, alpha~ even; it needs y - x = 1 (mod 2^l);
* so the comparison's plaintext is [x <= y] + t - ([beta < alpha~] xor glitch), see protocol_value: 0 or 1 where both faults
  cancel or neither occurs, and otherwise the complement OR a value that is no bit at all (2, or -1 = N - 1).

A row is wrong only if r is one of the 2^(l+1) values below N, so a uniform r gives a wrong result with probability below
2^(l+1) / N (2^-1006 for l = 16 and a 1024-bit N).
"""
from __future__ import annotations

import collections
import functools
import itertools

Row = collections.namedtuple("Row", "x y r delta_a")
Cond = collections.namedtuple("Cond", "rsmall d wrap le eq far c_beta c_alpha any_diff all_diff top_diff delta_a glitch edges")

R_EDGES = ("r=0", "r=1", "r=half-1", "r=half", "r=half+1", "r=N-2", "r=N-1", "r=N-2^l", "r=N-2^(l+1)-1", "r=N-2^(l+1)", "r=N-2^(l+1)+1")
Z_EDGES = ("z=0", "z=1", "z=2^l-1", "z=2^l", "z=half-1", "z=half", "z=half+1", "z=N-1")


def half_of(n: int) -> int:
    return (n - 1) // 2


def r_edges(n: int, l: int) -> dict:
    """name -> r for the boundaries of r that lie in [0, N)."""
    h, p = half_of(n), 1 << l
    vals = (0, 1, h - 1, h, h + 1, n - 2, n - 1, n - p, n - 2 * p - 1, n - 2 * p, n - 2 * p + 1)
    return {name: v for name, v in zip(R_EDGES, vals) if 0 <= v < n}


def z_edges(n: int, l: int) -> dict:
    h, p = half_of(n), 1 << l
    vals = (0, 1, p - 1, p, h - 1, h, h + 1, n - 1)
    return {name: v for name, v in zip(Z_EDGES, vals) if 0 <= v < n}


def plain(n: int, l: int, row: Row):
    """(z, beta, alpha, alpha~, n0) of a row, from the definitions."""
    p = 1 << l
    z = (p + row.r + row.y - row.x) % n
    return z, z % p, row.r % p, (row.r - n) % p, n % p


def conditions(n: int, l: int, row: Row) -> Cond:
    h, p = half_of(n), 1 << l
    z, beta, alpha, at, n0 = plain(n, l, row)
    rsmall, d = int(row.r < h), int(z < h)
    diff = alpha ^ at
    edges = tuple(name for name, v in r_edges(n, l).items() if v == row.r) + tuple(name for name, v in z_edges(n, l).items() if v == z)
    return Cond(rsmall=rsmall, d=d, wrap=int(not rsmall and d), le=int(row.x <= row.y), eq=int(row.x == row.y),
                far=int(abs(row.x - row.y) == p - 1), c_beta=int(beta + n0 >= p), c_alpha=int(at + n0 >= p),
                any_diff=int(diff != 0), all_diff=int(diff == p - 1), top_diff=int(at != beta), delta_a=row.delta_a,
                glitch=int(row.delta_a == 1 and at % 2 == 0 and beta == at + 1), edges=edges)


def cross_name(wrap, c_beta, c_alpha, delta_a, le) -> str:
    return f"wrap={wrap} c_beta={c_beta} c_alpha={c_alpha} delta_a={delta_a} x<=y={le}"


def condition_names(n: int, l: int, row: Row) -> tuple:
    """The named conditions a row meets (the unit the promise below is stated in)."""
    c = conditions(n, l, row)
    names = [cross_name(c.wrap, c.c_beta, c.c_alpha, c.delta_a, c.le), f"rsmall={c.rsmall} d={c.d}"]
    names += list(c.edges)
    if c.eq:
        names.append(f"x == y, wrap={c.wrap}")
    if c.far:
        names.append(f"|x - y| = 2^l - 1, wrap={c.wrap} x<=y={c.le}")
    names.append(f"wrap={c.wrap}: " + ("every alpha_i differs from alpha~_i" if c.all_diff else "some alpha_i differ from alpha~_i"))
    names.append(f"wrap={c.wrap}: " + ("alpha~ and beta differ somewhere" if c.top_diff else "alpha~ equals beta"))
    if c.wrap and c.glitch:
        names.append("wrap=1: c_-1 is zero through w_0 = -1 although beta > alpha~ (the glitch)")
    return tuple(names)


# ---- the prediction, from the analysis in the module's docstring (never from running a comparison)
def protocol_value(n: int, l: int, row: Row) -> int:
    """The plaintext (mod N) that the restated protocol's result decrypts to."""
    c = conditions(n, l, row)
    if not c.wrap:
        return c.le
    _, beta, _, at, _ = plain(n, l, row)
    decided = int(beta < at) ^ c.glitch                 # what steps 4d-4j and 6 hand to step 7
    owed = int(beta < at) ^ int(c.c_beta != c.c_alpha)    # [T mod 2^l < alpha]
    return (c.le + owed - decided) % n


def protocol_is_right(n: int, l: int, row: Row) -> bool:
    """Whether the restated protocol returns [x <= y] on this row: outside the wrap cell always; inside it when the carries agree
    and the glitch is absent, or when both faults occur and cancel."""
    c = conditions(n, l, row)
    return not c.wrap or (c.c_beta != c.c_alpha) == bool(c.glitch)


# ---- the rows
def values(l: int) -> tuple:
    top, mid = (1 << l) - 1, 1 << (l - 1)
    vals = {0, 1, top, mid - 1, mid, mid + 1}
    if l > 64:                                            # the 64-bit word edges of the flag rows
        vals |= {(1 << 64) - 1, 1 << 64}
    return tuple(sorted(v for v in vals if 0 <= v <= top))


def pairs(l: int) -> tuple:
    """(x, y): equal pairs, adjacent pairs in both orders, and the two pairs 2^l - 1 apart, over 0, 1, 2^(l-1) and its neighbours,
    2^l - 1 (and the 64-bit word edges for l > 64)."""
    vals, top = values(l), (1 << l) - 1
    out = [(v, v) for v in vals]
    for v in vals:
        if v + 1 <= top:
            out += [(v, v + 1), (v + 1, v)]
    out += [(0, top), (top, 0)]
    return tuple(dict.fromkeys(out))


def _low_targets(n: int, l: int) -> tuple:
    """Values of alpha~ or beta on either side of the carry threshold 2^l - n0, at the ends of the range, and the alpha~ for which
    every bit of alpha differs from alpha~ (alpha + alpha~ = 2^l - 1)."""
    p, n0 = 1 << l, n % (1 << l)
    return tuple(dict.fromkeys(v % p for v in (0, p - n0 - 1, p - n0, p - 1, (p - 1 - n0) // 2)))


def planted_r(n: int, l: int, x: int, y: int) -> tuple:
    """The r planted for one pair: the boundaries of r, the r that put z on its boundaries, r = N - k for the k that put alpha~ or
    beta on the targets above (k and k + 2^l: both halves of the wrap region), and the same low parts far from every boundary, on
    either side of half."""
    p, h, dlt = 1 << l, half_of(n), y - x
    out = list(r_edges(n, l).values())
    out += [(zt - p - dlt) % n for zt in z_edges(n, l).values()]
    for a in _low_targets(n, l):
        for k0 in ((-a) % p, (dlt - a) % p):
            out += [n - k for k in (k0, k0 + p) if 1 <= k <= 2 * p]
    for base, pick in ((h >> 1, 0), (h + (h >> 1), 1)):
        for a in _low_targets(n, l):
            out.append(((base >> l) << l) | ((a + n) % p, (a - p - dlt) % p)[pick])
    return tuple(dict.fromkeys(r for r in out if 0 <= r < n))


@functools.lru_cache(maxsize=None)
def rows(n: int, l: int) -> tuple:
    """Every row of the table for (N, l), in a fixed order."""
    return tuple(Row(x, y, r, da) for x, y in pairs(l) for r in planted_r(n, l, x, y) for da in (0, 1))


def reached(n: int, l: int, table) -> frozenset:
    return frozenset(name for row in table for name in condition_names(n, l, row))


def wrong_rows(n: int, l: int, table=None) -> tuple:
    return tuple(row for row in (rows(n, l) if table is None else table) if not protocol_is_right(n, l, row))


@functools.lru_cache(maxsize=None)
def cover(n: int, l: int, limit: int = 40, skip: int = 0) -> tuple:
    """At most `limit` rows of the table that still reach every named condition, chosen greedily (most conditions not yet reached
    first; a row the protocol gets wrong, then a row of the wrap cell, wins a tie; then table order).  `skip` rotates the table
    first, so that different cases run different rows.  What is left of `limit` goes to rows the protocol gets wrong."""
    table = rows(n, l)
    table = table[skip % len(table):] + table[:skip % len(table)]
    names = {row: frozenset(condition_names(n, l, row)) for row in table}
    rank = {row: (not protocol_is_right(n, l, row), conditions(n, l, row).wrap) for row in table}
    missing, out = set(reached(n, l, table)), []
    while missing:
        best = max(table, key=lambda row: (len(names[row] & missing),) + rank[row])
        out.append(best)
        missing -= names[best]
    if len(out) > limit:
        raise ValueError(f"{len(out)} rows are needed to reach every condition, {limit} allowed")
    spare = [row for row in wrong_rows(n, l, table) if row not in out]
    return tuple(out + spare[:limit - len(out)])


# ---- the promise
def promised(n: int, l: int) -> tuple:
    """The named conditions the table reaches for l = 1 and for l >= 5 (with 2^(l+2) < half), written down from the analysis, not
    from the rows.

    The cross wrap x c_beta x c_alpha x delta_a x [x <= y] is full but for what cannot exist:
    * wrap, x > y, c_beta = 1, c_alpha = 0: with x > y a wrapped z = 2^l - (x - y) - k is below 2^l, so beta = z = alpha~ - (x - y)
      < alpha~, and c_beta = 1 would put beta >= 2^l - n0 > alpha~;
    * l = 1 (n0 = 1, a carry is the bit itself): without a wrap and with x > y, (x, y) = (1, 0) and beta = alpha~ = 1 - alpha, so the
      carries agree; with a wrap and x > y, k = 1 alone keeps z >= 0: alpha~ = 1, beta = 0.
    `alpha~ equals beta` without a wrap needs y - x = -n0 (mod 2^l), which no pair of the table has but (1, 0) at l = 1; and at l = 1
    alpha_0 != alpha~_0 is every bit."""
    if not (l == 1 or l >= 5) or (1 << (l + 2)) >= half_of(n):
        raise ValueError("the promise is stated for l = 1 and l >= 5")
    names = [f"rsmall={a} d={b}" for a in (1, 0) for b in (1, 0)]
    for wrap, cb, ca, da, le in itertools.product((0, 1), repeat=5):
        if wrap and not le and cb and not ca:
            continue
        if l == 1 and not le and ((not wrap and cb != ca) or (wrap and (cb, ca) != (0, 1))):
            continue
        names.append(cross_name(wrap, cb, ca, da, le))
    names += list(r_edges(n, l)) + list(z_edges(n, l))
    names += [f"x == y, wrap={w}" for w in (0, 1)]
    names += [f"|x - y| = 2^l - 1, wrap={w} x<=y={le}" for w in (0, 1) for le in (0, 1)]
    for w in (0, 1):
        names += [f"wrap={w}: every alpha_i differs from alpha~_i", f"wrap={w}: alpha~ and beta differ somewhere"]
        if l > 1:
            names.append(f"wrap={w}: some alpha_i differ from alpha~_i")
        if w or l == 1:
            names.append(f"wrap={w}: alpha~ equals beta")
    names.append("wrap=1: c_-1 is zero through w_0 = -1 although beta > alpha~ (the glitch)")
    return tuple(names)



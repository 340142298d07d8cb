"""The draw layer restated: which generator call feeds which random input of the comparison, the selection and the multiplication,
and how a compare-exchange, a tournament, a sort, a top-m, an equality and an interval test string those calls together.

Independent of the package (it is never imported here): the generator is oracle/chacha_rng.py, the protocol steps are the pure-Python
models next to this file, and the order of the calls is written from the docstrings of include/sc_amd.h (sc_rng_*), batch.py,
selection.py, sorting.py and multiplication.py.  Every item of a generator call has its own keystream, so the draws of a few sampled
rows of a large batch are cheap to restate: every function takes the sampled `rows` and the batch's `count`.

Keys are oracle/sc_oracle.py PaillierKey / DGKKey objects.  No torch.
"""
from __future__ import annotations

import dataclasses

import _mult_model as mm
import _select_model as sm
import _sort_model as som
from oracle import chacha_rng as cr
from oracle import sc_oracle as o


class Replay:
    """One engine's generator: a key and the number of the next call.  Every method returns the values of the chosen items of the
    current call and advances the counter by one, the way sc_rng_bits / _below / _coins / _permutations number their calls.  `log`
    keeps (kind, bits or n or k, count, nonzero) per call."""

    def __init__(self, key: bytes) -> None:
        self.key, self.call, self.log = bytes(key), 0, []

    def _next(self, kind, arg, count, nonzero=False) -> int:
        self.log.append((kind, arg, count, bool(nonzero)))
        self.call += 1
        return self.call - 1

    def bits(self, bits, count, items):
        return cr.rng_bits(self.key, self._next("bits", bits, count), bits, count, items=list(items))

    def below(self, n, count, nonzero, items):
        return cr.rng_below(self.key, self._next("below", n, count, nonzero), n, count, nonzero, items=list(items))

    def coins(self, count, items):
        return cr.rng_coins(self.key, self._next("coins", None, count), count, items=list(items))

    def perms(self, k, count, items):
        return cr.rng_permutations(self.key, self._next("perms", k, count), k, count, items=list(items))


def _chunks(flat, size):
    return [flat[i * size:(i + 1) * size] for i in range(len(flat) // size)] if size else []


# ---- the three draw helpers ---------------------------------------------------------------------------------------------------------
def comparison(rp: Replay, rows, count, l, n, u, rbits, alice=True, bob=True) -> list:
    """The draws of the sampled rows of one comparison batch of `count` rows as oracle Draws (the other player's fields None).
    Alice, six calls: r below N; the coins; the (l + 1) count blinding exponents in [1, u), plane-major (plane i of row b is item
    i count + b); the shuffles of l + 1 positions; rho_z in [1, N); the (l + 1) count randomizer exponents of the sent [c_i], plane-major,
    `rbits` bits.  Bob, two calls: his 3 count Paillier randomizer bases in [1, N) -- zeta_1, zeta_2, delta_B of row b are items b,
    count + b, 2 count + b -- and the (l + 1) count randomizer exponents of [d], [beta_i], plane-major.
    The library randomizes c_j with exponent j before the shuffle, the oracle output k after it: r_c[k] = r_alice[perm[k]]."""
    rows, lp1 = list(rows), l + 1
    planes = [i * count + b for b in rows for i in range(lp1)]
    r = delta_a = rhos = perms = rho_z = r_c = rho3 = r_bob = [None] * len(rows)
    if alice:
        r = rp.below(n, count, False, rows)
        delta_a = rp.coins(count, rows)
        rhos = _chunks(rp.below(u, lp1 * count, True, planes), lp1)
        perms = rp.perms(lp1, count, rows)
        rho_z = rp.below(n, count, True, rows)
        r_alice = _chunks(rp.bits(rbits, lp1 * count, planes), lp1)
        r_c = [[ra[src] for src in pm] for ra, pm in zip(r_alice, perms)]
    if bob:
        rho3 = _chunks(rp.below(n, 3 * count, True, [t * count + b for b in rows for t in range(3)]), 3)
        r_bob = _chunks(rp.bits(rbits, lp1 * count, planes), lp1)
    out = []
    for k in range(len(rows)):
        z = rho3[k] or (None, None, None)
        out.append(o.Draws(r=r[k], delta_a=delta_a[k], rhos=rhos[k], perm=perms[k], rho_z=rho_z[k], r_d=r_bob[k] and r_bob[k][0],
                           r_beta=r_bob[k] and r_bob[k][1:], r_c=r_c[k], rho_zeta1=z[0], rho_zeta2=z[1], rho_delta_b=z[2]))
    return out


def merge_comparison(a, b):
    """Alice's half and Bob's half of the same rows as whole Draws."""
    return [dataclasses.replace(x, r_d=y.r_d, r_beta=y.r_beta, rho_zeta1=y.rho_zeta1, rho_zeta2=y.rho_zeta2, rho_delta_b=y.rho_delta_b)
            for x, y in zip(a, b)]


def _packed(rp, rows, count, a_bits, col_bits, n, alice, bob):
    """Alice: r_a, one call per column, rho_p in [1, N); Bob: the nf count randomizer bases of his products in [1, N), column-major
    (column j of row b is item j count + b).  Per row (r_a, [r_b_j], rho_p, [rho_j]), a missing half None."""
    rows, nf = list(rows), len(col_bits)
    r_a = rho_p = [None] * len(rows)
    r_b = rho_q = [None] * len(rows)
    if alice:
        r_a = rp.bits(a_bits, count, rows)
        cols = [rp.bits(w, count, rows) for w in col_bits]
        r_b = [[c[k] for c in cols] for k in range(len(rows))]
        rho_p = rp.below(n, count, True, rows)
    if bob:
        rho_q = _chunks(rp.below(n, nf * count, True, [j * count + b for b in rows for j in range(nf)]), nf)
    return [(r_a[k], r_b[k], rho_p[k], rho_q[k]) for k in range(len(rows))]


def selection(rp: Replay, rows, count, kappa, widths, n, alice=True, bob=True) -> list:
    """The draws of one selection batch as the tuples tests/_select_model.py takes: r_a of kappa bits, then column j's r_b of
    w_j + 1 + kappa bits, then rho_p; Bob's rhos."""
    return _packed(rp, rows, count, kappa, [w + 1 + kappa for w in widths], n, alice, bob)


def multiplication(rp: Replay, rows, count, kappa, wx, wy, n, alice=True, bob=True) -> list:
    """The draws of one multiplication batch as the tuples tests/_mult_model.py takes: r_a of wx + kappa bits, then column j's r_b of
    wy_j + kappa bits, then rho_p; Bob's rhos."""
    return _packed(rp, rows, count, wx + kappa, [w + kappa for w in wy], n, alice, bob)


def merge_packed(a, b):
    return [(x[0], x[1], x[2], y[3]) for x, y in zip(a, b)]


# ---- the network of the sort ----------------------------------------------------------------------------------------------------------
def sort_layers(k):
    """_sort_model.comparators(k) grouped into the layers the players walk.  A layer is one stage (p, q) of the network: the merges of
    sorted blocks of p positions at stride q.  Comparator (i, j) has q = j - i, and the smallest aligned power-of-two block that holds
    both i and j has 2 p0 positions; the m-th time (m = 0, 1, ..) the sequential list names (i, j) it belongs to p = 2^m p0, since the
    recursion finishes the smaller merges of a position first.  The layers come by ascending p, then descending q, and inside a layer
    the comparators by ascending i."""
    groups, seen = {}, {}
    for i, j in som.comparators(k):
        m = seen.get((i, j), 0)
        seen[(i, j)] = m + 1
        groups.setdefault(((i ^ j).bit_length() + m, i - j), []).append((i, j))
    return [sorted(groups[key]) for key in sorted(groups)]


def cuts(total, max_rows):
    return [(a, min(a + max_rows, total)) for a in range(0, total, max_rows)]


# ---- whole operations -----------------------------------------------------------------------------------------------------------------
class Driver:
    """Walks whole operations with Alice's Replay `a` and Bob's `b` (the same object when both players share one engine: then every
    helper's calls are Alice's followed by Bob's) and returns the expected ciphertexts of the sampled rows together with `calls`, the
    counters (Alice's, Bob's) the operation ended on.  `wire` collects, per selection or multiplication exchange in order, the P and
    the product ciphertexts of the sampled rows: {"P": [..], "products": [[..per column] per row], "rows": [..]}."""

    def __init__(self, sk, dgk, l, rbits, key_a, key_b=None, kappa=40) -> None:
        self.sk, self.dgk, self.l, self.rbits, self.kappa = sk, dgk, l, rbits, kappa
        self.a = Replay(key_a)
        self.b = self.a if key_b is None else Replay(key_b)
        self.wire = []

    @property
    def calls(self):
        return self.a.call, self.b.call

    # -- draws of both players for one helper call
    def _cmp_draws(self, rows, count):
        n, u = self.sk.n, self.dgk.u
        a = comparison(self.a, rows, count, self.l, n, u, self.rbits, alice=True, bob=False)
        return merge_comparison(a, comparison(self.b, rows, count, self.l, n, u, self.rbits, alice=False, bob=True))

    def _sel_draws(self, rows, count, widths):
        a = selection(self.a, rows, count, self.kappa, widths, self.sk.n, alice=True, bob=False)
        return merge_packed(a, selection(self.b, rows, count, self.kappa, widths, self.sk.n, alice=False, bob=True))

    def _mul_draws(self, rows, count, wx, wy):
        a = multiplication(self.a, rows, count, self.kappa, wx, wy, self.sk.n, alice=True, bob=False)
        return merge_packed(a, multiplication(self.b, rows, count, self.kappa, wx, wy, self.sk.n, alice=False, bob=True))

    # -- the steps
    def compare(self, xs, ys, rows, count):
        """([[x <= y]], [[d]] = [[y - x + 2^l]]) of the sampled rows: the oracle's comparison, and Alice's [[z + r]] (1 - r N)."""
        n, n2 = self.sk.n, self.sk.n2
        out = []
        for x, y, dr in zip(xs, ys, self._cmp_draws(rows, count)):
            tr = {}
            delta = o.compare(x, y, self.l, self.sk, self.dgk, dr, True, tr)
            out.append((delta, tr["z_enc"] * (1 - dr.r * n) % n2))
        return [t[0] for t in out], [t[1] for t in out]

    def _select(self, widths, sigma, d_cols, b_cols, rows, count):
        """One selection exchange over the sampled rows: d_cols[j][i], b_cols[j][i] -> out[j][i]."""
        sk, nf = self.sk, len(widths)
        rec = {"P": [], "products": [], "rows": list(rows)}
        out = [[] for _ in widths]
        for i, dr in enumerate(self._sel_draws(rows, count, widths)):
            r_a, r_bs, rho_p, rhos = dr
            d_cs, b_cs = [d_cols[j][i] for j in range(nf)], [b_cols[j][i] for j in range(nf)]
            P = sm.pack(sk, self.kappa, widths, sigma[i], d_cs, r_a, r_bs, rho_p)
            prods, _, bad = sm.mult(sk, self.kappa, widths, P, rhos)
            assert not bad
            rec["P"].append(P)
            rec["products"].append(prods)
            for j, c in enumerate(sm.finish(sk, self.kappa, widths, sigma[i], d_cs, b_cs, prods, r_a, r_bs)):
                out[j].append(c)
        self.wire.append(rec)
        return out

    def compare_exchange(self, f_cols, g_cols, widths, rows, count):
        """(lo[j][i], hi[j][i]) of one compare-exchange batch: the comparison of the key columns, whose own [[d]] is the key column's
        difference, then the selection's draws."""
        delta, d_key = self.compare(f_cols[0], g_cols[0], rows, count)
        rec = {"P": [], "products": [], "rows": list(rows)}
        lo, hi = [[] for _ in widths], [[] for _ in widths]
        for i, dr in enumerate(self._sel_draws(rows, count, widths)):
            tr = {}
            lo_i, hi_i = som.compare_exchange(self.sk, self.kappa, widths, delta[i], [c[i] for c in f_cols], [c[i] for c in g_cols], dr,
                                              d_key=d_key[i], trace=tr)
            rec["P"].append(tr["P"])
            rec["products"].append(tr["products"])
            for j in range(len(widths)):
                lo[j].append(lo_i[j])
                hi[j].append(hi_i[j])
        self.wire.append(rec)
        return lo, hi

    def minmax(self, xs, ys, rows, count, want_max):
        """([[min or max]], [[x <= y]]): max = x + delta (y - x), min = x + (1 - delta)(y - x), [[1 - delta]] = (1 + N) [[delta]]^-1."""
        n, n2 = self.sk.n, self.sk.n2
        delta, d = self.compare(xs, ys, rows, count)
        sigma = delta if want_max else [(n + 1) * pow(c, -1, n2) % n2 for c in delta]
        return self._select([self.l], sigma, [d], [list(xs)], rows, count)[0], delta

    def argext(self, vals, B, rows, want_max):
        """vals[i][p]: the k ciphertexts of sampled row rows[i].  The tournament with the pairing of _select_model.argext: per round
        the pairs (2t, 2t + 1) of every row form one batch of h B rows, pair t of row b at item t B + b; the odd element is carried.
        min compares (L, R) and selects with [[1 - delta]]; max compares (R, L) and selects with delta; both keep L on ties.  The index
        column starts as the trivial encryptions 1 + p N."""
        n, n2, l = self.sk.n, self.sk.n2, self.l
        k = len(vals[0])
        wi = sm.index_bits(k)
        cur = [[(v, (1 + p * n) % n2) for p, v in enumerate(r)] for r in vals]
        while len(cur[0]) > 1:
            h = len(cur[0]) // 2
            items = [t * B + b for t in range(h) for b in rows]
            pairs = [(cur[i][2 * t], cur[i][2 * t + 1]) for t in range(h) for i in range(len(rows))]
            lv, li = [p[0][0] for p in pairs], [p[0][1] for p in pairs]
            rv, ri = [p[1][0] for p in pairs], [p[1][1] for p in pairs]
            shift = 1 + (1 << wi) * n
            if want_max:
                delta, d_v = self.compare(rv, lv, items, h * B)
                sigma = delta
                d_i = [a * pow(b, -1, n2) % n2 * shift % n2 for a, b in zip(li, ri)]
                base = [rv, ri]
            else:
                delta, d_v = self.compare(lv, rv, items, h * B)
                sigma = [(n + 1) * pow(c, -1, n2) % n2 for c in delta]
                d_i = [b * pow(a, -1, n2) % n2 * shift % n2 for a, b in zip(li, ri)]
                base = [lv, li]
            out = self._select([l, wi], sigma, [d_v, d_i], base, items, h * B)
            nxt = [[(out[0][t * len(rows) + i], out[1][t * len(rows) + i]) for t in range(h)] for i in range(len(rows))]
            for i in range(len(rows)):
                if len(cur[i]) % 2:
                    nxt[i].append(cur[i][-1])
            cur = nxt
        return [r[0][0] for r in cur], [r[0][1] for r in cur]

    def _network(self, table, B, layers, rows, widths, max_rows, reverse):
        """table[i][j][p]: column j, position p of sampled row rows[i], changed in place.  Per layer the B len(layer) comparisons are
        numbered t = c B + b (comparator c, row b) and cut into sub-batches of at most max_rows; every sub-batch is one comparison
        batch and one selection batch of its own calls, and comparison t of a sub-batch [a, stop) is item t - a.  reverse
        (descending / largest): F is the value at j and G the one at i.  lo goes to F's position and hi to G's where that
        position's keep flag is set."""
        nf = len(widths)
        where = {b: i for i, b in enumerate(rows)}
        for layer in layers:
            for a, stop in cuts(B * len(layer), max_rows):
                ts = [t for t in range(a, stop) if t % B in where]
                todo = []
                for t in ts:
                    i, j, keep_i, keep_j = (tuple(layer[t // B]) + (True, True))[:4]
                    (fp, fk), (gp, gk) = ((j, keep_j), (i, keep_i)) if reverse else ((i, keep_i), (j, keep_j))
                    todo.append((where[t % B], fp, fk, gp, gk))
                f_cols = [[table[r][c][fp] for r, fp, _, _, _ in todo] for c in range(nf)]
                g_cols = [[table[r][c][gp] for r, _, _, gp, _ in todo] for c in range(nf)]
                lo, hi = self.compare_exchange(f_cols, g_cols, widths, [t - a for t in ts], stop - a)
                for x, (r, fp, fk, gp, gk) in enumerate(todo):
                    for c in range(nf):
                        if fk:
                            table[r][c][fp] = lo[c][x]
                        if gk:
                            table[r][c][gp] = hi[c][x]
        return table

    def sort(self, table, B, k, rows, widths, max_rows, descending):
        return self._network(table, B, sort_layers(k), rows, widths, max_rows, descending)

    def topk(self, table, B, layers, rows, widths, max_rows, largest):
        """`layers`: comparators (i, j, keep_i, keep_j) on the conventions of tests/_topk_model.py; a dead output leaves its position
        as it was."""
        return self._network(table, B, layers, rows, widths, max_rows, largest)

    def multiply(self, xs, y_cols, rows, count, wx, wy, signed=False, bases=None, coef=1):
        """out[j][i] = base_j [[x y_j]]^coef of the sampled rows of one multiplication batch."""
        sk = self.sk
        rec = {"P": [], "products": [], "rows": list(rows)}
        out = [[] for _ in wy]
        for i, dr in enumerate(self._mul_draws(rows, count, wx, wy)):
            r_a, r_bs, rho_p, rhos = dr
            y_cs = [c[i] for c in y_cols]
            P = mm.pack(sk, self.kappa, wx, wy, signed, xs[i], y_cs, r_a, r_bs, rho_p)
            prods, _, bad = mm.mult(sk, self.kappa, wx, wy, P, rhos)
            assert not bad
            rec["P"].append(P)
            rec["products"].append(prods)
            res = mm.finish(sk, self.kappa, wx, wy, signed, xs[i], y_cs, prods, r_a, r_bs, None if bases is None else [c[i] for c in bases], coef)
            for j, c in enumerate(res):
                out[j].append(c)
        self.wire.append(rec)
        return out

    def bit_op(self, a_cs, b_cs, rows, count, op):
        """AND: [[a b]]; OR / XOR: [[a]] [[b]] [[a b]]^coef with coef -1 / -2."""
        coef = {"and": 1, "or": -1, "xor": -2}[op]
        bases = None if coef == 1 else [[a * b % self.sk.n2 for a, b in zip(a_cs, b_cs)]]
        return self.multiply(a_cs, [b_cs], rows, count, 1, [1], False, bases, coef)[0]

    def two_comparisons(self, lo, hi, rows, B):
        """One comparison batch of 2B rows, lo = first operands (top half then bottom half), so that sampled row b draws items b and
        B + b; then the AND's draws.  lo, hi: ([..top], [..bottom]).  Returns (and, top bits, bottom bits)."""
        items = list(rows) + [B + b for b in rows]
        d, _ = self.compare(lo[0] + lo[1], hi[0] + hi[1], items, 2 * B)
        top, bottom = d[:len(rows)], d[len(rows):]
        return self.bit_op(top, bottom, rows, B, "and"), top, bottom

    def equal(self, xs, ys, rows, B):
        """([[x == y]], [[x <= y]], [[y <= x]]): (x, y) stacked on (y, x)."""
        return self.two_comparisons((list(xs), list(ys)), (list(ys), list(xs)), rows, B)

    def in_range(self, xs, los, his, rows, B):
        """[[lo <= x <= hi]]: (lo, x) stacked on (x, hi)."""
        return self.two_comparisons((list(los), list(xs)), (list(xs), list(his)), rows, B)[0]

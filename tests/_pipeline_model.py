"""Pure-Python reference of the chains of tests/test_gpu_pipelines.py on plain integers: the data of every chain -- planted rows ahead of
seeded random ones -- the width every stage declares, and the plaintext every stage must decrypt to.  No torch, nothing of the package.

Where a result depends on the network's choice among equal keys the reference follows the network through the existing models:
_topk_model.apply over the layers the caller hands in (sorting.topk_network's), _sort_model.apply over _sort_model.comparators, and the
tournament's left-wins rule as _select_model.argext plays it.  Nothing is skipped for ties.

B = 12 rows everywhere, k <= 8 values per row, dims <= 4, and every comparison runs at l <= 16 (the golden DGK key's).
"""
from __future__ import annotations

import random

import _sort_model as sort_model
import _topk_model as topk_model

B = 12


def bits_of(v: int) -> int:
    return max(1, int(v).bit_length())


def index_bits(k: int) -> int:
    return max(1, (k - 1).bit_length())


def first_diff(got, want):
    """The first row at which two flat lists differ, or None."""
    if len(got) != len(want):
        return min(len(got), len(want))
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


def arg_tournament(values, want_max=False):
    """(value, index) of the package's tournament: pairs (2t, 2t + 1), the odd element carried over, the left one wins a tie -- which is
    the lowest index."""
    cur = [(v, i) for i, v in enumerate(values)]
    while len(cur) > 1:
        nxt = []
        for t in range(len(cur) // 2):
            left, right = cur[2 * t], cur[2 * t + 1]
            nxt.append(left if (right[0] <= left[0] if want_max else left[0] <= right[0]) else right)
        if len(cur) % 2:
            nxt.append(cur[-1])
        cur = nxt
    return cur[0]


# ---- chains 1, 2 and 7: squared distance -> top-m with labels -> majority; -> argmin / argmax -> lookup / gather ------------------------
class Knn:
    """B queries, each with its own k points (the library takes one row per (query, point) pair, so a planted query brings the points
    that make its distances what the row is about) and one label per point."""
    dims, bits, k, m, classes = 4, 7, 8, 3, 4
    l = 2 * bits + bits_of(dims - 1)                    # the example's rule: a squared distance is below dims 2^(2 bits)
    label_bits = bits_of(classes - 1)
    top = (1 << bits) - 1

    # (name, q, points, labels); `a` on the first axis from the origin is the distance a^2
    @classmethod
    def _axis(cls, a):
        return [[v, 0, 0, 0] for v in a]

    @classmethod
    def planted(cls):
        z, t = [0] * 4, [cls.top] * 4
        return [
            ("all coordinates 0: eight distances 0", z, [z] * 8, [1, 0, 2, 1, 0, 3, 2, 1]),
            ("all coordinates 2^bits - 1 against 0: eight distances at the top of l, everyone in class 3", t, [z] * 8, [3] * 8),
            ("two equal distances straddle the cut (9 at positions 1 and 5) and decide the class", z,
             cls._axis([5, 3, 1, 6, 2, 3, 7, 8]), [3, 0, 0, 2, 1, 1, 2, 3]),
            ("three equal distances straddle the cut (9 at positions 0, 3, 5)", z, cls._axis([3, 4, 1, 3, 6, 3, 7, 8]), [0, 3, 2, 1, 3, 2, 0, 1]),
            ("all eight distances 25 from eight different points", z,
             [[5, 0, 0, 0], [3, 4, 0, 0], [0, 5, 0, 0], [4, 3, 0, 0], [0, 0, 5, 0], [0, 3, 4, 0], [0, 0, 0, 5], [0, 0, 3, 4]], [0, 1, 2, 3, 0, 1, 2, 3]),
            ("the three nearest carry classes 2, 1, 3: a tie the lowest class wins; nobody has class 0", z,
             cls._axis([9, 1, 2, 8, 3, 7, 6, 5]), [1, 2, 1, 3, 3, 2, 1, 2]),
            ("argmin at position k - 1, the largest distance twice (positions 0 and 3)", z, cls._axis([8, 3, 4, 8, 5, 6, 2, 1]), [0, 1, 2, 3, 3, 2, 1, 0]),
            ("argmin at position 0, the same distance again at position 5", z, cls._axis([1, 3, 4, 2, 5, 1, 7, 8]), [2, 0, 1, 3, 0, 1, 3, 2]),
            ("one distance at the top of l (position 0) among small ones", t, [z] + [[cls.top - i, cls.top, cls.top, cls.top] for i in range(1, 8)],
             [0, 3, 3, 1, 2, 0, 1, 2]),
        ]

    def __init__(self, seed="pipelines:knn"):
        rng = random.Random(seed)
        rows = [(q, p, lab) for _, q, p, lab in self.planted()]
        while len(rows) < B:
            rows.append(([rng.getrandbits(self.bits) for _ in range(self.dims)],
                         [[rng.getrandbits(self.bits) for _ in range(self.dims)] for _ in range(self.k)],
                         [rng.randrange(self.classes) for _ in range(self.k)]))
        self.q = [r[0] for r in rows]
        self.p = [r[1] for r in rows]
        self.label = [r[2] for r in rows]
        assert len(rows) == B and all(len(p) == self.k and len(lab) == self.k for _, p, lab in rows)

    # the library's layout: row b k + t is the pair (query b, point t); plane j holds coordinate j of every row
    def x_planes(self):
        return [[self.q[r // self.k][j] for r in range(B * self.k)] for j in range(self.dims)]

    def y_planes(self):
        return [[self.p[r // self.k][r % self.k][j] for r in range(B * self.k)] for j in range(self.dims)]

    def label_rows(self):
        return [self.label[r // self.k][r % self.k] for r in range(B * self.k)]

    def table(self):
        """[k][B]: entry t of row b's table is the label of its point t."""
        return [[self.label[b][t] for b in range(B)] for t in range(self.k)]

    def distances(self):
        """[B][k]."""
        return [[sum((a - c) ** 2 for a, c in zip(self.q[b], pt)) for pt in self.p[b]] for b in range(B)]

    def nearest(self, layers):
        """The m (distance, label) pairs the network leaves in positions 0 .. m - 1 of every row: [B][m]."""
        d = self.distances()
        rows = [[(d[b][t], self.label[b][t]) for t in range(self.k)] for b in range(B)]
        return [[tuple(t) for t in r[:self.m]] for r in topk_model.apply(layers, rows)]

    def votes(self, layers):
        """[m][B]: the payload column transposed, as the majority takes it."""
        near = self.nearest(layers)
        return [[near[b][i][1] for b in range(B)] for i in range(self.m)]

    def majority(self, layers):
        """([class], [count]) per row; the argmax over the counts keeps the lowest class on a tie."""
        votes = self.votes(layers)
        out = []
        for b in range(B):
            tally = [sum(1 for i in range(self.m) if votes[i][b] == c) for c in range(self.classes)]
            cnt, cls = arg_tournament(tally, want_max=True)
            out.append((cls, cnt))
        return [c for c, _ in out], [n for _, n in out]

    def argmin(self):
        return [arg_tournament(r) for r in self.distances()]                    # (value, index)

    def argmax(self):
        return [arg_tournament(r, want_max=True) for r in self.distances()]

    def looked_up(self):
        return [self.label[b][i] for b, (_, i) in enumerate(self.argmin())]

    def gathered(self):
        """[2][B]: the label at the argmin and the label at the argmax."""
        return [self.looked_up(), [self.label[b][i] for b, (_, i) in enumerate(self.argmax())]]


# ---- chain 3: linear map -> offset -> argmax --------------------------------------------------------------------------------------------
class Linear:
    """K = 4 feature planes of `bits` bits, feature 3 a copy of feature 2 in every row, so that the weights +-(2^64 - 1) of row 3 cancel
    and its score stays inside l; J = 5 classes.  reach bounds |score|: the largest sum_k |W[j][k]| (2^bits - 1) + |b_j| over the rows, the
    pair on the copied feature counted by its net weight.  The offset is reach and l = bits(2 reach), as the example chooses them."""
    bits, K, J = 3, 4, 5
    M = (1 << 64) - 1
    W = [[0, 0, 0, 0],                  # the zero row: its output is the bare 1 + b N
         [0, 1, 0, 0],                  # a unit row
         [4, -1, 1, 0],
         [1, 0, M, -M],
         [-4, -2, -1, 0]]               # reaches -reach at x = (7, 7, 7, .)
    bias = [-10, -11, -9, -10, -8]      # at x = (0, 1, 0, 0) every score is -10
    top = (1 << bits) - 1

    PLANTED = [("all coordinates 0: the scores are the biases", [0, 0, 0, 0]),
               ("all coordinates 2^bits - 1: row 4 scores exactly -reach, the offset's lower bound", [7, 7, 7, 7]),
               ("every score equal (-10): the argmax keeps class 0", [0, 1, 0, 0]),
               ("the largest score there is (26 in class 2): the top bit of l", [7, 0, 7, 7])]

    def __init__(self, seed="pipelines:linear"):
        rng = random.Random(seed)
        rows = [list(x) for _, x in self.PLANTED]
        while len(rows) < B:
            x = [rng.getrandbits(self.bits) for _ in range(3)]
            rows.append(x + [x[2]])
        self.x = rows                                                           # [B][K]
        assert all(r[3] == r[2] for r in rows)

    @classmethod
    def net_weights(cls):
        return [[w[0], w[1], w[2] + w[3]] for w in cls.W]

    @classmethod
    def reach(cls):
        return max(sum(abs(v) for v in w) * cls.top + abs(b) for w, b in zip(cls.net_weights(), cls.bias))

    @classmethod
    def l(cls):
        return bits_of(2 * cls.reach())

    @classmethod
    def x_bits(cls, nbits):
        """The largest declared input width the fit rule admits: bits(sum_k |W[j][k]|) + x_bits + 1 < nbits - 1 on every row."""
        return nbits - 1 - 1 - max(bits_of(sum(abs(v) for v in w)) for w in cls.W) - 1

    def planes(self):
        return [[self.x[b][k] for b in range(B)] for k in range(self.K)]

    def scores(self):
        """[J][B], signed."""
        return [[sum(w * v for w, v in zip(self.W[j], self.x[b])) + self.bias[j] for b in range(B)] for j in range(self.J)]

    def shifted(self):
        r = self.reach()
        return [[v + r for v in row] for row in self.scores()]

    def best(self):
        s = self.shifted()
        return [arg_tournament([s[j][b] for j in range(self.J)], want_max=True) for b in range(B)]     # (value, label)


# ---- chain 4: histogram -> running sum -> quantile ---------------------------------------------------------------------------------------
class Histogram:
    """m = 5 indices per row of index_bits(k) + 1 bits, so that an index at or above k exists and counts at i mod k."""
    m = 5

    def __init__(self, k, seed="pipelines:histogram"):
        self.k = k
        self.ib = index_bits(k) + 1
        rng = random.Random(f"{seed}:{k}")
        cols = [[0] * self.m,                                                     # all in bin 0
                [k - 1] * self.m,                                                 # all in bin k - 1
                [k + (k - 1), 0, k, k - 1, 0][:self.m],                           # indices at or above k: counted at i mod k
                [0, k - 1, 0, k - 1, 0]]                                          # only the two end bins
        while len(cols) < B:
            cols.append([rng.getrandbits(self.ib) for _ in range(self.m)])
        assert all(v < (1 << self.ib) for c in cols for v in c)
        self.idx = [[cols[b][q] for b in range(B)] for q in range(self.m)]       # [m][B]
        self.ranks = [b % self.m for b in range(B)]                               # the encrypted per-row rank

    @property
    def l(self):
        return bits_of(self.m)                                                    # a count of at most m

    def hist(self):
        return [[sum(1 for q in range(self.m) if self.idx[q][b] % self.k == t) for b in range(B)] for t in range(self.k)]

    def cdf(self, exclusive=False):
        h = self.hist()
        return [[sum(h[tt][b] for tt in range(t + (0 if exclusive else 1))) for b in range(B)] for t in range(self.k)]

    def quantile(self, kth):
        """kth: an integer or one rank per row.  The bin of that rank among the binned values."""
        ranks = [kth] * B if isinstance(kth, int) else kth
        return [sorted(self.idx[q][b] % self.k for q in range(self.m))[ranks[b]] for b in range(B)]

    def bits_below(self, kth):
        """[k - 1][B]: [cdf_t <= kth], what the comparison batch of the quantile decrypts to."""
        ranks = [kth] * B if isinstance(kth, int) else kth
        c = self.cdf()
        return [[int(c[t][b] <= ranks[b]) for b in range(B)] for t in range(self.k - 1)]

    def kth_of_indices(self, kth):
        """The sorting-network route sorts the indices as they are, not binned: equal to quantile() on the rows below_k() names."""
        return [sorted(self.idx[q][b] for q in range(self.m))[kth] for b in range(B)]

    def below_k(self):
        return [b for b in range(B) if all(self.idx[q][b] < self.k for q in range(self.m))]


# ---- chain 5: group-by sum -> sort with the permutation -> gather by its first index ---------------------------------------------------
class Groupby:
    """G = 4 data sets of B rows (value, group) each, k = 4 groups, values of `bits` bits; the k sums of every set are one row of the sort
    (descending: the first index of the permutation is the group with the largest sum), l = bits + bits(B)."""
    G, k, bits, table_bits = 4, 4, 12, 5
    l = bits + bits_of(B)

    def __init__(self, seed="pipelines:groupby"):
        rng = random.Random(seed)
        top = (1 << self.bits) - 1
        self.ib = index_bits(self.k) + 1
        self.vals = [[top] * B,                                                   # every row in group k - 1 at the top: the largest sum l admits
                     [0] * B,                                                     # every sum 0: four equal keys
                     [rng.getrandbits(self.bits) for _ in range(B)],
                     [rng.getrandbits(self.bits) for _ in range(B)]]
        self.idx = [[self.k - 1] * B,
                    [rng.randrange(self.k) for _ in range(B)],
                    [rng.getrandbits(self.ib) for _ in range(B)],                 # groups at or above k: counted at i mod k
                    [rng.randrange(2) for _ in range(B)]]                         # groups 2 and 3 empty: two sums 0
        self.table = [[rng.getrandbits(self.table_bits) for _ in range(self.G)] for _ in range(self.k)]       # [k][G]
        self.table[0][0], self.table[self.k - 1][0] = 0, (1 << self.table_bits) - 1

    def sums(self):
        """[G][k]."""
        return [[sum(v for v, i in zip(self.vals[g], self.idx[g]) if i % self.k == t) for t in range(self.k)] for g in range(self.G)]

    def ranked(self):
        """([G][k] sorted sums, [G][k] permutation) as Batcher's network leaves them, descending."""
        rows = [[(s, t) for t, s in enumerate(r)] for r in self.sums()]
        out = sort_model.apply([[c] for c in sort_model.comparators(self.k)], rows, descending=True)
        return [[t[0] for t in r] for r in out], [[t[1] for t in r] for r in out]

    def first_label(self):
        return [self.table[perm[0]][g] for g, perm in enumerate(self.ranked()[1])]


# ---- chain 6: signed products -> segment sums -> offset -> interval and equality ------------------------------------------------------
class Arithmetic:
    """3 B signed pairs of xb bits, one sum per segment of 3 products (B sums), shifted by 2^(l - 1) into 0 .. 2^l - 1 and compared with
    encrypted constants.  l: |sum| <= 3 * 2^(2 xb - 2), so l = bits(3 * 2^(2 xb - 2)) + 1."""
    xb, seg = 4, 3
    lo_v, hi_v = -1 << (xb - 1), (1 << (xb - 1)) - 1
    l = bits_of(seg * lo_v * lo_v) + 1
    offset = 1 << (l - 1)
    range_lo, range_hi, equal_to = -56, 41, 0                                    # lo <= sum <= hi; sum == 0

    PLANTED = [[(-8, -8), (-8, -8), (-8, -8)],                                    # the most negative operand with itself, three times: 192
               [(-8, 7), (-8, 7), (7, -8)],                                       # the most negative sum: -168
               [(0, 5), (3, 4), (-3, 4)],                                         # a sum that is 0
               [(0, 0), (0, 0), (0, 0)],                                          # a sum of zeros
               [(-1, 1), (0, -8), (7, 0)],                                        # -1
               [(-8, 7), (0, 0), (0, 7)],                                         # exactly the interval's lower end
               [(6, 7), (-1, 1), (0, 3)]]                                         # exactly its upper end

    def __init__(self, seed="pipelines:arithmetic"):
        rng = random.Random(seed)
        segs = [list(s) for s in self.PLANTED]
        while len(segs) < B:
            segs.append([(rng.randint(self.lo_v, self.hi_v), rng.randint(self.lo_v, self.hi_v)) for _ in range(self.seg)])
        self.x = [p[0] for s in segs for p in s]                                  # [3 B]
        self.y = [p[1] for s in segs for p in s]

    def products(self):
        return [a * b for a, b in zip(self.x, self.y)]

    def sums(self):
        p = self.products()
        return [sum(p[i:i + self.seg]) for i in range(0, len(p), self.seg)]

    def shifted(self):
        return [s + self.offset for s in self.sums()]

    def in_range(self):
        return [int(self.range_lo <= s <= self.range_hi) for s in self.sums()]

    def equal(self):
        """([sum == c], [sum <= c], [c <= sum])."""
        s, c = self.sums(), self.equal_to
        return [int(v == c) for v in s], [int(v <= c) for v in s], [int(c <= v) for v in s]

"""The reference of the chained-family tests (tests/_pipeline_model.py) pinned without the library's arithmetic.

1. Every planted row against values written down by hand: distances, the m nearest, the class and its count, argmin and argmax with
   their ties, the looked-up labels; the linear scores, the offset and the label; histogram, running sum and quantiles; group sums, the
   order and the label of the first; products, segment sums, interval and equality.  Where equal keys meet a cut the literal is the
   network's choice (recorded from the model over sorting.topk_network and Batcher's network) and is checked to be a valid one.
2. Every width a stage declares -- l, payload_bits, index_bits, x_bits, the count's width -- is the smallest that admits the planted
   extreme: one bit less does not.  The GPU tests therefore sit on the boundary.
3. The stand-in engine: NO chain runs on tests/_oracle_engine.py.  Every chain goes through at least one scheme-level entry point the
   stand-in does not have (the inner product's, the selection's, the one-hot's, the multiplication's, the axis sum, scan and linear
   map), and the stand-in is not extended for this; test_no_chain_fits_the_stand_in_engine keeps this statement true.
"""
import os
import random
import sys

import pytest

from conftest import oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_model as PM  # noqa: E402
import _select_model as select_model  # noqa: E402

B = PM.B


def _fits(v, bits):
    return 0 <= v < (1 << bits)


def _smallest(bits, extreme):
    """`bits` admits the planted extreme and one bit less does not."""
    return _fits(extreme, bits) and not _fits(extreme, bits - 1)


def _layers(K):
    from protocols.secure_comparison_amd.sorting import topk_network

    return topk_network(K.k, K.m)


# ---- chains 1, 2, 7 -----------------------------------------------------------------------------------------------------------------------
def test_knn_planted_rows():
    K = PM.Knn()
    P = len(K.planted())
    assert P == 9 and (K.dims, K.bits, K.k, K.m, K.classes, K.l, K.label_bits) == (4, 7, 8, 3, 4, 16, 2)
    d = K.distances()
    assert d[:P] == [[0] * 8, [64516] * 8, [25, 9, 1, 36, 4, 9, 49, 64], [9, 16, 1, 9, 36, 9, 49, 64], [25] * 8,
                     [81, 1, 4, 64, 9, 49, 36, 25], [64, 9, 16, 64, 25, 36, 4, 1], [1, 9, 16, 4, 25, 1, 49, 64],
                     [64516, 1, 4, 9, 16, 25, 36, 49]]
    layers = _layers(K)
    near = K.nearest(layers)
    for b in range(B):                                             # every row: the right keys, and each label from a point at that distance
        assert [v for v, _ in near[b]] == sorted(d[b])[:K.m], b
        assert all(any(d[b][t] == v and K.label[b][t] == lab for t in range(K.k)) for v, lab in near[b]), b
    assert sorted(d[2])[K.m - 1] == sorted(d[2])[K.m] == 9                              # two equal distances straddle the cut
    assert sorted(d[3])[1:4] == [9, 9, 9] and sorted(d[4]) == [25] * 8                  # three; all eight
    # rows 1, 5, 6, 7, 8 do not depend on the network; rows 0, 2, 3, 4 are its choice among equal distances
    assert [t[1] for t in near[5]] == [2, 1, 3] and [t[1] for t in near[6]] == [0, 1, 1] and [t[1] for t in near[8]] == [3, 3, 1]
    assert sorted(t[1] for t in near[7]) == [1, 2, 3]
    assert near[2] == [(1, 0), (4, 1), (9, 0)] and near[3] == [(1, 2), (9, 1), (9, 0)]
    cls, cnt = K.majority(layers)
    assert cls[:P] == [0, 3, 0, 0, 0, 1, 1, 1, 3] and cnt[:P] == [1, 3, 2, 1, 1, 1, 2, 1, 2]
    assert cnt[1] == K.m and 0 not in K.label[5]                                        # a count of m; a class nobody has
    votes = K.votes(layers)
    assert len(votes) == K.m and len(votes[0]) == B and [votes[i][5] for i in range(K.m)] == [2, 1, 3]
    for b in range(B):                                             # the class against a plain tally of the model's own votes
        tally = [sum(1 for i in range(K.m) if votes[i][b] == c) for c in range(K.classes)]
        assert (cls[b], cnt[b]) == (tally.index(max(tally)), max(tally)), b


def test_nearest_label_planted_rows():
    K = PM.Knn()
    P = len(K.planted())
    assert K.argmin()[:P] == [(0, 0), (64516, 0), (1, 2), (1, 2), (25, 0), (1, 1), (1, 7), (1, 0), (1, 1)]
    assert K.argmax()[:P] == [(0, 0), (64516, 0), (64, 7), (64, 7), (25, 0), (81, 0), (64, 0), (64, 7), (64516, 0)]
    assert K.looked_up()[:P] == [1, 3, 0, 2, 0, 2, 0, 2, 3]
    assert K.gathered()[1][:P] == [1, 3, 3, 1, 0, 1, 0, 2, 0]
    d = K.distances()
    for b in range(B):                                             # ties go to the lowest index: list.index's rule
        assert K.argmin()[b] == (min(d[b]), d[b].index(min(d[b]))) and K.argmax()[b] == (max(d[b]), d[b].index(max(d[b]))), b
    assert K.table()[7][6] == K.label[6][7] and len(K.table()) == K.k and len(K.table()[0]) == B


def test_tournament_rule_is_the_selection_model_s(keys):
    """arg_tournament against _select_model.argext, which plays the tournament through the selection protocol, on the tied rows."""
    sk = oracle_paillier(keys, 1024)
    K = PM.Knn()
    d = K.distances()
    rng = random.Random("pipelines:tournament")
    for b, want_max in ((7, False), (6, True), (4, True)):         # the minimum twice, the maximum twice, all eight equal
        assert select_model.argext(sk, d[b], K.l, rng, want_max=want_max) == PM.arg_tournament(d[b], want_max=want_max)


def test_knn_widths_are_the_smallest():
    K = PM.Knn()
    assert _smallest(K.l, max(max(r) for r in K.distances())) and K.l == 2 * K.bits + (K.dims - 1).bit_length() <= 16
    assert _smallest(K.bits, max(v for q in K.q for v in q))
    assert _smallest(K.label_bits, max(max(r) for r in K.label))                        # payload_bits, the lookup's bits, index_bits
    assert _smallest(PM.index_bits(K.k), max(i for _, i in K.argmin()))                 # the lookup's default index width
    assert _smallest(PM.bits_of(K.m), max(K.majority(_layers(K))[1]))                   # the majority's l = bits(m)


# ---- chain 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_linear_planted_rows():
    L = PM.Linear()
    assert (L.reach(), L.l(), L.M) == (57, 7, 2 ** 64 - 1)
    s = L.scores()
    col = lambda b: [s[j][b] for j in range(L.J)]  # noqa: E731
    assert col(0) == L.bias == [-10, -11, -9, -10, -8]
    assert col(1) == [-10, -4, 19, -3, -57] and col(1)[4] == -L.reach()                 # exactly the offset's lower bound
    assert col(2) == [-10] * 5 and col(3) == [-10, -11, 26, -3, -43]
    assert L.best()[:4] == [(49, 4), (76, 2), (47, 0), (83, 2)]
    assert L.shifted()[4][1] == 0 and all(0 <= v <= 2 * L.reach() for row in L.shifted() for v in row)
    assert all(s[0][b] == L.bias[0] for b in range(B)) and all(s[1][b] == L.x[b][1] + L.bias[1] for b in range(B))   # zero row, unit row
    assert all(s[3][b] == L.x[b][0] + L.bias[3] for b in range(B))                      # +-(2^64 - 1) cancel on the copied feature
    for b in range(B):
        shifted = [L.shifted()[j][b] for j in range(L.J)]
        assert L.best()[b] == (max(shifted), shifted.index(max(shifted))), b


def test_linear_widths_are_the_smallest(keys):
    from protocols.secure_comparison_amd.linear import check_fit

    L = PM.Linear()
    assert _smallest(L.l(), max(v for row in L.shifted() for v in row)) and _smallest(L.l(), 2 * L.reach()) and L.l() <= 16
    assert _smallest(L.bits, max(v for x in L.x for v in x))
    nbits = oracle_paillier(keys, 1024).n.bit_length()
    assert L.x_bits(nbits) == 956
    check_fit(L.W, L.x_bits(nbits), nbits)                                              # the fit rule just holds
    with pytest.raises(ValueError, match="row 3"):
        check_fit(L.W, L.x_bits(nbits) + 1, nbits)


# ---- chain 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_histogram_planted_rows():
    H = PM.Histogram(4)
    col = lambda rows, b: [r[b] for r in rows]  # noqa: E731
    assert (H.m, H.ib, H.l) == (5, 3, 3)
    assert [col(H.idx, b) for b in range(4)] == [[0] * 5, [3] * 5, [7, 0, 4, 3, 0], [0, 3, 0, 3, 0]]
    assert [col(H.hist(), b) for b in range(4)] == [[5, 0, 0, 0], [0, 0, 0, 5], [3, 0, 0, 2], [3, 0, 0, 2]]    # 7 and 4 count at i mod k
    assert [col(H.cdf(), b) for b in range(4)] == [[5, 5, 5, 5], [0, 0, 0, 5], [3, 3, 3, 5], [3, 3, 3, 5]]
    assert [col(H.cdf(exclusive=True), b) for b in range(2)] == [[0, 5, 5, 5], [0, 0, 0, 0]]
    assert H.quantile(0)[:4] == [0, 3, 0, 0] and H.quantile(4)[:4] == [0, 3, 3, 3] and H.quantile(2)[:4] == [0, 3, 0, 0]
    assert H.ranks[:6] == [0, 1, 2, 3, 4, 0] and H.quantile(H.ranks)[:4] == [0, 3, 0, 3]
    assert col(H.bits_below(0), 1) == [1, 1, 1] and col(H.bits_below(0), 0) == [0, 0, 0] and col(H.bits_below(4), 2) == [1, 1, 1]
    for kth in range(H.m):                                         # the quantile is the number of bins whose running count stays at or below the rank
        assert H.quantile(kth) == [sum(col(H.bits_below(kth), b)) for b in range(B)]
    assert H.below_k()[:3] == [0, 1, 3] and 2 not in H.below_k()
    assert all(H.kth_of_indices(kth)[b] == H.quantile(kth)[b] for kth in range(H.m) for b in H.below_k())
    assert H.kth_of_indices(4)[2] == 7 and H.quantile(4)[2] == 3                        # the sorting network sorts the indices as they are
    one = PM.Histogram(1)
    assert one.hist() == [[5] * B] and one.cdf() == [[5] * B] and one.quantile(4) == [0] * B and one.bits_below(0) == []
    assert max(v for r in one.idx for v in r) >= 1                                      # indices at or above k = 1


def test_histogram_widths_are_the_smallest():
    for k in (4, 1):
        H = PM.Histogram(k)
        assert _smallest(H.ib, max(v for r in H.idx for v in r))
        assert _smallest(H.l, max(v for r in H.cdf() for v in r)) and max(v for r in H.cdf() for v in r) == H.m
        assert min(v for r in H.cdf() for v in r) == (0 if k > 1 else H.m)              # a count of 0 and a count of m


# ---- chain 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_groupby_planted_rows():
    G = PM.Groupby()
    sums = G.sums()
    assert sums[0] == [0, 0, 0, 12 * 4095] and sums[1] == [0] * 4 and sums[3][2:] == [0, 0]
    assert any(i >= G.k for i in G.idx[2])                                              # groups at or above k
    for g in range(G.G):
        assert sums[g] == [sum(v for v, i in zip(G.vals[g], G.idx[g]) if i % G.k == t) for t in range(G.k)]
    ordered, perm = G.ranked()
    for g in range(G.G):
        assert ordered[g] == sorted(sums[g], reverse=True) and sorted(perm[g]) == list(range(G.k)), g
        assert [sums[g][t] for t in perm[g]] == ordered[g], g
    assert perm[0][0] == 3 and perm[1] == [0, 1, 2, 3] and perm[3][:2] == [0, 1]        # equal keys are never exchanged
    assert G.first_label()[0] == G.table[3][0] == 31 and G.first_label()[1] == G.table[0][1]


def test_groupby_widths_are_the_smallest():
    G = PM.Groupby()
    assert _smallest(G.l, max(max(r) for r in G.sums())) and G.l == 16
    assert _smallest(G.bits, max(max(r) for r in G.vals)) and _smallest(G.ib, max(max(r) for r in G.idx))
    assert _smallest(G.table_bits, max(max(r) for r in G.table)) and _smallest(PM.index_bits(G.k), max(max(r) for r in G.ranked()[1]))


# ---- chain 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_arithmetic_planted_rows():
    Ar = PM.Arithmetic()
    P = len(Ar.PLANTED)
    assert (Ar.xb, Ar.l, Ar.offset) == (4, 9, 256)
    assert Ar.products()[:6] == [64, 64, 64, -56, -56, -56]                              # the most negative operand with itself
    assert Ar.sums()[:P] == [192, -168, 0, 0, -1, -56, 41]
    assert Ar.shifted()[:P] == [448, 88, 256, 256, 255, 200, 297]
    assert Ar.in_range()[:P] == [0, 0, 1, 1, 1, 1, 1]                                   # both ends of the interval belong to it
    eq, le, ge = Ar.equal()
    assert eq[:P] == [0, 0, 1, 1, 0, 0, 0] and le[:P] == [0, 1, 1, 1, 1, 1, 0] and ge[:P] == [1, 0, 1, 1, 0, 0, 1]
    assert all(e == (a & b) for e, a, b in zip(eq, le, ge))


def test_arithmetic_widths_are_the_smallest():
    Ar = PM.Arithmetic()
    signed_fits = lambda v, bits: -(1 << (bits - 1)) <= v < (1 << (bits - 1))  # noqa: E731
    assert all(signed_fits(v, Ar.xb) for v in Ar.x + Ar.y) and not signed_fits(min(Ar.x), Ar.xb - 1)
    assert _smallest(Ar.l, max(Ar.shifted())) and min(Ar.shifted()) >= 0 and Ar.l <= 16
    assert all(_fits(c + Ar.offset, Ar.l) for c in (Ar.range_lo, Ar.range_hi, Ar.equal_to))


# ---- the stand-in engine ------------------------------------------------------------------------------------------------------------------
def test_no_chain_fits_the_stand_in_engine():
    """One entry point per chain that tests/_oracle_engine.py does not have: the module docstring's statement, kept true."""
    from _oracle_engine import OracleEngine

    needs = {"kNN classify, nearest label, two players": "initiator_dot_pack", "linear score": "paillier_linear_axis",
             "histogram median": "initiator_onehot_pack", "group-by then rank": "initiator_mul_pack", "arithmetic chain": "paillier_sum_axis"}
    assert [chain for chain, name in needs.items() if hasattr(OracleEngine, name)] == []

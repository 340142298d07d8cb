"""The draw layer on the CPU: the generator calls draw_alice / draw_bob / draw_select / draw_mul make -- their order, arguments and
item layout -- against tests/_draw_replay.py; the widths and the freshness of what they return; and the replay's drivers themselves
decrypting to plain Python, so that the expected side of tests/test_gpu_own_draws.py is right before a GPU sees it."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _draw_replay as dr  # noqa: E402
import _select_model as sm  # noqa: E402
import _sort_model as som  # noqa: E402
import _topk_model as tm  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402
from conftest import oracle_dgk  # noqa: E402
from oracle import sc_oracle as o  # noqa: E402

KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
KEY_B = bytes((13 * i + 1) & 0xFF for i in range(32))
L, RBITS = 16, 400


class RecordingEngine(OracleEngine):
    """The CPU stand-in engine, keeping (kind, bits or n or k, count, nonzero) of every generator call."""

    def __init__(self, key=KEY):
        super().__init__()
        self.calls = []
        self.rng_seed(key)

    def rng_bits(self, bits, count):
        self.calls.append(("bits", bits, count, False))
        return super().rng_bits(bits, count)

    def rng_below(self, n, count, nonzero=False):
        self.calls.append(("below", n, count, bool(nonzero)))
        return super().rng_below(n, count, nonzero)

    def rng_coins(self, count):
        self.calls.append(("coins", None, count, False))
        return super().rng_coins(count)

    def rng_permutations(self, k, count):
        self.calls.append(("perms", k, count, False))
        return super().rng_permutations(k, count)


@pytest.fixture(scope="module")
def sk512():
    return o.PaillierKey.generate(512, random.Random(1))


@pytest.fixture(scope="module")
def dgk(keys):
    return oracle_dgk(keys, "dgk_1024_l16")


def _schemes(eng, sk, dk):
    from protocols.secure_comparison_amd import DGK, Paillier

    bp = Paillier(sk.n, sk.p, sk.q, engine=eng)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=eng, randomizer_bits=RBITS)
    return bp.public_copy(), bd.public_copy(), bp, bd


def _ints(eng, t):
    return eng.download(t.reshape(-1, t.shape[-1]))


# ---- call order -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 5])
def test_comparison_draws_follow_the_replay(sk512, dgk, count):
    from protocols.secure_comparison_amd.batch import draw_alice, draw_bob
    from protocols.secure_comparison_amd.selection import _comparison_draws

    eng = RecordingEngine()
    ap, ad, bp, bd = _schemes(eng, sk512, dgk)
    rp = dr.Replay(KEY)
    rows, lp1 = range(count), L + 1
    a = draw_alice(count, L, ap, ad)
    want_a = dr.comparison(rp, rows, count, L, sk512.n, dgk.u, RBITS, alice=True, bob=False)
    b = draw_bob(count, L, bp, bd)
    want_b = dr.comparison(rp, rows, count, L, sk512.n, dgk.u, RBITS, alice=False, bob=True)
    both = _comparison_draws(count, L, ap, ad, bp, bd)
    want = dr.comparison(rp, rows, count, L, sk512.n, dgk.u, RBITS)
    assert eng.calls == rp.log and len(rp.log) == 16 and eng._rng_call == rp.call
    assert [c[0] for c in rp.log[:8]] == ["below", "coins", "below", "perms", "below", "bits", "below", "bits"]

    def check_alice(t, w):
        assert _ints(eng, t.r) == [d.r for d in w] and t.delta_a.tolist() == [d.delta_a for d in w]
        assert t.permutation.tolist() == [d.perm for d in w] and _ints(eng, t.rho_z) == [d.rho_z for d in w]
        assert tuple(t.rhos.shape[:2]) == (lp1, count) and tuple(t.r_alice_dgk.shape) == (lp1, count, (RBITS + 31) // 32)
        for k in range(count):
            assert eng.download(t.rhos[:, k]) == w[k].rhos
            ra = eng.download(t.r_alice_dgk[:, k])
            assert [ra[src] for src in w[k].perm] == w[k].r_c

    def check_bob(t, w):
        assert _ints(eng, t.rho_zeta_1) == [d.rho_zeta1 for d in w] and _ints(eng, t.rho_zeta_2) == [d.rho_zeta2 for d in w]
        assert _ints(eng, t.rho_delta_b) == [d.rho_delta_b for d in w]
        for k in range(count):
            assert eng.download(t.r_bob_dgk[:, k]) == [w[k].r_d] + w[k].r_beta

    check_alice(a, want_a), check_bob(b, want_b), check_alice(both, want), check_bob(both, want)
    assert a.r_bob_dgk is None and a.rho_zeta_1 is None and b.r is None and b.rhos is None and b.permutation is None
    assert want_a[0].r_d is None and want_a[0].rho_zeta1 is None and want_b[0].r is None and want_b[0].r_c is None


@pytest.mark.parametrize("kappa", [1, 32, 33, 62])
@pytest.mark.parametrize("widths", [(16,), (16, 3), (7, 40, 1), (64, 10, 33, 2)])
@pytest.mark.parametrize("alice,bob", [(True, True), (True, False), (False, True)])
def test_select_draws_follow_the_replay(sk512, kappa, widths, alice, bob):
    from protocols.secure_comparison_amd import Paillier
    from protocols.secure_comparison_amd.selection import SelectLayout, draw_select

    eng = RecordingEngine()
    pai = Paillier(sk512.n, engine=eng)
    lay = SelectLayout(widths[0], kappa, widths[1:], 2048)        # the layout's fit rule is not the subject here
    rp = dr.Replay(KEY)
    count, n, nf = 6, sk512.n, len(widths)
    for _ in range(2):                                            # two calls in a row: the second continues the numbering
        got = draw_select(count, lay, pai, alice=alice, bob=bob)
        want = dr.selection(rp, range(count), count, kappa, list(widths), n, alice=alice, bob=bob)
        assert eng.calls == rp.log and eng._rng_call == rp.call
        if alice:
            assert tuple(got.r_a.shape) == (count, (kappa + 31) // 32) and _ints(eng, got.r_a) == [w[0] for w in want]
            assert tuple(got.r_b.shape) == (nf, count, (max(widths) + kappa + 2 + 31) // 32)
            for j in range(nf):                                   # integer equality: the padding up to the widest column is zero
                assert eng.download(got.r_b[j]) == [w[1][j] for w in want]
            assert _ints(eng, got.rho_p) == [w[2] for w in want]
        else:
            assert got.r_a is None and got.r_b is None and got.rho_p is None and want[0][:3] == (None, None, None)
        if bob:
            assert tuple(got.rho_products.shape[:2]) == (nf, count)
            for j in range(nf):
                assert eng.download(got.rho_products[j]) == [w[3][j] for w in want]
        else:
            assert got.rho_products is None and want[0][3] is None
    kinds = ([("bits", kappa)] + [("bits", w + 1 + kappa) for w in widths] + [("below", n)] if alice else []) + ([("below", n)] if bob else [])
    assert [c[:2] for c in rp.log] == kinds * 2
    assert all(c[3] for c in rp.log if c[0] == "below")           # every randomizer base is drawn nonzero


@pytest.mark.parametrize("kappa", [1, 32, 33, 62])
@pytest.mark.parametrize("wx,wy", [(16, (16,)), (16, (16, 7)), (1, (1, 255, 8)), (255, (3, 64, 33, 2))])
@pytest.mark.parametrize("alice,bob", [(True, True), (True, False), (False, True)])
def test_mul_draws_follow_the_replay(sk512, kappa, wx, wy, alice, bob):
    from protocols.secure_comparison_amd import Paillier
    from protocols.secure_comparison_amd.multiplication import MulLayout, draw_mul

    eng = RecordingEngine()
    pai = Paillier(sk512.n, engine=eng)
    lay = MulLayout(kappa, wx, wy, False, 4096)
    rp = dr.Replay(KEY)
    count, n, nf = 6, sk512.n, len(wy)
    for _ in range(2):
        got = draw_mul(count, lay, pai, alice=alice, bob=bob)
        want = dr.multiplication(rp, range(count), count, kappa, wx, list(wy), n, alice=alice, bob=bob)
        assert eng.calls == rp.log and eng._rng_call == rp.call
        if alice:
            assert tuple(got.r_a.shape) == (count, (wx + kappa + 31) // 32) and _ints(eng, got.r_a) == [w[0] for w in want]
            assert tuple(got.r_b.shape) == (nf, count, (max(wy) + kappa + 31) // 32)
            for j in range(nf):
                assert eng.download(got.r_b[j]) == [w[1][j] for w in want]
            assert _ints(eng, got.rho_p) == [w[2] for w in want]
        else:
            assert got.r_a is None and got.r_b is None and got.rho_p is None and want[0][:3] == (None, None, None)
        if bob:
            assert tuple(got.rho_products.shape[:2]) == (nf, count)
            for j in range(nf):
                assert eng.download(got.rho_products[j]) == [w[3][j] for w in want]
        else:
            assert got.rho_products is None and want[0][3] is None
    kinds = ([("bits", wx + kappa)] + [("bits", w + kappa) for w in wy] + [("below", n)] if alice else []) + ([("below", n)] if bob else [])
    assert [c[:2] for c in rp.log] == kinds * 2
    assert all(c[3] for c in rp.log if c[0] == "below")


def test_replay_restates_the_generator_per_item():
    """The Replay object itself: each method is oracle/chacha_rng.py at the current call number for the chosen items, and advances by
    one."""
    from oracle import chacha_rng as cr

    rp = dr.Replay(KEY)
    n = (1 << 200) + 12345
    assert rp.bits(70, 100, [0, 64, 99]) == [cr.rng_bits(KEY, 0, 70, 100)[i] for i in (0, 64, 99)]
    assert rp.below(n, 100, True, [3, 98]) == [cr.rng_below(KEY, 1, n, 100, True)[i] for i in (3, 98)]
    assert rp.coins(600, [0, 511, 512]) == [cr.rng_coins(KEY, 2, 600)[i] for i in (0, 511, 512)]
    assert rp.perms(17, 70, [63, 64]) == [cr.rng_permutations(KEY, 3, 17, 70)[i] for i in (63, 64)]
    assert rp.bits(8, 4, []) == [] and rp.call == 5
    assert rp.log == [("bits", 70, 100, False), ("below", n, 100, True), ("coins", None, 600, False), ("perms", 17, 70, False),
                      ("bits", 8, 4, False)]


def test_sort_layers_are_the_packages_layers():
    """The grouping of _sort_model.comparators into layers, written from the network's definition, is the schedule both players walk."""
    from protocols.secure_comparison_amd.sorting import batcher_network, sort_schedule

    for k in list(range(1, 40)) + [64, 100, 257]:
        assert dr.sort_layers(k) == batcher_network(k), k
    for k, B, max_rows in ((5, 6, 7), (5, 6, 65536), (9, 4, 5), (17, 3, 1)):
        assert [c for _, c in sort_schedule(k, B, max_rows)] == [dr.cuts(B * len(layer), max_rows) for layer in dr.sort_layers(k)]
    assert [len(layer) for layer in dr.sort_layers(5)] == [2, 2, 1, 1, 1, 2] and dr.cuts(12, 7) == [(0, 7), (7, 12)]


# ---- widths ---------------------------------------------------------------------------------------------------------------------------
ROWS = 4096


def _width_checks(eng, first, second, a_bits, col_bits, n):
    """first: the draws of a ROWS-row call; second: of the next call.  Every value inside its range and, over ROWS rows, beyond 3/4 of
    it (a uniform draw misses that with probability (3/4)^4096 < 2^-1000; a draw 8 bits short never reaches it); no two rows, no two
    columns and no two calls alike."""
    seen = []
    for name, t, top in [("r_a", first.r_a, 1 << a_bits)] + [(f"r_b[{j}]", first.r_b[j], 1 << w) for j, w in enumerate(col_bits)] + \
            [("rho_p", first.rho_p, n)] + [(f"rho_products[{j}]", first.rho_products[j], n) for j in range(len(col_bits))]:
        v = eng.download(t)
        assert len(v) == ROWS and all(0 <= x < top for x in v), name
        assert max(v) > 3 * top // 4, name
        if name.startswith("rho"):
            assert min(v) >= 1, name
        if top >= 1 << 40:                                       # (narrower ranges repeat by birthday alone)
            assert len(set(v)) == ROWS, name
        seen.append((name, v))
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            if seen[i][0][:3] == seen[j][0][:3]:                 # the columns of r_b among themselves, every rho array among themselves
                assert seen[i][1] != seen[j][1] and (seen[i][0][:3] != "rho" or not set(seen[i][1]) & set(seen[j][1])), (seen[i][0], seen[j][0])
    for (name, v), t in zip(seen, [second.r_a, *second.r_b, second.rho_p, *second.rho_products]):
        w = eng.download(t)
        assert w != v[:len(w)], name
        if max(v) >= 1 << 40:
            assert not set(w) & set(v), name


def test_select_draws_fill_their_ranges_and_never_repeat(sk512):
    from protocols.secure_comparison_amd import Paillier
    from protocols.secure_comparison_amd.selection import SelectLayout, draw_select

    eng = RecordingEngine()
    pai = Paillier(sk512.n, engine=eng)
    kappa, widths = 40, (16, 16)                                 # two columns of one width: only fresh calls tell them apart
    lay = SelectLayout(widths[0], kappa, widths[1:], 2048)
    first, second = draw_select(ROWS, lay, pai), draw_select(64, lay, pai)
    _width_checks(eng, first, second, kappa, [w + 1 + kappa for w in widths], sk512.n)


def test_mul_draws_fill_their_ranges_and_never_repeat(sk512):
    from protocols.secure_comparison_amd import Paillier
    from protocols.secure_comparison_amd.multiplication import MulLayout, draw_mul

    eng = RecordingEngine()
    pai = Paillier(sk512.n, engine=eng)
    kappa, wx, wy = 40, 16, (7, 7)
    lay = MulLayout(kappa, wx, wy, False, 2048)
    first, second = draw_mul(ROWS, lay, pai), draw_mul(64, lay, pai)
    _width_checks(eng, first, second, wx + kappa, [w + kappa for w in wy], sk512.n)


# ---- the drivers on plaintext -----------------------------------------------------------------------------------------------------------
def _enc(sk, rng, values):
    return [sm.enc(sk, v, rng.randrange(1, sk.n)) for v in values]


def _dec(sk, cs):
    return [sm.dec(sk, c) for c in cs]


TOP = (1 << L) - 1


@pytest.mark.parametrize("two_keys", [False, True])
def test_driver_compare_exchange_minimum_maximum(sk512, dgk, two_keys):
    sk, rng = sk512, random.Random(3)
    xs, ys = [0, TOP, 7, 7, 9, 123], [TOP, 0, 7, 8, 3, 123]
    rows, count = [0, 1, 63, 64, 69, 5], 70
    x_c, y_c = _enc(sk, rng, xs), _enc(sk, rng, ys)
    d = dr.Driver(sk, dgk, L, RBITS, KEY, KEY_B if two_keys else None)
    lo, hi = d.compare_exchange([x_c], [y_c], [L], rows, count)
    assert _dec(sk, lo[0]) == [min(x, y) for x, y in zip(xs, ys)] and _dec(sk, hi[0]) == [max(x, y) for x, y in zip(xs, ys)]
    assert d.calls == ((6 + 3, 2 + 1) if two_keys else (12, 12))   # comparison (6 + 2 calls), one-column selection (3 + 1)
    mn, delta = d.minmax(x_c, y_c, rows, count, False)
    mx, delta2 = d.minmax(x_c, y_c, rows, count, True)
    assert _dec(sk, mn) == [min(x, y) for x, y in zip(xs, ys)] and _dec(sk, mx) == [max(x, y) for x, y in zip(xs, ys)]
    assert _dec(sk, delta) == _dec(sk, delta2) == [int(x <= y) for x, y in zip(xs, ys)]
    assert d.calls == ((27, 9) if two_keys else (36, 36)) and len(d.wire) == 3
    assert len({c for rec in d.wire for c in rec["P"]}) == 3 * len(rows)      # fresh draws in every exchange


@pytest.mark.parametrize("want_max", [False, True])
def test_driver_tournament(sk512, dgk, want_max):
    sk, rng = sk512, random.Random(4)
    rows_plain = [[5, 5, 1, 1, 9], [0, TOP, 0, TOP, TOP], [3, 2, 1, 0, 0], [7, 7, 7, 7, 7]]
    vals = [_enc(sk, rng, r) for r in rows_plain]
    d = dr.Driver(sk, dgk, L, RBITS, KEY)
    v, i = d.argext(vals, 4, range(4), want_max)
    best = [max(r) if want_max else min(r) for r in rows_plain]
    assert _dec(sk, v) == best and _dec(sk, i) == [r.index(b) for r, b in zip(rows_plain, best)]
    assert d.calls[0] == 3 * (8 + 5)                             # three rounds, a two-column selection each


@pytest.mark.parametrize("descending,max_rows", [(False, 4), (True, 65536)])
def test_driver_sort(sk512, dgk, descending, max_rows):
    sk, rng = sk512, random.Random(5)
    k, B = 5, 3
    keys_plain = [[5, 5, 1, TOP, 0], [9, 8, 7, 6, 5], [3, 3, 3, 0, 3]]
    pays = [[rng.getrandbits(10) for _ in range(k)] for _ in range(B)]
    table = [[_enc(sk, rng, keys_plain[b]), _enc(sk, rng, pays[b]), [(1 + p * sk.n) % sk.n2 for p in range(k)]] for b in range(B)]
    widths = [L, 10, sm.index_bits(k)]
    d = dr.Driver(sk, dgk, L, RBITS, KEY)
    out = d.sort(table, B, k, range(B), widths, max_rows, descending)
    want = som.apply(dr.sort_layers(k), [[(keys_plain[b][p], pays[b][p], p) for p in range(k)] for b in range(B)], descending)
    for b in range(B):
        got = list(zip(*[_dec(sk, col) for col in out[b]]))
        assert got == [tuple(t) for t in want[b]] and [t[0] for t in got] == sorted(keys_plain[b], reverse=descending)
    batches = sum(len(dr.cuts(B * len(layer), max_rows)) for layer in dr.sort_layers(k))
    assert batches == (9 if max_rows == 4 else 6) and d.calls[0] == batches * (8 + 6)


@pytest.mark.parametrize("largest", [False, True])
def test_driver_topk_and_kth(sk512, dgk, largest):
    from protocols.secure_comparison_amd.sorting import topk_network

    sk, rng = sk512, random.Random(6)
    k, m, B = 6, 2, 2
    plain = [[4, 9, 4, 0, TOP, 7], [1, 1, 1, 1, 0, 1]]
    for only_last in (False, True):
        layers = topk_network(k, m, only_last)
        table = [[_enc(sk, rng, r)] for r in plain]
        d = dr.Driver(sk, dgk, L, RBITS, KEY)
        out = d.topk(table, B, layers, range(B), [L], 65536, largest)
        want = tm.apply(layers, [[(v,) for v in r] for r in plain], largest)
        for b in range(B):
            got = _dec(sk, out[b][0])
            assert got == [t[0] for t in want[b]]
            ordered = sorted(plain[b], reverse=largest)
            assert got[m - 1] == ordered[m - 1] and (only_last or got[:m] == ordered[:m])
        assert d.calls[0] == len(layers) * (8 + 4)


def test_driver_multiply_boolean_equal_in_range(sk512, dgk):
    sk, rng, n = sk512, random.Random(7), sk512.n
    xs, y0, y1 = [-32768, 32767, 0, -1, 255], [32767, -32768, 5, -1, 255], [-64, 63, 1, 0, -7]
    rows, count = [0, 1, 63, 64, 69], 70
    d = dr.Driver(sk, dgk, L, RBITS, KEY)
    x_c = _enc(sk, rng, xs)
    out = d.multiply(x_c, [_enc(sk, rng, y0), _enc(sk, rng, y1)], rows, count, 16, [16, 7], signed=True)
    assert _dec(sk, out[0]) == [x * y % n for x, y in zip(xs, y0)] and _dec(sk, out[1]) == [x * y % n for x, y in zip(xs, y1)]
    assert d.calls == (5, 5)                                     # r_a, two columns, rho_p; Bob's products
    sq = d.multiply(x_c, [x_c], rows, count, 16, [16], signed=True)
    assert _dec(sk, sq[0]) == [x * x % n for x in xs]
    a, b = [0, 0, 1, 1], [0, 1, 0, 1]
    a_c, b_c = _enc(sk, rng, a), _enc(sk, rng, b)
    for op, fn in (("and", lambda p, q: p & q), ("or", lambda p, q: p | q), ("xor", lambda p, q: p ^ q)):
        assert _dec(sk, d.bit_op(a_c, b_c, range(4), 4, op)) == [fn(p, q) for p, q in zip(a, b)]
    pairs = [(0, 0), (TOP, TOP), (0, TOP), (TOP, 0), (5, 6), (6, 5), (-1, -1), (-5, -4)]
    before = d.calls[0]
    eq, le, ge = d.equal(_enc(sk, rng, [p for p, _ in pairs]), _enc(sk, rng, [q for _, q in pairs]), range(8), 8)
    assert _dec(sk, eq) == [int(p == q) for p, q in pairs] and _dec(sk, le) == [int(p <= q) for p, q in pairs]
    assert _dec(sk, ge) == [int(q <= p) for p, q in pairs] and d.calls[0] == before + 8 + 4
    trip = [(3, 3, 9), (9, 3, 9), (2, 3, 9), (10, 3, 9), (0, 0, TOP), (5, 6, 4)]
    got = d.in_range(*[_enc(sk, rng, [t[c] for t in trip]) for c in range(3)], range(6), 6)
    assert _dec(sk, got) == [int(lo <= x <= hi) for x, lo, hi in trip]

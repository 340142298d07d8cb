"""Secure inner product without a GPU: the pure-Python model (tests/_dot_model.py) decrypts to sum_j x_j y_j on a 512-bit oracle key;
the package's DotLayout, the library's sc_dot_layout (host code, no context) and the model agree on (sa, sb, pb, g, M, ebits) and on
every refusal; g is maximal; the pair-to-message mapping is a bijection; and draw_dot's generator calls -- order, item layout, widths,
padding, an independent mask per field -- are held to tests/_draw_replay.py's Replay."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _dot_model as model  # noqa: E402
import _draw_replay as dr  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402

KEY = bytes((7 * i + 3) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def sk():
    from oracle import sc_oracle as o

    return o.PaillierKey.generate(512, random.Random(20261))


def _edges(w, signed):
    return [-(1 << (w - 1)), -1, (1 << (w - 1)) - 1, 0, 1] if signed else [0, 1, (1 << w) - 1]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("wx,wy,k", [(1, 1, 1), (8, 8, 3), (32, 17, 4), (32, 17, 9), (64, 64, 2), (16, 1, 17)])
def test_model_dot_decrypts_to_the_inner_product(sk, signed, wx, wy, k):
    """512-bit key, kappa = 40: (32, 17) has pb = 131 and g = 3, so k = 4 and 9 take two and three messages with a partial top position."""
    rng = random.Random(wx * 1000 + wy * 10 + k + signed)
    n, kappa = sk.n, 40
    ex, ey = _edges(wx, signed), _edges(wy, signed)
    for t in range(len(ex)):
        xs = [ex[(t + j) % len(ex)] for j in range(k)]
        ys = [ey[(t + 2 * j) % len(ey)] for j in range(k)]
        for fill in (0, 1, None):                 # every mask 0, every mask at its maximum, random masks
            draws = None
            if fill is not None:
                M = model.layout(kappa, wx, wy, False, k, n.bit_length())[4]
                draws = ([fill * ((1 << (wx + kappa)) - 1)] * k, [fill * ((1 << (wy + kappa)) - 1)] * k, [rng.randrange(1, n) for _ in range(M)],
                         rng.randrange(1, n))
            assert model.dot(sk, xs, ys, wx, wy, rng, signed, kappa, draws) == sum(x * y for x, y in zip(xs, ys)) % n, (xs, ys, fill)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("wx,k", [(1, 1), (8, 5), (32, 6), (32, 7), (33, 13), (100, 3)])
def test_model_sum_of_squares(sk, signed, wx, k):
    """512-bit key, kappa = 40, square mode: wx = 32 has pb = 73 and g = 6."""
    rng = random.Random(wx * 100 + k + signed)
    n, kappa = sk.n, 40
    ex = _edges(wx, signed)
    for t in range(len(ex)):
        xs = [ex[(t + j) % len(ex)] for j in range(k)]
        for fill in (0, 1, None):
            draws = None
            if fill is not None:
                M = model.layout(kappa, wx, 0, True, k, n.bit_length())[4]
                draws = ([fill * ((1 << (wx + kappa)) - 1)] * k, None, [rng.randrange(1, n) for _ in range(M)], rng.randrange(1, n))
            assert model.dot(sk, xs, None, wx, 0, rng, signed, kappa, draws) == sum(x * x for x in xs) % n, (xs, fill)


def test_model_coef_and_base(sk):
    rng = random.Random(5)
    n = sk.n
    xs, ys = [3, -4, 5], [7, 6, -2]
    x_cs, y_cs = [model.enc(sk, x, rng.randrange(1, n)) for x in xs], [model.enc(sk, y, rng.randrange(1, n)) for y in ys]
    base = model.enc(sk, 1000, rng.randrange(1, n))
    for coef in (1, -1, -2):
        out = model.dot_enc(sk, 40, 8, 8, True, False, x_cs, y_cs, model.draw(rng, 40, 8, 8, False, 3, n), base, coef)
        assert model.dec(sk, out) == (1000 + coef * (21 - 24 - 10)) % n


def test_model_flags_a_message_past_its_own_end(sk):
    """k = 8 at g = 3: messages 0 and 1 hold three pairs, message 2 two.  A key holder who reads the same messages with k = 7 expects two
    pairs in message 1 and finds a third: flagged, though no message has a bit past message 0's end."""
    rng = random.Random(6)
    n, kappa, w = sk.n, 40, 32
    top = (1 << (w + kappa)) - 1
    x_cs = [model.enc(sk, (1 << w) - 1)] * 8
    Ps = model.pack(sk, kappa, w, 17, False, False, x_cs, x_cs, [top] * 8, [(1 << (17 + kappa)) - 1] * 8, [rng.randrange(1, n) for _ in range(3)])
    assert model.layout(kappa, w, 17, False, 8, 512)[3:5] == (3, 3)
    assert model.answer(sk, kappa, w, 17, False, 8, Ps, 5)[2] is False
    # k = 7 keeps M = 3 but message 1 then holds two pairs, not three: its third position is past its end
    assert model.answer(sk, kappa, w, 17, False, 7, Ps, 5)[2] is True
    # message 0 alone decides nothing there: with end_0 taken for every message the k = 7 reading would pass
    assert all(model.dec(sk, P) >> (3 * 131) == 0 for P in Ps)


# ---- the three copies of the fit rule ---------------------------------------------------------------------------------------------------
def _three(nbits, kappa, wx, wy, square, k):
    """(sa, sb, pb, g, M, ebits) from DotLayout, sc_dot_layout and the model, or None from each on a refusal; they must agree."""
    from protocols.secure_comparison_amd import DotLayout, _lib
    from protocols.secure_comparison_amd.engine import dot_layout

    def attempt(f):
        try:
            return tuple(f())
        except ValueError:
            return None

    def py():
        lay = DotLayout(kappa, wx, wy, k, False, square, nbits)
        return lay.sa, lay.sb, lay.pb, lay.g, lay.M, lay.ebits

    got = [attempt(py), attempt(lambda: dot_layout(_lib.load(), nbits, kappa, wx, wy, False, square, k)),
           attempt(lambda: model.layout(kappa, wx, wy, square, k, nbits))]
    assert got[0] == got[1] == got[2], (nbits, kappa, wx, wy, square, k, got)
    return got[0]


@pytest.mark.parametrize("nbits", [512, 1024, 2048, 3072])
@pytest.mark.parametrize("square", [False, True])
def test_layouts_agree_over_the_sweep(nbits, square):
    fits = refused = 0
    for kappa in (1, 40, 62):
        for wx in (1, 31, 32, 33, 255):
            for wy in ((0,) if square else (1, 31, 32, 33, 255)):
                one = _three(nbits, kappa, wx, wy, square, 1)
                if one is None:                                    # not even one pair: every k is refused alike
                    assert _three(nbits, kappa, wx, wy, square, 1024) is None
                    refused += 1
                    continue
                sa, sb, pb, g, M, ebits = one
                assert sa == wx + kappa + 1 and sb == (0 if square else wy + kappa + 1) and pb == sa + sb and M == 1
                assert g * pb < nbits - 1 <= (g + 1) * pb          # g is maximal
                assert ebits == (sa + 1 if square else max(sa, sb))
                for k in sorted({1, g - 1, g, g + 1, 2 * g, 1024} - {0}):
                    got = _three(nbits, kappa, wx, wy, square, k)
                    if got is None:
                        refused += 1
                        # only the sum rule or k's own range (narrow fields: 2 g > 1024) can refuse here
                        assert k > 1024 or (2 * sa if square else pb) + (k - 1).bit_length() >= nbits - 1
                        continue
                    fits += 1
                    assert got[:4] == (sa, sb, pb, g) and got[4] == -(-k // g)
    assert fits > 20 and (refused > 0 or nbits > 512)


def test_the_issue_s_own_figures():
    assert _three(2048, 40, 32, 32, False, 14)[3:5] == (14, 1)
    assert _three(2048, 40, 32, 0, True, 28)[3:5] == (28, 1)
    assert _three(1024, 40, 32, 32, False, 17)[3:5] == (7, 3)
    assert _three(1024, 40, 255, 200, False, 5)[3:5] == (1, 5)


def test_refusals_agree_and_name_the_quantity():
    from protocols.secure_comparison_amd import DotLayout

    for nbits, kappa, wx, wy, square, k in ((2048, 0, 8, 8, False, 4), (2048, 63, 8, 8, False, 4), (2048, 40, 0, 8, False, 4),
                                            (2048, 40, 256, 8, False, 4), (2048, 40, 8, 0, False, 4), (2048, 40, 8, 256, False, 4),
                                            (2048, 40, 8, 8, False, 0), (2048, 40, 8, 8, False, 1025), (2048, 40, 8, 8, True, 0),
                                            (512, 62, 255, 255, False, 1),       # pb = 636: no pair fits
                                            (512, 62, 255, 0, True, 1),          # square: one field of 318 bits fits, its square (636) does not
                                            (299, 62, 87, 85, False, 1), (300, 62, 87, 85, False, 2)):
        assert _three(nbits, kappa, wx, wy, square, k) is None, (nbits, kappa, wx, wy, square, k)
    # the sum rule one bit either side: pb' = 87 + 85 + 126 = 298; k = 1 needs 298 < nbits - 1, k = 2 needs 299 < nbits - 1
    assert _three(299, 62, 87, 85, False, 1) is None and _three(300, 62, 87, 85, False, 1) is not None
    assert _three(300, 62, 87, 85, False, 2) is None and _three(301, 62, 87, 85, False, 2) is not None
    assert _three(301, 62, 87, 85, False, 3) is None and _three(302, 62, 87, 85, False, 3) is not None      # ceil(log2 3) = 2
    assert _three(302, 62, 87, 85, False, 4) is not None and _three(302, 62, 87, 85, False, 5) is None
    # square mode ignores wy altogether
    assert _three(2048, 40, 8, 999, True, 4) == _three(2048, 40, 8, 0, True, 4)
    for kw, what in ((dict(kappa=63), "kappa"), (dict(wx=256), "wx"), (dict(wy=0), "wy"), (dict(k=1025), "k = 1025"),
                     (dict(kappa=62, wx=255, wy=255, nbits=512), "pb = 636"), (dict(kappa=62, wx=87, wy=85, k=2, nbits=300), "sum of k = 2")):
        args = dict(kappa=40, wx=8, wy=8, k=4, nbits=2048)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            DotLayout(**args)


@pytest.mark.parametrize("nbits,wx,wy,square", [(1024, 32, 32, False), (2048, 32, 32, False), (2048, 32, 0, True), (1024, 255, 200, False),
                                                (512, 1, 1, False)])
def test_the_mapping_is_a_bijection(nbits, wx, wy, square):
    from protocols.secure_comparison_amd import DotLayout

    g = DotLayout(40, wx, wy, 1, False, square, nbits).g
    for k in sorted({1, 2, g - 1, g, g + 1, 2 * g, 2 * g + 1, 3 * g - 1, 100, 1024} - {0}):
        try:
            lay = DotLayout(40, wx, wy, k, False, square, nbits)
        except ValueError:
            continue
        M = lay.M
        where = [lay.position(j) for j in range(k)]
        assert where == [model.position(j, M) for j in range(k)]
        assert len(set(where)) == k                                           # no two pairs share a slot
        n_m = [sum(1 for m, _ in where if m == mm) for mm in range(M)]
        assert sum(n_m) == k and max(n_m) <= lay.g and min(n_m) >= 1
        for mm in range(M):                                                   # positions 0 .. n_m - 1, no holes; the members by ascending j
            assert sorted(t for m, t in where if m == mm) == list(range(n_m[mm]))
            assert model.members(mm, k, M) == [t * M + mm for t in range(n_m[mm])]
        top = max(t for _, t in where)                                        # the messages with a pair at the top position are a prefix
        holders = [m for m, t in where if t == top]
        assert holders == list(range(len(holders)))
        assert all(n_m[mm] * lay.pb < nbits - 1 for mm in range(M))
    with pytest.raises(ValueError):
        DotLayout(40, wx, wy, 3, False, square, nbits).position(3)


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------
class RecordingEngine(OracleEngine):
    """The CPU stand-in engine, keeping (kind, bits or n, count, nonzero) of every generator call."""

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


def _ints(eng, t):
    return eng.download(t.reshape(-1, t.shape[-1]))


@pytest.mark.parametrize("wx,wy,k,square", [(32, 17, 9, False), (24, 24, 1, False), (1, 255, 2, False), (32, 0, 7, True), (33, 0, 13, True)])
def test_draw_dot_against_the_replay(sk, wx, wy, k, square):
    """Alice: r_a as k count items of wx + kappa bits, pair j of row b at item j count + b; r_b likewise (absent for a square); rho_p as
    M count items in [1, N), message m of row b at item m count + b.  Bob: count bases.  Rows of exactly ceil(bits / 32) words."""
    from protocols.secure_comparison_amd import DotLayout, Paillier, draw_dot

    kappa, count, n = 40, 6, sk.n
    eng = RecordingEngine()
    pai = Paillier(sk.n, engine=eng)
    lay = DotLayout(kappa, wx, wy, k, False, square, n.bit_length())
    M = lay.M
    rp = dr.Replay(KEY)
    for alice, bob in ((True, True), (True, False), (False, True)):
        got = draw_dot(count, lay, pai, alice=alice, bob=bob)
        if alice:
            r_a = rp.bits(wx + kappa, k * count, range(k * count))
            r_b = None if square else rp.bits(wy + kappa, k * count, range(k * count))
            rho_p = rp.below(n, M * count, True, range(M * count))
        if bob:
            rho_d = rp.below(n, count, True, range(count))
        assert eng.calls == rp.log and eng._rng_call == rp.call
        if alice:
            assert tuple(got.r_a.shape) == (k, count, (wx + kappa + 31) // 32) and _ints(eng, got.r_a) == r_a
            assert eng.download(got.r_a[k - 1])[count - 1] == r_a[(k - 1) * count + count - 1]          # element-major
            if square:
                assert got.r_b is None
            else:
                assert tuple(got.r_b.shape) == (k, count, (wy + kappa + 31) // 32) and _ints(eng, got.r_b) == r_b
            assert tuple(got.rho_p.shape) == (M, count, (n.bit_length() + 31) // 32) and _ints(eng, got.rho_p) == rho_p
            assert all(1 <= v < n for v in rho_p)
        else:
            assert got.r_a is None and got.r_b is None and got.rho_p is None
        if bob:
            assert tuple(got.rho_d.shape) == (count, (n.bit_length() + 31) // 32) and eng.download(got.rho_d) == rho_d
        else:
            assert got.rho_d is None
    hers = ["bits", "below"] if square else ["bits", "bits", "below"]
    assert [c[0] for c in eng.calls] == hers + ["below"] + hers + ["below"]         # both players, Alice alone, Bob alone


def test_no_two_fields_of_a_row_share_a_mask(sk):
    """4096 rows of k = 5 pairs: the 10 masks of a row are pairwise different, fill their ranges, and differ from row to row and from
    call to call (a mask shared across the fields of a row would hand the key holder x_i - x_j)."""
    from protocols.secure_comparison_amd import DotLayout, Paillier, draw_dot

    rows, k, kappa, w = 4096, 5, 40, 16
    eng = RecordingEngine()
    pai = Paillier(sk.n, engine=eng)
    lay = DotLayout(kappa, w, w, k, False, False, sk.n.bit_length())
    first, second = draw_dot(rows, lay, pai), draw_dot(64, lay, pai)
    a, b = _ints(eng, first.r_a), _ints(eng, first.r_b)
    top = 1 << (w + kappa)
    for name, v in (("r_a", a), ("r_b", b)):
        assert len(v) == k * rows and all(0 <= x < top for x in v) and max(v) > 3 * top // 4, name
        assert len(set(v)) == len(v), name                      # 56-bit values: a repeat among 20480 is a shared mask, not chance
    assert not set(a) & set(b)
    for r in range(rows):
        fields = [a[j * rows + r] for j in range(k)] + [b[j * rows + r] for j in range(k)]
        assert len(set(fields)) == 2 * k, r
    rho = _ints(eng, first.rho_p)
    assert len(rho) == lay.M * rows and len(set(rho)) == len(rho) and min(rho) >= 1 and max(rho) < sk.n
    assert not set(_ints(eng, second.r_a)) & set(a) and not set(_ints(eng, second.r_b)) & set(b) and not set(_ints(eng, second.rho_p)) & set(rho)
    assert not set(eng.download(first.rho_d)) & set(rho)
    sq = draw_dot(rows, DotLayout(kappa, w, 0, k, False, True, sk.n.bit_length()), pai)
    v = _ints(eng, sq.r_a)
    assert sq.r_b is None and len(set(v)) == k * rows and not set(v) & set(a)


def test_exports_and_bindings():
    import protocols.secure_comparison_amd as pkg
    from protocols.secure_comparison_amd import _lib, dotproduct

    for name in ("DotLayout", "DotDraws", "draw_dot", "secure_dot_batch", "secure_sum_squares_batch", "secure_squared_distance_batch"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("dot_pack", "dot_sum", "dot_finish", "dot_batch"):
        assert hasattr(dotproduct, name)
    for name in ("sc_dot_prep", "sc_dot_split", "sc_dot_layout", "sc_initiator_dot_pack", "sc_keyholder_dot", "sc_initiator_dot_finish"):
        assert name in _lib.SYMBOLS
    for cls in (pkg.Initiator, pkg.KeyHolder):
        assert hasattr(cls, "perform_secure_dot_batch")
    assert pkg.DotLayout(40, 32, 32, 15, True, False, 2048).header == [40, 32, 32, 1, 0, 15]
    assert pkg.DotLayout(40, 32, 32, 15, False, True, 2048).header == [40, 32, 0, 0, 1, 15]

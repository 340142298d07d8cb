"""Secure multiplication without a GPU: the pure-Python model (tests/_mult_model.py) decrypts to the products on a 512-bit oracle
key, the package's MulLayout equals the model's layout and refuses what the model refuses, and the Boolean operations, equality and
interval membership come out right through the model's finish with coef."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _mult_model as model  # noqa: E402


@pytest.fixture(scope="module")
def sk():
    from oracle import sc_oracle as o

    return o.PaillierKey.generate(512, random.Random(20260))


def _edges(w, signed):
    return [-(1 << (w - 1)), -1, (1 << (w - 1)) - 1, 0, 1] if signed else [0, 1, (1 << w) - 1]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("wx,wy", [(1, [1]), (32, [17]), (64, [64, 8]), (24, [23, 1, 40]), (16, [16, 1, 33, 7])])
def test_model_multiply_decrypts_to_the_product(sk, signed, wx, wy):
    rng = random.Random(wx * 100 + len(wy) + signed)
    n, kappa = sk.n, 40
    for x in _edges(wx, signed):
        for t in range(len(_edges(1, signed))):
            ys = [_edges(w, signed)[(t + j) % len(_edges(w, signed))] for j, w in enumerate(wy)]
            for r_a in (0, (1 << (wx + kappa)) - 1, None):
                draws = None
                if r_a is not None:            # the extreme draws: r_a at both ends, r_b all ones
                    draws = (r_a, [(1 << (w + kappa)) - 1 for w in wy], rng.randrange(1, n), [rng.randrange(1, n) for _ in wy])
                got = model.multiply(sk, x, ys, wx, wy, rng, signed, kappa, draws)
                assert got == [x * y % n for y in ys], (x, ys, r_a)


def test_model_flags_a_wider_layout(sk):
    rng = random.Random(3)
    n = sk.n
    r_a, r_bs, rho_p, rhos = model.draw(rng, 40, 64, [64], n)
    P = model.pack(sk, 40, 64, [64], False, model.enc(sk, (1 << 64) - 1), [model.enc(sk, (1 << 64) - 1)], (1 << 104) - 1, [(1 << 104) - 1], rho_p)
    assert model.mult(sk, 40, 64, [64], P, rhos)[2] is False
    assert model.mult(sk, 20, 16, [16], P, rhos)[2] is True


# (wx, wy, kappa) that put s = wx + kappa + 1 at 63, 64, 65, 96 and 318 bits
@pytest.mark.parametrize("wx,wy,kappa,s", [(22, (22,), 40, 63), (23, (23, 5), 40, 64), (24, (24,), 40, 65), (33, (1, 64, 17), 62, 96),
                                           (255, (255,), 62, 318), (32, (17, 5, 64, 1), 40, 73)])
@pytest.mark.parametrize("signed", [False, True])
def test_mul_layout_equals_the_model(wx, wy, kappa, s, signed):
    from protocols.secure_comparison_amd.multiplication import MulLayout

    lay = MulLayout(kappa, wx, wy, signed, 2048)
    ms, moffs, mfb, mend, mebits = model.layout(kappa, wx, list(wy), 2048)
    assert (lay.s, lay.offsets, lay.fbits, lay.end, lay.ebits) == (ms, moffs, mfb, mend, mebits)
    assert lay.s == s and lay.wy == tuple(wy) and lay.signed is signed
    assert lay.header == [kappa, wx, int(signed), len(wy), *wy]


def _both(kappa, wx, wy, nbits):
    from protocols.secure_comparison_amd.multiplication import MulLayout

    def fits(f):
        try:
            f()
            return True
        except ValueError:
            return False

    a, b = fits(lambda: MulLayout(kappa, wx, tuple(wy), False, nbits)), fits(lambda: model.layout(kappa, wx, list(wy), nbits))
    assert a == b, (kappa, wx, wy, nbits)
    return a


def test_mul_layout_raises_exactly_where_the_model_does():
    nbits, kappa = 1024, 40
    # the sum rule, three columns: s + sum fbits = wx + sum wy + 4 (kappa + 1) < 1023  <=>  wx + sum wy <= 858
    assert _both(kappa, 255, [255, 255, 93], nbits) is True         # 1022 bits: the last layout that fits
    assert _both(kappa, 255, [255, 255, 94], nbits) is False        # 1023: one bit over, through a column
    assert _both(kappa, 254, [255, 255, 94], nbits) is True
    assert _both(kappa, 255, [254, 255, 94], nbits) is True
    # four columns: wx + sum wy + 5 (kappa + 1) < 1023  <=>  wx + sum wy <= 817
    assert _both(kappa, 200, [200, 200, 200, 17], nbits) is True
    assert _both(kappa, 201, [200, 200, 200, 17], nbits) is False   # one bit over, through x
    # the product rule s + fbits_j < bits(N) - 1 is implied by the sum rule for every layout (a product's bits are a part of the
    # sum), and with one column the two are the same bound wx + wy + 2 kappa + 2 < bits(N) - 1.  Widths stop at 255, so on a 1024-bit N
    # a single column cannot reach it (255 + 255 + 126 = 636); the bound itself is probed one bit either side on small N
    assert _both(62, 255, [255], nbits) is True
    for nb in (299, 300, 301):
        assert _both(62, 87, [85], nb) is (87 + 85 + 126 < nb - 1)           # 298 bits
    assert _both(62, 87, [85], 299) is False and _both(62, 86, [85], 299) is True and _both(62, 87, [84], 299) is True    # 298 < 298 fails
    # arguments out of range
    for kw in ((0, 8, [8]), (63, 8, [8]), (40, 0, [8]), (40, 256, [8]), (40, 8, [0]), (40, 8, [256]), (40, 8, []), (40, 8, [1] * 5)):
        assert _both(*kw, 2048) is False


def test_mul_layout_names_the_column():
    from protocols.secure_comparison_amd.multiplication import MulLayout

    with pytest.raises(ValueError, match="column 2"):
        MulLayout(40, 255, (255, 255, 94), False, 1024)


@pytest.mark.parametrize("op,table", [("and", [0, 0, 0, 1]), ("or", [0, 1, 1, 1]), ("xor", [0, 1, 1, 0])])
def test_boolean_truth_tables_through_the_model(sk, op, table):
    rng = random.Random(11)
    assert [model.bit_op(sk, a, b, op, rng) for a in (0, 1) for b in (0, 1)] == table


def test_coef_without_base(sk):
    rng = random.Random(12)
    n, n2 = sk.n, sk.n2
    for coef in (1, -1, -2):
        x_c, y_c = model.enc(sk, 5, rng.randrange(1, n)), model.enc(sk, -7, rng.randrange(1, n))
        out = model.multiply_enc(sk, 40, 8, [8], True, x_c, [y_c], model.draw(rng, 40, 8, [8], n), None, coef)
        assert model.dec(sk, out[0]) == coef * -35 % n


@pytest.mark.parametrize("l", [1, 16, 64, 80])
def test_equal_and_in_range_through_the_model(sk, l):
    rng = random.Random(l)
    top = (1 << l) - 1
    pairs = [(0, 0), (top, top), (0, top), (top, 0), (top - 1, top), (top, top - 1), (0, 1), (1, 0)]
    for x, y in pairs:
        assert model.equal(sk, x, y, rng) == (int(x == y), int(x <= y), int(y <= x))
    lo, hi = (0, top) if l == 1 else (1, top - 1)
    for x in {lo, hi, max(lo - 1, 0), min(hi + 1, top), (lo + hi) // 2}:
        assert model.in_range(sk, x, lo, hi, rng) == int(lo <= x <= hi)


def test_exports_and_bindings():
    import protocols.secure_comparison_amd as pkg
    from protocols.secure_comparison_amd import _lib

    for name in ("MulLayout", "MulDraws", "draw_mul", "secure_multiply_batch", "secure_and_batch", "secure_or_batch", "secure_xor_batch",
                 "secure_equal_batch", "secure_in_range_batch"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("sc_mul_prep", "sc_mul_split", "sc_initiator_mul_pack", "sc_keyholder_mul", "sc_initiator_mul_finish"):
        assert name in _lib.SYMBOLS
    for cls in (pkg.Initiator, pkg.KeyHolder):
        assert hasattr(cls, "perform_secure_multiply_batch") and hasattr(cls, "perform_secure_equal_batch")

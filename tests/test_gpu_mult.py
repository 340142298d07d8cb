"""Secure multiplication on the GPU: the three steps bit for bit against the pure-Python model
(tests/_mult_model.py) with injected draws -- P, the exponent rows e, the products rab, the key holder's products and the result --
on every key size with a per-row pair instance, on a 512-bit key and with SC_KEY_NO_PAIRS (the fallback composition); decrypted
products, Boolean operations, equality and interval membership against Python; the refusals; the two players over a communicator;
and the selection's residues, which this feature must not change.

A batch has 100 rows (not a multiple of a wave's items).  The model is plain Python on big integers, so it follows a subset of the
rows -- edge rows and random ones, fewer on the larger keys -- bit for bit, while the plaintext arrays and the decryption of every
row are checked."""
import asyncio
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _mult_model as model  # noqa: E402
import _select_model as smodel  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA, COUNT = 40, 100


def _rows(engine, t):
    return engine.download(t.reshape(-1, t.shape[-1]).contiguous())


def _paillier(engine, sk, use_pairs=True):
    from protocols.secure_comparison_amd import Paillier

    bob = Paillier(sk.n, sk.p, sk.q, engine=engine, use_pairs=use_pairs)
    return bob.public_copy(), bob


_KEYS = {}


def _key(keys, bits):
    if bits not in _KEYS:
        if bits == 512:
            from oracle import sc_oracle as o

            _KEYS[bits] = o.PaillierKey.generate(512, random.Random(512))
        else:
            _KEYS[bits] = oracle_paillier(keys, bits)
    return _KEYS[bits]


def _edges(w, signed):
    return [-(1 << (w - 1)), -1, (1 << (w - 1)) - 1] if signed else [0, 1, (1 << w) - 1]


def _value(rng, w, signed):
    return rng.getrandbits(w) - ((1 << (w - 1)) if signed else 0)


def _case(rng, sk, kappa, wx, wy, signed, count):
    """Plaintext rows and draws: every (x, y) pair of edge values with r_a at both ends of its range and r_b all ones, then random
    rows.  Returns (xs, ys [nf][count], draws [count])."""
    n = sk.n
    xs, ys, draws = [], [[] for _ in wy], []
    ex = _edges(wx, signed)
    for x in ex:
        for t in range(3):
            for r_a in (0, (1 << (wx + kappa)) - 1):
                xs.append(x)
                for j, w in enumerate(wy):
                    ys[j].append(_edges(w, signed)[(t + j) % 3])
                draws.append((r_a, [(1 << (w + kappa)) - 1 for w in wy], rng.randrange(1, n), [rng.randrange(1, n) for _ in wy]))
    while len(xs) < count:
        xs.append(_value(rng, wx, signed))
        for j, w in enumerate(wy):
            ys[j].append(_value(rng, w, signed))
        draws.append(model.draw(rng, kappa, wx, wy, n))
    return xs[:count], [c[:count] for c in ys], draws[:count]


def _upload_draws(engine, ap, kappa, wx, wy, draws):
    from protocols.secure_comparison_amd.multiplication import MulDraws

    nw, nf = ap.mod_n.nwords, len(wy)
    aw, bw = (wx + kappa + 31) // 32, (max(wy) + kappa + 31) // 32
    return MulDraws(r_a=engine.upload([d[0] for d in draws], aw),
                    r_b=torch.stack([engine.upload([d[1][j] for d in draws], bw) for j in range(nf)]).contiguous(),
                    rho_p=engine.upload([d[2] for d in draws], nw),
                    rho_products=torch.stack([engine.upload([d[3][j] for d in draws], nw) for j in range(nf)]).contiguous())


def _enc(engine, sk, ap, rng, values):
    """Randomized encryptions of `values` (residues modulo N), made on the device: (the ciphertexts as Python ints, the array)."""
    n, nw = sk.n, ap.mod_n.nwords
    c = ap.randomize_batch(ap.encrypt_raw_batch(engine.upload([v % n for v in values], nw)),
                           engine.upload([rng.randrange(1, n) for _ in values], nw))
    return engine.download(c), c


def _encrypt(engine, sk, ap, rng, xs, ys):
    x_c, x_t = _enc(engine, sk, ap, rng, xs)
    cols = [_enc(engine, sk, ap, rng, col) for col in ys]
    return x_c, [c for c, _ in cols], x_t, torch.stack([t for _, t in cols]).contiguous()


def _model_rows(bits, count):
    """The rows the model follows (plain Python on big integers: about 1 ms, 80 ms and 250 ms per exponentiation at 1024, 2048 and
    3072 bits): the 18 edge rows -- thinned out on the larger keys, so that every x edge, every y rotation and both ends of r_a still
    occur -- and the last random rows."""
    if bits <= 1024:
        return list(range(18)) + list(range(count - 12, count))
    if bits <= 2048:
        return [0, 5, 10, 15] + list(range(count - 3, count))
    return [0, 7, 14] + list(range(count - 2, count))


def _steps(engine, sk, ap, bp, kappa, wx, wy, signed, seed, bits, count=COUNT, rows=None):
    from protocols.secure_comparison_amd.multiplication import MulLayout, mul_finish, mul_mult, mul_pack

    n, nf = sk.n, len(wy)
    rng = random.Random(seed)
    lay = MulLayout(kappa, wx, tuple(wy), signed, n.bit_length())
    xs, ys, draws = _case(rng, sk, kappa, wx, wy, signed, count)
    x_c, y_c, x_t, y_t = _encrypt(engine, sk, ap, rng, xs, ys)
    md = _upload_draws(engine, ap, kappa, wx, wy, draws)
    rows = _model_rows(bits, count) if rows is None else rows          # (rows: the rows the model follows, when the caller says)
    ycol = lambda i: [y_c[j][i] for j in range(nf)]  # noqa: E731

    P, (e, rab) = mul_pack(lay, x_t, y_t, md, ap)
    got_P = engine.download(P)
    want_P = {i: model.pack(sk, kappa, wx, wy, signed, x_c[i], ycol(i), draws[i][0], draws[i][1], draws[i][2]) for i in rows}
    assert [got_P[i] for i in rows] == [want_P[i] for i in rows]
    # the plaintext arrays of the finish: every row (cheap): e planes e_x_0 .. e_x_(nf-1), e_y; rab_j = e_x_j e_y
    assert e.shape == (nf + 1, count, (lay.ebits + 31) // 32) and rab.shape == (nf, count, ap.mod_n.nwords)
    pl = [model.plain(kappa, wx, wy, signed, d[0], d[1]) for d in draws]
    assert _rows(engine, e) == [pl[i][1][j] for j in range(nf) for i in range(count)] + [pl[i][0] for i in range(count)]
    assert _rows(engine, rab) == [pl[i][2][j] for j in range(nf) for i in range(count)]

    prods = mul_mult(lay, P, bp, md.rho_products)
    want = {i: model.mult(sk, kappa, wx, wy, want_P[i], draws[i][3]) for i in rows}
    got_prods = _rows(engine, prods)
    assert [got_prods[j * count + i] for j in range(nf) for i in rows] == [want[i][0][j] for j in range(nf) for i in rows]
    assert not any(want[i][2] for i in rows)

    out = mul_finish(lay, x_t, y_t, prods, (e, rab), ap)
    got = _rows(engine, out)
    want_out = {i: model.finish(sk, kappa, wx, wy, signed, x_c[i], ycol(i), want[i][0], draws[i][0], draws[i][1]) for i in rows}
    assert [got[j * count + i] for j in range(nf) for i in rows] == [want_out[i][j] for j in range(nf) for i in rows]
    dec = engine.download(bp.decrypt_raw_batch(out.reshape(nf * count, -1).contiguous()))
    assert dec == [xs[i] * ys[j][i] % n for j in range(nf) for i in range(count)]


# kappa = 40: (23, 23) and (24, 24) put s at 64 / 65 bits, the old one-word edge; (255, 255) at 296 bits (ten words)
@pytest.mark.parametrize("wx,wy,signed", [(1, [1], False), (1, [1], True), (23, [23], False), (24, [24], True), (32, [17], True),
                                          (64, [64], False), (255, [255], True), (255, [255], False)])
def test_steps_bit_exact_vs_model_widths(engine, keys, wx, wy, signed):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    _steps(engine, sk, ap, bp, KAPPA, wx, wy, signed, 1000 + wx + signed, 1024)


@pytest.mark.parametrize("bits,wx,wy,signed", [(2048, 32, [17], False), (2048, 255, [255], True), (3072, 64, [64], True),
                                               (3072, 23, [24], False)])
def test_steps_bit_exact_vs_model_keys(engine, keys, bits, wx, wy, signed):
    sk = _key(keys, bits)
    ap, bp = _paillier(engine, sk)
    _steps(engine, sk, ap, bp, KAPPA, wx, wy, signed, bits + wx, bits)


@pytest.mark.parametrize("bits,signed", [(1024, True), (2048, False)])
def test_steps_four_columns_at_unaligned_offsets(engine, keys, bits, signed):
    """Widths 32 | 17, 5, 64, 1 at kappa = 40: offsets 73, 131, 177, 282 -- none on a word boundary."""
    from protocols.secure_comparison_amd.multiplication import MulLayout

    assert [o % 32 for o in MulLayout(KAPPA, 32, (17, 5, 64, 1), signed, bits).offsets] == [9, 3, 17, 26]
    sk = _key(keys, bits)
    ap, bp = _paillier(engine, sk)
    _steps(engine, sk, ap, bp, KAPPA, 32, [17, 5, 64, 1], signed, 4, bits)


def test_steps_on_a_512_bit_key(engine, keys):
    """No per-row pair instance for this modulus: the entries compose exponentiations modulo N^2 themselves."""
    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    _steps(engine, sk, ap, bp, KAPPA, 32, [17, 24], True, 512, 512)


def test_steps_with_sc_key_no_pairs(engine, keys):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk, use_pairs=False)
    _steps(engine, sk, ap, bp, KAPPA, 24, [64, 23], True, 77, 1024)


def test_kappa_at_both_ends(engine, keys):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    _steps(engine, sk, ap, bp, 1, 62, [1, 33], False, 5, 1024)           # s = 64
    _steps(engine, sk, ap, bp, 62, 33, [64], True, 6, 1024)             # s = 96


# ---- decrypted results ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True])
def test_secure_multiply_batch_and_square(engine, keys, signed):
    from protocols.secure_comparison_amd import secure_multiply_batch

    sk = _key(keys, 2048)
    ap, bp = _paillier(engine, sk)
    rng = random.Random(9 + signed)
    n, w = sk.n, 32
    xs, ys, _ = _case(rng, sk, KAPPA, w, [w, 17], signed, COUNT)
    _, _, x_t, y_t = _encrypt(engine, sk, ap, rng, xs, ys)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    out = secure_multiply_batch(x_t, y_t, w, (w, 17), ap, bp, signed=signed)
    assert out.shape == y_t.shape
    assert dec(out) == [x * y % n for col in ys for x, y in zip(xs, col)]
    one = secure_multiply_batch(x_t, y_t[0].contiguous(), w, w, ap, bp, signed=signed)
    assert one.shape == x_t.shape and dec(one) == [x * y % n for x, y in zip(xs, ys[0])]
    sq = secure_multiply_batch(x_t, x_t, w, w, ap, bp, signed=signed)          # y is the same tensor as x
    assert dec(sq) == [x * x % n for x in xs]


@pytest.mark.parametrize("coef", [-1, -2])
@pytest.mark.parametrize("with_base", [False, True])
def test_finish_with_coef_and_base(engine, keys, coef, with_base):
    from protocols.secure_comparison_amd.multiplication import MulLayout, mul_finish, mul_mult, mul_pack

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, n2, wx, wy, nf = sk.n, sk.n2, 16, [16, 9], 2
    rng = random.Random(100 + coef + with_base)
    lay = MulLayout(KAPPA, wx, tuple(wy), True, n.bit_length())
    xs, ys, draws = _case(rng, sk, KAPPA, wx, wy, True, COUNT)
    x_c, y_c, x_t, y_t = _encrypt(engine, sk, ap, rng, xs, ys)
    md = _upload_draws(engine, ap, KAPPA, wx, wy, draws)
    bs = [[rng.getrandbits(40) for _ in range(COUNT)] for _ in range(nf)]
    b_c, b_t = zip(*[_enc(engine, sk, ap, rng, col) for col in bs])
    b_t = torch.stack(b_t).contiguous() if with_base else None
    P, plain = mul_pack(lay, x_t, y_t, md, ap)
    prods = mul_mult(lay, P, bp, md.rho_products)
    out = mul_finish(lay, x_t, y_t, prods, plain, ap, b_t, coef)
    got = _rows(engine, out)
    got_prods = _rows(engine, prods)
    for i in range(COUNT):
        want = model.finish(sk, KAPPA, wx, wy, True, x_c[i], [y_c[0][i], y_c[1][i]], [got_prods[i], got_prods[COUNT + i]], draws[i][0],
                            draws[i][1], [b_c[0][i], b_c[1][i]] if with_base else None, coef)
        assert [got[i], got[COUNT + i]] == want, i
    dec = engine.download(bp.decrypt_raw_batch(out.reshape(nf * COUNT, -1).contiguous()))
    assert dec == [((bs[j][i] if with_base else 0) + coef * xs[i] * ys[j][i]) % n for j in range(nf) for i in range(COUNT)]


def test_and_or_xor_truth_tables(engine, keys):
    from protocols.secure_comparison_amd import secure_and_batch, secure_or_batch, secure_xor_batch

    sk = _key(keys, 2048)
    ap, bp = _paillier(engine, sk)
    rng = random.Random(21)
    a = [0, 0, 1, 1] * 25
    b = [0, 1, 0, 1] * 25
    a_t, b_t = _enc(engine, sk, ap, rng, a)[1], _enc(engine, sk, ap, rng, b)[1]
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t))  # noqa: E731
    assert dec(secure_and_batch(a_t, b_t, ap, bp)) == [x & y for x, y in zip(a, b)]
    assert dec(secure_or_batch(a_t, b_t, ap, bp)) == [x | y for x, y in zip(a, b)]
    assert dec(secure_xor_batch(a_t, b_t, ap, bp)) == [x ^ y for x, y in zip(a, b)]


# ---- comparison-based calls ------------------------------------------------------------------------------------------------------------
def _players(engine, keys, l):
    from protocols.secure_comparison_amd import DGK

    if l <= 16:
        pbits, dk = 1024, oracle_dgk(keys, "dgk_1024_l16")
    elif l <= 64:
        pbits, dk = 2048, oracle_dgk(keys, "dgk_2048_l64")
    else:
        import json

        from conftest import GOLDEN
        from oracle import sc_oracle as o

        k = json.load(open(os.path.join(GOLDEN, "keys_wide.json")))["dgk_2048_l128"]
        p, q = int(k["p"], 16), int(k["q"], 16)
        pbits, dk = 2048, o.DGKKey(p * q, int(k["g"], 16), int(k["h"], 16), int(k["u"], 16), k["t"], p, q, int(k["v_p"], 16), int(k["v_q"], 16))
    sk = _key(keys, pbits)
    ap, bp = _paillier(engine, sk)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=engine, randomizer_bits=400)
    return sk, ap, bd.public_copy(), bp, bd


def _equal_rows(l, rng, B=24):
    """x = y, x = y +- 1, both extremes, negative pairs (the comparison reads y - x alone: |y - x| < 2^l), then random rows."""
    top = (1 << l) - 1
    mid = rng.getrandbits(l) if l > 1 else 1
    rows = [(0, 0), (top, top), (0, top), (top, 0), (mid, mid), (-1, -1), (-5, -5), (-5, -4), (-4, -5), (-1, 0), (0, -1)]
    if l > 1:
        rows += [(mid, mid + 1) if mid < top else (mid - 1, mid), (mid + 1, mid) if mid < top else (mid, mid - 1), (top - 1, top), (1, 0)]
    while len(rows) < B:
        x = rng.getrandbits(l)
        rows.append((x, x) if rng.random() < 0.3 else (x, rng.getrandbits(l)))
    return rows[:B]


@pytest.mark.parametrize("l", [1, 16, 64, 80])
def test_secure_equal_batch(engine, keys, l):
    from protocols.secure_comparison_amd import secure_equal_batch

    sk, ap, ad, bp, bd = _players(engine, keys, l)
    rng = random.Random(l)
    rows = _equal_rows(l, rng)
    x_t, y_t = _enc(engine, sk, ap, rng, [x for x, _ in rows])[1], _enc(engine, sk, ap, rng, [y for _, y in rows])[1]
    eq, le, ge = secure_equal_batch(x_t, y_t, l, ap, ad, bp, bd)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.contiguous()))  # noqa: E731
    assert dec(eq) == [int(x == y) for x, y in rows]
    assert dec(le) == [int(x <= y) for x, y in rows]
    assert dec(ge) == [int(y <= x) for x, y in rows]


@pytest.mark.parametrize("l", [1, 16, 64])
def test_secure_in_range_batch(engine, keys, l):
    from protocols.secure_comparison_amd import secure_in_range_batch

    sk, ap, ad, bp, bd = _players(engine, keys, l)
    rng = random.Random(50 + l)
    top = (1 << l) - 1
    lo, hi = (0, top) if l == 1 else (3, top - 2)
    rows = [(lo, lo, hi), (hi, lo, hi), ((lo + hi) // 2, lo, hi), (lo, lo, lo), (0, 0, top), (top, 0, top)]       # on and inside the bounds
    if l > 1:
        rows += [(lo - 1, lo, hi), (hi + 1, lo, hi), (lo + 1, lo, hi), (hi - 1, lo, hi), (0, lo, hi), (top, lo, hi), (5, 6, 4)]
    while len(rows) < 24:
        a, b = sorted((rng.getrandbits(l), rng.getrandbits(l)))
        rows.append((rng.getrandbits(l), a, b))
    up = lambda k: _enc(engine, sk, ap, rng, [r[k] for r in rows])[1]  # noqa: E731
    out = secure_in_range_batch(up(0), up(1), up(2), l, ap, ad, bp, bd)
    assert engine.download(bp.decrypt_raw_batch(out)) == [int(lo_ <= x <= hi_) for x, lo_, hi_ in rows]


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_a_layout_that_does_not_fit_is_refused_before_any_launch(engine, keys):
    from protocols.secure_comparison_amd import secure_multiply_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    nw, B = ap.mod_n.nwords, 4
    x_t = engine.upload([model.enc(sk, 1)] * B, 2 * nw)
    y_t = torch.stack([x_t, x_t, x_t]).contiguous()
    with pytest.raises(ValueError, match="column 2"):
        secure_multiply_batch(x_t, y_t, 255, (255, 255, 94), ap, bp)
    assert secure_multiply_batch(x_t, y_t, 255, (255, 255, 93), ap, bp).shape == y_t.shape        # one bit less fits
    # the library's own copy of the rule (SC_ERR_ARG), with nothing launched: no interpreter launch, no output word written
    wy = [255, 255, 94]
    r_a, r_b, rho = engine.upload([1] * B, 10), torch.stack([engine.upload([1] * B, 10)] * 3).contiguous(), engine.upload([2] * B, nw)
    before = dict(engine.launch_counts())
    sentinel = 0x5A5A5A5A
    P = torch.full((B, 2 * nw), sentinel, dtype=torch.int32, device=engine.device)
    e = torch.full((4, B, 10), sentinel, dtype=torch.int32, device=engine.device)
    rab = torch.full((3, B, nw), sentinel, dtype=torch.int32, device=engine.device)
    _, pw = engine._widths(wy)
    rc = engine.lib.sc_initiator_mul_pack(engine.ctx, ap.key.id, KAPPA, 255, 3, pw, 0, engine._ptr(x_t), engine._ptr(y_t), engine._ptr(r_a), 10,
                                          engine._ptr(r_b), 10, engine._ptr(rho), 10, engine._ptr(P), engine._ptr(e), engine._ptr(rab), B)
    assert rc == -1 and b"column 2" in engine.lib.sc_last_error(engine.ctx)
    engine.synchronize()
    assert dict(engine.launch_counts()) == before
    assert all(bool((t == sentinel).all()) for t in (P, e, rab))
    with pytest.raises(ValueError, match="column 2"):
        engine.keyholder_mul(bp.key, KAPPA, 255, wy, x_t, torch.zeros((3, B, nw), dtype=torch.int32, device=engine.device))
    with pytest.raises(ValueError, match="column 2"):
        engine.initiator_mul_finish(ap.key, KAPPA, 255, wy, x_t, y_t, y_t, e, rab)


def test_a_null_rho_p_is_refused(engine, keys):
    from protocols.secure_comparison_amd.multiplication import MulDraws, MulLayout, draw_mul, mul_pack

    sk = _key(keys, 1024)
    ap, _ = _paillier(engine, sk)
    lay = MulLayout(KAPPA, 8, (8,), False, 1024)
    x_t = engine.upload([model.enc(sk, 3)] * 4, ap.mod_n2.nwords)
    d = draw_mul(4, lay, ap)
    with pytest.raises(ValueError, match="rho_p is required"):
        mul_pack(lay, x_t, x_t, MulDraws(d.r_a, d.r_b, None, None), ap)


def test_mul_mult_refuses_a_wider_layout(engine, keys):
    from protocols.secure_comparison_amd.multiplication import MulLayout, draw_mul, mul_mult, mul_pack

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    big, small = MulLayout(40, 64, (64,), False, 1024), MulLayout(20, 16, (16,), False, 1024)
    B, nw = 8, ap.mod_n.nwords
    x_t = engine.upload([model.enc(sk, (1 << 64) - 1)] * B, 2 * nw)
    db = draw_mul(B, big, ap)
    db.r_a = engine.upload([(1 << 104) - 1] * B, 4)                     # the top field certainly reaches past the small layout's end
    db.r_b = engine.upload([(1 << 104) - 1] * B, 4).unsqueeze(0).contiguous()
    P, _ = mul_pack(big, x_t, x_t, db, ap)
    rho = draw_mul(B, small, ap).rho_products
    out = torch.empty((1, B, 2 * nw), dtype=torch.int32, device=engine.device)
    _, pw = engine._widths(small.wy)
    rc = engine.lib.sc_keyholder_mul(engine.ctx, bp.key.id, small.kappa, small.wx, 1, pw, engine._ptr(P), engine._ptr(rho), engine._ptr(out), B)
    assert rc == -5                                                     # SC_ERR_LAYOUT
    with pytest.raises(ValueError, match="exceeds the announced field layout"):
        mul_mult(small, P, bp, rho)
    assert mul_mult(big, P, bp, db.rho_products).shape == (1, B, 2 * nw)       # and the verdict word is clean again


def test_a_non_invertible_product_names_its_flat_index(engine, keys):
    from protocols.secure_comparison_amd.engine import NotInvertibleError
    from protocols.secure_comparison_amd.multiplication import MulLayout, draw_mul, mul_finish, mul_mult, mul_pack

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = MulLayout(KAPPA, 8, (8, 8), False, 1024)
    B = 10
    x_t = engine.upload([model.enc(sk, 3 + i, 7 + i) for i in range(B)], ap.mod_n2.nwords)
    y_t = torch.stack([x_t, x_t]).contiguous()
    d = draw_mul(B, lay, ap)
    P, plain = mul_pack(lay, x_t, y_t, d, ap)
    prods = mul_mult(lay, P, bp, d.rho_products)
    bad = prods.clone()
    bad[1, 7] = engine.upload([sk.p], ap.mod_n2.nwords)[0]             # shares the factor p with N^2
    with pytest.raises(NotInvertibleError) as err:
        mul_finish(lay, x_t, y_t, bad, plain, ap, None, -1)
    assert err.value.index == 1 * B + 7
    got = engine.download(bp.decrypt_raw_batch(mul_finish(lay, x_t, y_t, prods, plain, ap, None, -1).reshape(2 * B, -1).contiguous()))
    assert got == [-(3 + i) ** 2 % sk.n for i in range(B)] * 2


# ---- two players over a communicator ------------------------------------------------------------------------------------------------
def _two_players(engine, keys, l, timeout_s=600.0):
    from protocols.secure_comparison_amd import InMemoryCommunicator, Initiator, KeyHolder

    sk, ap, ad, bp, bd = _players(engine, keys, l)
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=timeout_s)
    alice = Initiator(l, communicator=comm, other_party="keyholder")
    bob = KeyHolder(l, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    return sk, ap, bp, alice, bob


def test_players_multiply_and_equal(engine, keys):
    sk, ap, bp, alice, bob = _two_players(engine, keys, 16)
    rng = random.Random(41)
    n = sk.n
    xs, ys, _ = _case(rng, sk, KAPPA, 16, [16, 7], True, 40)
    _, _, x_t, y_t = _encrypt(engine, sk, ap, rng, xs, ys)
    rows = _equal_rows(16, rng)
    ex, ey = _enc(engine, sk, ap, rng, [x for x, _ in rows])[1], _enc(engine, sk, ap, rng, [y for _, y in rows])[1]

    async def run():
        prod, _ = await asyncio.gather(alice.perform_secure_multiply_batch(x_t, y_t, 16, (16, 7), signed=True, engine=engine),
                                       bob.perform_secure_multiply_batch(16, (16, 7), signed=True))
        three, _ = await asyncio.gather(alice.perform_secure_equal_batch(ex, ey, engine=engine), bob.perform_secure_equal_batch())
        return prod, three

    prod, (eq, le, ge) = asyncio.run(run())
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    assert dec(prod) == [x * y % n for col in ys for x, y in zip(xs, col)]
    assert dec(eq) == [int(x == y) for x, y in rows]
    assert dec(le) == [int(x <= y) for x, y in rows] and dec(ge) == [int(y <= x) for x, y in rows]


@pytest.mark.parametrize("theirs", [dict(kappa=50), dict(x_bits=15), dict(signed=False), dict(y_bits=(16, 8))])
def test_key_holder_refuses_a_different_header(engine, keys, theirs):
    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, timeout_s=30.0)
    nw2 = ap.mod_n2.nwords
    x_t = engine.upload([model.enc(sk, 5)] * 8, nw2)
    y_t = torch.stack([x_t, x_t]).contiguous()
    his = dict(x_bits=16, y_bits=(16, 7), signed=True, kappa=40)
    his.update(theirs)

    async def run():          # the key holder refuses on his own; the initiator, still waiting for products, is cancelled: no time limit runs out
        a = asyncio.ensure_future(alice.perform_secure_multiply_batch(x_t, y_t, 16, (16, 7), signed=True, kappa=40, engine=engine))
        (got,) = await asyncio.gather(bob.perform_secure_multiply_batch(**his), return_exceptions=True)
        pending = not a.done()
        a.cancel()
        await asyncio.gather(a, return_exceptions=True)
        return got, pending

    got_b, alice_waits = asyncio.run(run())
    assert isinstance(got_b, ValueError) and "announces" in str(got_b)
    assert alice_waits                               # the initiator never gets products back


def test_chunked_sessions_raise(engine, keys):
    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, timeout_s=30.0)
    x_t = engine.upload([model.enc(sk, 5)] * 8, ap.mod_n2.nwords)
    with pytest.raises(ValueError, match="chunks"):
        asyncio.run(alice.perform_secure_multiply_batch(x_t, x_t, 8, 8, chunks=2, engine=engine))
    with pytest.raises(ValueError, match="chunks"):
        asyncio.run(alice.perform_secure_equal_batch(x_t, x_t, chunks=2, engine=engine))


# ---- existing paths unchanged ---------------------------------------------------------------------------------------------------------
def test_selection_minimum_and_compare_exchange_residues_are_unchanged(engine, keys):
    """With injected draws the selection's steps give the residues tests/_select_model.py gives: select_batch on its own, the selection
    of a minimum (sigma = [[1 - delta]] after a real comparison) and both outputs of a compare-exchange."""
    from protocols.secure_comparison_amd import selection as sel
    from protocols.secure_comparison_amd.sorting import cx_finish

    l, B, kappa = 16, 40, 40
    sk, ap, ad, bp, bd = _players(engine, keys, l)
    n, n2, nw = sk.n, sk.n2, ap.mod_n.nwords
    rng = random.Random(2)
    lay = sel.SelectLayout(l, kappa, (), n.bit_length())
    xs = [0, 65535, 7, 7] + [rng.getrandbits(l) for _ in range(B - 4)]
    ys = [65535, 0, 7, 8] + [rng.getrandbits(l) for _ in range(B - 4)]
    (x_c, x_t), (y_c, y_t) = _enc(engine, sk, ap, rng, xs), _enc(engine, sk, ap, rng, ys)
    draws = [smodel.draw(rng, kappa, [l], n) for _ in range(B)]
    bw = (max(lay.fbits) + 31) // 32
    sd = sel.SelectDraws(r_a=engine.upload([d[0] for d in draws], 2), r_b=engine.upload([d[1][0] for d in draws], bw).unsqueeze(0).contiguous(),
                         rho_p=engine.upload([d[2] for d in draws], nw), rho_products=engine.upload([d[3][0] for d in draws], nw).unsqueeze(0).contiguous())
    delta, d = sel._compare(x_t, y_t, l, ap, ad, bp, bd, None)
    sigma = sel._one_minus(ap, delta)
    delta_c, d_c, sigma_c = engine.download(delta), engine.download(d), engine.download(sigma)
    # select_batch = the minimum's selection
    out = sel.select_batch(lay, sigma, d.unsqueeze(0), x_t.unsqueeze(0), ap, bp, sd)
    want = [smodel.select(sk, kappa, [l], sigma_c[i], [d_c[i]], [x_c[i]], draws[i])[0] for i in range(B)]
    assert _rows(engine, out) == want
    assert engine.download(bp.decrypt_raw_batch(out[0])) == [min(x, y) for x, y in zip(xs, ys)]
    # the compare-exchange: hi = F ab T^-1 (the selection's finish with base F), lo = G T ab^-1
    P, plain = sel.select_pack(lay, delta, d.unsqueeze(0), sd, ap)
    prods = sel.select_mult(lay, P, bp, sd.rho_products)
    both = cx_finish(lay, delta, d.unsqueeze(0), x_t.unsqueeze(0), y_t.unsqueeze(0), prods, plain, sd, ap)
    pc = _rows(engine, prods)
    assert engine.download(P) == [smodel.pack(sk, kappa, [l], delta_c[i], [d_c[i]], draws[i][0], draws[i][1], draws[i][2]) for i in range(B)]
    hi = [smodel.finish(sk, kappa, [l], delta_c[i], [d_c[i]], [x_c[i]], [pc[i]], draws[i][0], draws[i][1])[0] for i in range(B)]
    t_inv = [smodel.finish(sk, kappa, [l], delta_c[i], [d_c[i]], [1], [1], draws[i][0], draws[i][1])[0] for i in range(B)]
    lo = [y_c[i] * pow(t_inv[i], -1, n2) % n2 * pow(pc[i], -1, n2) % n2 for i in range(B)]
    assert engine.download(both[0, 0]) == lo and engine.download(both[1, 0]) == hi

"""Secure inner product on the GPU: every step bit for bit against the pure-Python model (tests/_dot_model.py) with
injected draws -- the exponent planes e, the packed masks R, S, the messages P, the key holder's [[D]] and the result -- on 1024-bit
keys (g = 7 at kappa = 40, w = 32) for the smallest k that reach each path, on a 2048-bit key, a 512-bit key and with
SC_KEY_NO_PAIRS; the refusals; coef with a base; the squared distance; the two players over a communicator; the library's own draws;
and the selection's and the multiplication's residues, which this feature must not change.

A batch has 100 rows (not a multiple of a wave).  The plaintext arrays and the decryption are checked on every row; the model's
ciphertexts (plain Python on big integers) on the edge rows and the last random ones, fewer on the 2048-bit key."""
import asyncio
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _dot_model as model  # noqa: E402
import _draw_replay as dr  # noqa: E402
import _mult_model as mmodel  # noqa: E402
import _select_model as smodel  # noqa: E402
from oracle import chacha_rng as cr  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA, COUNT = 40, 100
KEY = bytes((5 * i + 9) & 0xFF for i in range(32))


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


def _case(rng, sk, kappa, wx, wy, signed, square, k, count):
    """Plaintext rows and draws.  Rows 0 .. 5: every element at one edge value -- for signed vectors -2^(w-1), -1 and 2^(w-1) - 1 --
    with all masks at 0 and at their maximum (the carries of S and D run through the high words); rows 6 .. 8: the edges rotating
    along the vector under random masks; then random rows.  Returns (xs [k][count], ys [k][count] or None, draws [count])."""
    n = sk.n
    M = model.layout(kappa, wx, wy, square, k, n.bit_length())[4]
    ex, ey = _edges(wx, signed), (None if square else _edges(wy, signed))
    rows = []
    for v in range(3):
        for fill in (0, 1):
            xs = [ex[v]] * k
            ys = None if square else [ey[v]] * k
            draws = ([fill * ((1 << (wx + kappa)) - 1)] * k, None if square else [fill * ((1 << (wy + kappa)) - 1)] * k,
                     [rng.randrange(1, n) for _ in range(M)], rng.randrange(1, n))
            rows.append((xs, ys, draws))
    for t in range(3):
        rows.append(([ex[(t + j) % 3] for j in range(k)], None if square else [ey[(t + 2 * j) % 3] for j in range(k)],
                     model.draw(rng, kappa, wx, wy, square, k, n)))
    while len(rows) < count:
        rows.append(([_value(rng, wx, signed) for _ in range(k)], None if square else [_value(rng, wy, signed) for _ in range(k)],
                     model.draw(rng, kappa, wx, wy, square, k, n)))
    rows = rows[:count]
    xs = [[r[0][j] for r in rows] for j in range(k)]
    ys = None if square else [[r[1][j] for r in rows] for j in range(k)]
    return xs, ys, [r[2] for r in rows]


def _upload_draws(engine, ap, lay, draws):
    from protocols.secure_comparison_amd import DotDraws

    nw, k, M = ap.mod_n.nwords, lay.k, lay.M
    aw, bw = (lay.wx + lay.kappa + 31) // 32, (lay.wy + lay.kappa + 31) // 32
    planes = lambda f, cnt, w: torch.stack([engine.upload([f(d, j) for d in draws], w) for j in range(cnt)]).contiguous()  # noqa: E731
    return DotDraws(r_a=planes(lambda d, j: d[0][j], k, aw), r_b=None if lay.square else planes(lambda d, j: d[1][j], k, bw),
                    rho_p=planes(lambda d, j: d[2][j], M, nw), rho_d=engine.upload([d[3] for d in draws], nw))


def _enc(engine, sk, ap, rng, values):
    """Randomized encryptions of `values` (residues modulo N), made on the device: (the ciphertexts as Python ints, the array)."""
    n, nw = sk.n, ap.mod_n.nwords
    c = ap.randomize_batch(ap.encrypt_raw_batch(engine.upload([v % n for v in values], nw)),
                           engine.upload([rng.randrange(1, n) for _ in values], nw))
    return engine.download(c), c


def _enc_planes(engine, sk, ap, rng, cols):
    """cols [k][count] -> (ints [k][count], array [k][count][2nw]): one encryption launch for all of them."""
    k, count = len(cols), len(cols[0])
    ints, t = _enc(engine, sk, ap, rng, [v for col in cols for v in col])
    return [ints[j * count:(j + 1) * count] for j in range(k)], t.reshape(k, count, -1).contiguous()


def _model_rows(bits, count):
    """The rows the model follows: at 1024 bits the nine edge rows and the last three; thinned on the larger keys."""
    if bits <= 1024:
        return list(range(9)) + list(range(count - 3, count))
    return [1, 4, 7, count - 1]


def _layout(sk, kappa, wx, wy, signed, square, k):
    from protocols.secure_comparison_amd import DotLayout

    return DotLayout(kappa, wx, wy, k, signed, square, sk.n.bit_length())


def _prep_raw(engine, sk, ap, lay, md, count):
    """sc_dot_prep itself (the dev entry): (e, R, S) for every row."""
    nw, k = ap.mod_n.nwords, lay.k
    ew = (lay.ebits + 31) // 32
    _, pn = engine._host_n_words(sk.n, nw)
    e = torch.empty((k if lay.square else 2 * k, count, ew), dtype=torch.int32, device=engine.device)
    R = torch.empty((lay.M, count, nw), dtype=torch.int32, device=engine.device)
    S = engine.empty(count, nw)
    engine._sync_stream()
    rc = engine.lib.sc_dot_prep(engine.ctx, pn, nw, lay.kappa, lay.wx, lay.wy, int(lay.signed), int(lay.square), k, engine._ptr(md.r_a),
                                md.r_a.shape[-1], engine._ptr(md.r_b), 0 if lay.square else md.r_b.shape[-1], ew, engine._ptr(e), engine._ptr(R),
                                engine._ptr(S), count)
    assert rc == 0, engine.lib.sc_last_error(engine.ctx)
    return e, R, S


def _split_raw(engine, sk, ap, lay, P_plain, count):
    """sc_dot_split itself on plaintext messages [M][count][nw]: (D, bad)."""
    nw = ap.mod_n.nwords
    _, pn = engine._host_n_words(sk.n, nw)
    D = engine.empty(count, nw)
    bad = torch.zeros(1, dtype=torch.int32, device=engine.device)
    engine._sync_stream()
    rc = engine.lib.sc_dot_split(engine.ctx, pn, nw, lay.kappa, lay.wx, lay.wy, int(lay.square), lay.k, engine._ptr(P_plain), engine._ptr(D),
                                 engine._ptr(bad), count)
    assert rc == 0, engine.lib.sc_last_error(engine.ctx)
    engine.synchronize()
    return D, int(bad.item())


def _steps(engine, sk, ap, bp, kappa, wx, wy, signed, square, k, seed, bits, count=COUNT, rows=None):
    from protocols.secure_comparison_amd.dotproduct import dot_finish, dot_pack, dot_sum

    n, nw = sk.n, ap.mod_n.nwords
    rng = random.Random(seed)
    lay = _layout(sk, kappa, wx, wy, signed, square, k)
    M = lay.M
    xs, ys, draws = _case(rng, sk, kappa, wx, wy, signed, square, k, count)
    x_c, x_t = _enc_planes(engine, sk, ap, rng, xs)
    y_c, y_t = (None, None) if square else _enc_planes(engine, sk, ap, rng, ys)
    md = _upload_draws(engine, ap, lay, draws)
    rows = _model_rows(bits, count) if rows is None else rows          # (rows: the rows the model follows, when the caller says)
    xv = lambda i: [x_c[j][i] for j in range(k)]  # noqa: E731
    yv = lambda i: None if square else [y_c[j][i] for j in range(k)]  # noqa: E731

    # the plaintext arrays, every row: sc_dot_prep's e, R, S against the model
    pl = [model.plain(kappa, wx, wy, signed, square, k, n.bit_length(), d[0], d[1]) for d in draws]
    planes = k if square else 2 * k
    e_raw, R_raw, S_raw = _prep_raw(engine, sk, ap, lay, md, count)
    assert _rows(engine, e_raw) == [pl[i][0][p] for p in range(planes) for i in range(count)]
    assert _rows(engine, R_raw) == [pl[i][1][m] for m in range(M) for i in range(count)]
    assert engine.download(S_raw) == [pl[i][2] for i in range(count)]
    # sc_dot_split on the plaintexts the key holder will see: D for every row, the verdict word clean
    want_D = []
    for i in range(count):
        a, b = model.masks(kappa, wx, wy, signed, square, draws[i][0], draws[i][1])
        A = [xs[j][i] + a[j] for j in range(k)]
        want_D.append(sum(v * v for v in A) if square else sum(v * (ys[j][i] + b[j]) for j, v in enumerate(A)))
    plain_P = []
    for m in range(M):
        for i in range(count):
            p = pl[i][1][m]
            for j in model.members(m, k, M):
                t = j // M
                p += xs[j][i] << (t * lay.pb)
                if not square:
                    p += ys[j][i] << (t * lay.pb + lay.sa)
            plain_P.append(p)
    assert all(0 <= p < n for p in plain_P)
    D_raw, bad = _split_raw(engine, sk, ap, lay, engine.upload(plain_P, nw).reshape(M, count, nw).contiguous(), count)
    assert engine.download(D_raw) == want_D and bad == 0

    # the three scheme-level steps
    P, (e, S) = dot_pack(lay, x_t, y_t, md, ap)
    assert P.shape == (M, count, 2 * nw) and e.shape == (planes, count, (lay.ebits + 31) // 32) and S.shape == (count, nw)
    assert torch.equal(e, e_raw) and torch.equal(S, S_raw)
    got_P = _rows(engine, P)
    want_P = {i: model.pack(sk, kappa, wx, wy, signed, square, xv(i), yv(i), draws[i][0], draws[i][1], draws[i][2]) for i in rows}
    assert [got_P[m * count + i] for m in range(M) for i in rows] == [want_P[i][m] for m in range(M) for i in rows]

    d_enc = dot_sum(lay, P, bp, md.rho_d)
    got_D = engine.download(d_enc)
    want = {i: model.answer(sk, kappa, wx, wy, square, k, want_P[i], draws[i][3]) for i in rows}
    assert [got_D[i] for i in rows] == [want[i][0] for i in rows]
    assert [want[i][1] for i in rows] == [want_D[i] for i in rows] and not any(want[i][2] for i in rows)

    out = dot_finish(lay, x_t, y_t, d_enc, (e, S), ap)
    got = engine.download(out)
    want_out = {i: model.finish(sk, kappa, wx, wy, signed, square, xv(i), yv(i), want[i][0], draws[i][0], draws[i][1]) for i in rows}
    assert [got[i] for i in rows] == [want_out[i] for i in rows]
    dec = engine.download(bp.decrypt_raw_batch(out))
    assert dec == [sum(xs[j][i] * (xs[j][i] if square else ys[j][i]) for j in range(k)) % n for i in range(count)]
    return lay


# ---- 1024-bit keys, kappa = 40, w = 32: g = 7 ---------------------------------------------------------------------------------------------
def test_k1_equals_the_multiplication_under_the_same_masks(engine, keys):
    """One pair: the same message, the same product, the same residue as secure_multiply_batch with (r_a, r_b, rho_p, rho)."""
    from protocols.secure_comparison_amd import secure_dot_batch, secure_multiply_batch
    from protocols.secure_comparison_amd.multiplication import MulDraws

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 32, 32, True, False, 1, 101, 1024)
    assert (lay.g, lay.M) == (7, 1)
    rng = random.Random(102)
    xs, ys, draws = _case(rng, sk, KAPPA, 32, 32, True, False, 1, COUNT)
    (_, x_t), (_, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
    md = _upload_draws(engine, ap, lay, draws)
    got = secure_dot_batch(x_t, y_t, 32, 32, ap, bp, signed=True, draws=md)
    mul = secure_multiply_batch(x_t[0].contiguous(), y_t[0].contiguous(), 32, 32, ap, bp, signed=True,
                                draws=MulDraws(md.r_a[0].contiguous(), md.r_b.contiguous(), md.rho_p[0].contiguous(), md.rho_d.unsqueeze(0).contiguous()))
    assert torch.equal(got, mul)


@pytest.mark.parametrize("k,M,signed", [(7, 1, False), (8, 2, True), (17, 3, True)])
def test_steps_bit_exact_vs_model(engine, keys, k, M, signed):
    """k = 7: one full message.  k = 8: the second message holds one pair, so the two ends differ.  k = 17: three messages, a partial
    top position (messages 0 and 1 hold three pairs, message 2 two) and T from groups of 3 + 3 + 3 + 3 + 3 + 2 planes per side."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 32, 32, signed, False, k, 200 + k, 1024)
    assert (lay.g, lay.M) == (7, M)


@pytest.mark.parametrize("k,M", [(1, 1), (14, 1), (15, 2)])
def test_steps_square_mode(engine, keys, k, M):
    """k = 1: a message of one field, so the blinded [[x + R]] rho_p^N is P itself and no squaring follows."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 32, 0, True, True, k, 300 + k, 1024)
    assert (lay.g, lay.M, lay.pb, lay.ebits) == (14, M, 73, 74)


@pytest.mark.parametrize("wx,wy,kappa,k,signed", [(255, 200, 40, 3, True), (1, 1, 40, 9, False), (1, 1, 40, 3, True), (20, 33, 62, 6, True)])
def test_steps_widths_and_kappa(engine, keys, wx, wy, kappa, k, signed):
    """(255, 200): g = 1, every field multi-word and unaligned (sa = 296, sb = 241).  (1, 1): pb = 84, g = 12.  kappa = 62:
    sa = 83, sb = 96, g = 5, so k = 6 takes two messages."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, kappa, wx, wy, signed, False, k, 400 + wx + k, 1024)
    assert lay.g == {255: 1, 1: 12, 20: 5}[wx]


def test_steps_on_a_2048_bit_key(engine, keys):
    sk = _key(keys, 2048)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 32, 32, True, False, 15, 2048, 2048)
    assert (lay.g, lay.M) == (14, 2)


def test_steps_on_a_512_bit_key(engine, keys):
    """No per-row pair instance for this modulus: the finish composes exponentiations modulo N^2 itself.  g = 3."""
    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 32, 17, True, False, 4, 512, 512)
    assert (lay.g, lay.M) == (3, 2)
    _steps(engine, sk, ap, bp, KAPPA, 32, 0, False, True, 7, 513, 512)


def test_steps_with_sc_key_no_pairs(engine, keys):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk, use_pairs=False)
    _steps(engine, sk, ap, bp, KAPPA, 24, 33, True, False, 8, 77, 1024)


# ---- the verdict word: every message against its OWN end -----------------------------------------------------------------------------------
def test_split_checks_every_message_against_its_own_end(engine, keys):
    """k = 9, g = 7, M = 2: message 0 holds five pairs, message 1 four.  A bit at 4 pb of message 1 is past its end and inside
    message 0's; rows in the first and the second wave."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _layout(sk, KAPPA, 32, 32, False, False, 9)
    assert (lay.M, lay.pb) == (2, 146)
    nw, B = ap.mod_n.nwords, 70
    for row, msg, bit, want_bad in ((0, 1, 4 * 146 - 1, 0), (69, 1, 4 * 146, 1), (33, 0, 5 * 146 - 1, 0), (64, 0, 5 * 146, 1), (5, 1, 1021, 1)):
        vals = [0] * (2 * B)
        vals[msg * B + row] = 1 << bit
        _, bad = _split_raw(engine, sk, ap, lay, engine.upload(vals, nw).reshape(2, B, nw).contiguous(), B)
        assert bad == want_bad, (row, msg, bit)


def test_key_holder_refuses_a_too_wide_message_through_the_c_entry(engine, keys):
    from protocols.secure_comparison_amd.dotproduct import dot_pack, dot_sum, draw_dot

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    nw, B = ap.mod_n.nwords, 8
    hers, his = _layout(sk, KAPPA, 32, 32, False, False, 9), _layout(sk, KAPPA, 32, 32, False, False, 8)     # both M = 2
    assert hers.M == his.M == 2
    x_t = engine.upload([model.enc(sk, (1 << 32) - 1)] * (9 * B), 2 * nw).reshape(9, B, -1).contiguous()
    d = draw_dot(B, hers, ap)
    d.r_a = engine.upload([(1 << 72) - 1] * (9 * B), 3).reshape(9, B, 3).contiguous()      # her fifth pair of message 0 certainly has bits
    P, _ = dot_pack(hers, x_t, x_t, d, ap)
    out = engine.empty(B, 2 * nw)
    rc = engine.lib.sc_keyholder_dot(engine.ctx, bp.key.id, KAPPA, 32, 32, 0, 8, engine._ptr(P), engine._ptr(d.rho_d), engine._ptr(out), B)
    assert rc == -5                                                     # SC_ERR_LAYOUT
    with pytest.raises(ValueError, match="exceeds the end of its message"):
        dot_sum(his, P, bp, d.rho_d)
    assert dot_sum(hers, P, bp, d.rho_d).shape == (B, 2 * nw)           # and the verdict word is clean again


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(engine, keys):
    from protocols.secure_comparison_amd import DotDraws, secure_dot_batch, secure_sum_squares_batch
    from protocols.secure_comparison_amd.dotproduct import dot_pack, draw_dot

    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    nw, B = ap.mod_n.nwords, 4
    one = engine.upload([model.enc(sk, 1)] * B, 2 * nw)
    x2 = torch.stack([one, one]).contiguous()
    with pytest.raises(ValueError, match="pb = 636"):                   # a layout that does not fit
        secure_dot_batch(x2, x2, 255, 255, ap, bp, kappa=62)
    with pytest.raises(ValueError, match="sum of k = 2"):               # one field fits (g = 1), the squares' sum does not
        secure_sum_squares_batch(x2, 215, ap, bp)
    with pytest.raises(ValueError, match="k = 0"):
        secure_dot_batch(x2[:0], x2[:0], 8, 8, ap, bp)
    big = one.unsqueeze(0).expand(1025, B, 2 * nw).contiguous()
    with pytest.raises(ValueError, match="k = 1025"):
        secure_dot_batch(big, big, 8, 8, ap, bp)
    # the library's own copy of the rule, with nothing launched and nothing written
    before = dict(engine.launch_counts())
    sentinel = 0x5A5A5A5A
    full = lambda *shape: torch.full(shape, sentinel, dtype=torch.int32, device=engine.device)  # noqa: E731
    r = engine.upload([1] * (2 * B), 10).reshape(2, B, 10).contiguous()
    rho = engine.upload([2] * (2 * B), nw).reshape(2, B, nw).contiguous()
    for args, what in (((62, 255, 255, 0, 0, 2), b"pb = 636"), ((40, 215, 0, 0, 1, 2), b"sum of k = 2"), ((40, 8, 8, 0, 0, 0), b"k = 0"),
                       ((40, 8, 8, 0, 0, 1025), b"k = 1025"), ((40, 8, 256, 0, 0, 2), b"wy = 256")):
        P, e, S = full(2, B, 2 * nw), full(4, B, 10), full(B, nw)
        rc = engine.lib.sc_initiator_dot_pack(engine.ctx, ap.key.id, *args, engine._ptr(x2), engine._ptr(x2), engine._ptr(r), 10, engine._ptr(r), 10,
                                              engine._ptr(rho), 10, engine._ptr(P), engine._ptr(e), engine._ptr(S), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        rc = engine.lib.sc_keyholder_dot(engine.ctx, bp.key.id, args[0], args[1], args[2], args[4], args[5], engine._ptr(P), engine._ptr(rho),
                                         engine._ptr(S), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        rc = engine.lib.sc_initiator_dot_finish(engine.ctx, ap.key.id, args[0], args[1], args[2], args[4], args[5], engine._ptr(x2), engine._ptr(x2),
                                                engine._ptr(one), engine._ptr(e), 10, engine._ptr(S), None, 1, engine._ptr(P), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        engine.synchronize()
        assert all(bool((t == sentinel).all()) for t in (P, e, S))
    assert dict(engine.launch_counts()) == before
    # a null rho_p
    lay = _layout(sk, KAPPA, 8, 8, False, False, 2)
    d = draw_dot(B, lay, ap)
    with pytest.raises(ValueError, match="rho_p is required"):
        dot_pack(lay, x2, x2, DotDraws(d.r_a, d.r_b, None, None), ap)
    # a coefficient out of range
    with pytest.raises(ValueError, match="coef = 2"):
        engine.initiator_dot_finish(ap.key, KAPPA, 8, 8, False, 2, x2, x2, one, torch.zeros((4, B, 2), dtype=torch.int32, device=engine.device),
                                    engine.upload([0] * B, nw), None, 2)


def test_a_non_invertible_answer_names_its_row(engine, keys):
    from protocols.secure_comparison_amd.dotproduct import dot_finish, dot_pack, dot_sum, draw_dot
    from protocols.secure_comparison_amd.engine import NotInvertibleError

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    k, B = 4, 10
    lay = _layout(sk, KAPPA, 8, 8, False, False, k)
    x_t = engine.upload([model.enc(sk, 1 + (j + i) % 5, 7 + i + j) for j in range(k) for i in range(B)], ap.mod_n2.nwords).reshape(k, B, -1).contiguous()
    d = draw_dot(B, lay, ap)
    P, plain = dot_pack(lay, x_t, x_t, d, ap)
    d_enc = dot_sum(lay, P, bp, d.rho_d)
    bad = d_enc.clone()
    bad[7] = engine.upload([sk.p], ap.mod_n2.nwords)[0]                 # shares the factor p with N^2
    with pytest.raises(NotInvertibleError) as err:
        dot_finish(lay, x_t, x_t, bad, plain, ap, None, -1)
    assert err.value.index == 7
    got = engine.download(bp.decrypt_raw_batch(dot_finish(lay, x_t, x_t, d_enc, plain, ap, None, -1)))
    assert got == [-sum((1 + (j + i) % 5) ** 2 for j in range(k)) % sk.n for i in range(B)]


# ---- coef and base, the squared distance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef,with_base", [(-1, True), (-2, False), (1, True)])
def test_finish_with_coef_and_base(engine, keys, coef, with_base):
    from protocols.secure_comparison_amd.dotproduct import dot_finish, dot_pack, dot_sum

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, k, wx, wy = sk.n, 5, 16, 9
    rng = random.Random(600 + coef + with_base)
    lay = _layout(sk, KAPPA, wx, wy, True, False, k)
    xs, ys, draws = _case(rng, sk, KAPPA, wx, wy, True, False, k, COUNT)
    (x_c, x_t), (y_c, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
    md = _upload_draws(engine, ap, lay, draws)
    bs = [rng.getrandbits(40) for _ in range(COUNT)]
    b_c, b_t = _enc(engine, sk, ap, rng, bs)
    P, plain = dot_pack(lay, x_t, y_t, md, ap)
    d_enc = dot_sum(lay, P, bp, md.rho_d)
    out = dot_finish(lay, x_t, y_t, d_enc, plain, ap, b_t if with_base else None, coef)
    got, got_d = engine.download(out), engine.download(d_enc)
    for i in list(range(9)) + [COUNT - 1]:
        want = model.finish(sk, KAPPA, wx, wy, True, False, [c[i] for c in x_c], [c[i] for c in y_c], got_d[i], draws[i][0], draws[i][1],
                            b_c[i] if with_base else None, coef)
        assert got[i] == want, i
    dec = engine.download(bp.decrypt_raw_batch(out))
    assert dec == [((bs[i] if with_base else 0) + coef * sum(xs[j][i] * ys[j][i] for j in range(k))) % n for i in range(COUNT)]


def test_secure_squared_distance_and_sum_of_squares(engine, keys):
    from protocols.secure_comparison_amd import secure_dot_batch, secure_squared_distance_batch, secure_sum_squares_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    rng = random.Random(700)
    n, k, w = sk.n, 16, 32
    top = (1 << w) - 1
    xs = [[(0, top, top, 0, 1)[i] if i < 5 else rng.getrandbits(w) for i in range(COUNT)] for _ in range(k)]
    ys = [[(top, 0, top, 0, 0)[i] if i < 5 else rng.getrandbits(w) for i in range(COUNT)] for _ in range(k)]
    (_, x_t), (_, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t))  # noqa: E731
    assert dec(secure_squared_distance_batch(x_t, y_t, w, ap, bp)) == [sum((xs[j][i] - ys[j][i]) ** 2 for j in range(k)) for i in range(COUNT)]
    assert dec(secure_sum_squares_batch(x_t, w, ap, bp)) == [sum(xs[j][i] ** 2 for j in range(k)) for i in range(COUNT)]
    assert dec(secure_dot_batch(x_t, y_t, w, w, ap, bp)) == [sum(xs[j][i] * ys[j][i] for j in range(k)) for i in range(COUNT)]
    with pytest.raises(ValueError, match="shape"):
        secure_squared_distance_batch(x_t, y_t[:8].contiguous(), w, ap, bp)


# ---- the library's own draws ---------------------------------------------------------------------------------------------------------------
def test_own_draws_follow_the_replay(engine, keys):
    """The generator seeded with a known key and no draws argument: Alice's three calls (r_a, r_b, rho_p), then Bob's one, item layout as
    DESIGN.md 8g; the rows compared as integers and the generator left at call 4."""
    from protocols.secure_comparison_amd import secure_dot_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, k, w, B = sk.n, 9, 32, 70
    M = model.layout(KAPPA, w, w, False, k, 1024)[4]
    rng = random.Random(800)
    xs = [[_value(rng, w, True) for _ in range(B)] for _ in range(k)]
    ys = [[_value(rng, w, True) for _ in range(B)] for _ in range(k)]
    (x_c, x_t), (y_c, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
    rows = [0, 1, 63, 64, B - 1]
    try:
        engine.rng_seed(KEY)
        got = engine.download(secure_dot_batch(x_t, y_t, w, w, ap, bp, signed=True))
        rp = dr.Replay(KEY)
        r_a = rp.bits(w + KAPPA, k * B, [j * B + b for b in rows for j in range(k)])
        r_b = rp.bits(w + KAPPA, k * B, [j * B + b for b in rows for j in range(k)])
        rho_p = rp.below(n, M * B, True, [m * B + b for b in rows for m in range(M)])
        rho_d = rp.below(n, B, True, rows)
        for t, b in enumerate(rows):
            draws = (r_a[t * k:(t + 1) * k], r_b[t * k:(t + 1) * k], rho_p[t * M:(t + 1) * M], rho_d[t])
            assert got[b] == model.dot_enc(sk, KAPPA, w, w, True, False, [c[b] for c in x_c], [c[b] for c in y_c], draws), b
        assert rp.call == 4
        assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(KEY, rp.call, 64, 4)
    finally:
        engine.rng_seed(None)


# ---- two players over a communicator -------------------------------------------------------------------------------------------------------
_HIS = []


def _two_players(engine, keys, timeout_s=30.0):
    """An engine each: the initiator works on the fixture's, the key holder on one of his own (made once for the module)."""
    from protocols.secure_comparison_amd import DGK, InMemoryCommunicator, Initiator, KeyHolder, Paillier
    from protocols.secure_comparison_amd.engine import Engine

    sk, dk = _key(keys, 1024), oracle_dgk(keys, "dgk_1024_l16")
    if not _HIS:
        _HIS.append(Engine())
    his = _HIS[0]
    bp = Paillier(sk.n, sk.p, sk.q, engine=his)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=his, randomizer_bits=400)
    ap = Paillier(sk.n, engine=engine)
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=timeout_s)
    alice = Initiator(16, communicator=comm, other_party="keyholder")
    bob = KeyHolder(16, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    return sk, ap, bp, alice, bob, his


def test_players_dot_and_square(engine, keys):
    sk, ap, bp, alice, bob, his = _two_players(engine, keys, 600.0)
    rng = random.Random(900)
    n, k, B = sk.n, 9, 40
    xs, ys, _ = _case(rng, sk, KAPPA, 16, 7, True, False, k, B)
    (_, x_t), (_, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)

    async def run():
        dot, _ = await asyncio.gather(alice.perform_secure_dot_batch(x_t, y_t, 16, 7, signed=True, engine=engine),
                                      bob.perform_secure_dot_batch(k, 16, 7, signed=True))
        sq, _ = await asyncio.gather(alice.perform_secure_dot_batch(x_t, None, 16, signed=True, square=True, engine=engine),
                                     bob.perform_secure_dot_batch(k, 16, signed=True, square=True, count=B))
        return dot, sq

    dot, sq = asyncio.run(run())
    dec = lambda t: his.download(bp.decrypt_raw_batch(t.to(his.device).contiguous()))  # noqa: E731
    assert dot.shape == (B, ap.mod_n2.nwords)
    assert dec(dot) == [sum(xs[j][i] * ys[j][i] for j in range(k)) % n for i in range(B)]
    assert dec(sq) == [sum(xs[j][i] ** 2 for j in range(k)) % n for i in range(B)]


@pytest.mark.parametrize("theirs", [dict(k=8), dict(square=True), dict(x_bits=15), dict(y_bits=8), dict(kappa=50), dict(signed=False)])
def test_key_holder_refuses_a_different_header(engine, keys, theirs):
    sk, ap, bp, alice, bob, _ = _two_players(engine, keys)
    k = 9
    x_t = engine.upload([model.enc(sk, 5)] * (k * 8), ap.mod_n2.nwords).reshape(k, 8, -1).contiguous()
    his = dict(k=k, x_bits=16, y_bits=7, signed=True, square=False, kappa=40)
    his.update(theirs)

    async def run():          # the key holder refuses on his own; the initiator, still waiting for [[D]], is cancelled: no time limit runs out
        a = asyncio.ensure_future(alice.perform_secure_dot_batch(x_t, x_t, 16, 7, signed=True, kappa=40, engine=engine))
        (got,) = await asyncio.gather(bob.perform_secure_dot_batch(**his), return_exceptions=True)
        pending = not a.done()
        a.cancel()
        await asyncio.gather(a, return_exceptions=True)
        return got, pending

    got_b, alice_waits = asyncio.run(run())
    assert isinstance(got_b, ValueError) and "announces" in str(got_b)
    assert alice_waits


def test_chunked_sessions_raise(engine, keys):
    sk, ap, bp, alice, bob, _ = _two_players(engine, keys)
    x_t = engine.upload([model.enc(sk, 5)] * 16, ap.mod_n2.nwords).reshape(2, 8, -1).contiguous()
    with pytest.raises(ValueError, match="chunks"):
        asyncio.run(alice.perform_secure_dot_batch(x_t, x_t, 8, 8, chunks=2, engine=engine))


# ---- existing paths unchanged ---------------------------------------------------------------------------------------------------------------
def test_selection_and_multiplication_residues_are_unchanged(engine, keys):
    """One fixed case each, with injected draws, against the values their own models compute (tests/_select_model.py,
    tests/_mult_model.py): the same comparison on this change and on its parent."""
    from protocols.secure_comparison_amd import selection as sel
    from protocols.secure_comparison_amd.multiplication import MulDraws, MulLayout, mul_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, nw, B, kappa, l = sk.n, ap.mod_n.nwords, 40, 40, 16
    rng = random.Random(2)
    # multiplication: two columns, signed
    wx, wy = 16, [16, 9]
    xs = [_value(rng, wx, True) for _ in range(B)]
    ys = [[_value(rng, w, True) for _ in range(B)] for w in wy]
    (x_c, x_t), (y_c, y_t) = _enc(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
    draws = [mmodel.draw(rng, kappa, wx, wy, n) for _ in range(B)]
    mdr = MulDraws(r_a=engine.upload([d[0] for d in draws], 2),
                   r_b=torch.stack([engine.upload([d[1][j] for d in draws], 2) for j in range(2)]).contiguous(),
                   rho_p=engine.upload([d[2] for d in draws], nw),
                   rho_products=torch.stack([engine.upload([d[3][j] for d in draws], nw) for j in range(2)]).contiguous())
    out = mul_batch(MulLayout(kappa, wx, tuple(wy), True, n.bit_length()), x_t, y_t, ap, bp, mdr)
    want = [mmodel.multiply_enc(sk, kappa, wx, wy, True, x_c[i], [y_c[0][i], y_c[1][i]], draws[i]) for i in range(B)]
    assert _rows(engine, out) == [want[i][j] for j in range(2) for i in range(B)]
    # selection: sigma a bit, one column of l bits
    lay = sel.SelectLayout(l, kappa, (), n.bit_length())
    sig = [i % 2 for i in range(B)]
    dv = [rng.getrandbits(l + 1) for _ in range(B)]
    bv = [rng.getrandbits(l) for _ in range(B)]
    (s_c, s_t), (d_c, d_t), (b_c, b_t) = _enc(engine, sk, ap, rng, sig), _enc(engine, sk, ap, rng, dv), _enc(engine, sk, ap, rng, bv)
    sdraws = [smodel.draw(rng, kappa, [l], n) for _ in range(B)]
    bw = (max(lay.fbits) + 31) // 32
    sd = sel.SelectDraws(r_a=engine.upload([d[0] for d in sdraws], 2), r_b=engine.upload([d[1][0] for d in sdraws], bw).unsqueeze(0).contiguous(),
                         rho_p=engine.upload([d[2] for d in sdraws], nw),
                         rho_products=engine.upload([d[3][0] for d in sdraws], nw).unsqueeze(0).contiguous())
    got = sel.select_batch(lay, s_t, d_t.unsqueeze(0), b_t.unsqueeze(0), ap, bp, sd)
    assert _rows(engine, got) == [smodel.select(sk, kappa, [l], s_c[i], [d_c[i]], [b_c[i]], sdraws[i])[0] for i in range(B)]


# ---- the three families interleaved on one context -----------------------------------------------------------------------------------------
def test_families_interleaved_on_one_context(engine, keys):
    """The selection, the multiplication and the inner product share their temporaries (TMP_SEL_*), the packing program and the ratio
    finish's programs, so they run here in turn on one context and a 512-bit key (no per-row pair instance: the plain product of
    powers): a two-column selection on B = 3 rows, a two-column multiplication with coef = -2 and a base, an inner product with k = 3 at
    g = 2, M = 2 (message 0 holds pairs 0 and 2, message 1 holds pair 1 and joins the Horner chain below the partial top position), a
    sum of squares with k = 3 (g = 4, M = 1: no message joins), and the selection again on B = 5 rows -- every slot grows and shrinks,
    the packing program runs with `count` and with M * count items, the finish under the keys (2 pairs, base) and (1 pair, no base).
    Every ciphertext against the models under injected draws, and every decryption against the plain result."""
    from protocols.secure_comparison_amd import selection as sel
    from protocols.secure_comparison_amd.dotproduct import dot_batch
    from protocols.secure_comparison_amd.multiplication import MulDraws, MulLayout, mul_batch

    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    n, nw, B, kappa = sk.n, ap.mod_n.nwords, 3, KAPPA
    nbits = n.bit_length()
    rng = random.Random(900)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    stack = lambda f, cols, w, draws: torch.stack([engine.upload([f(d, j) for d in draws], w) for j in range(cols)]).contiguous()  # noqa: E731

    def selection(count):
        widths = [16, 12]
        lay = sel.SelectLayout(widths[0], kappa, (widths[1],), nbits)
        sig = [i % 2 for i in range(count)]
        av = [[rng.getrandbits(w) for _ in range(count)] for w in widths]
        bv = [[rng.getrandbits(w) for _ in range(count)] for w in widths]
        dv = [[av[j][i] - bv[j][i] + (1 << w) for i in range(count)] for j, w in enumerate(widths)]
        (s_c, s_t), (d_c, d_t), (b_c, b_t) = _enc(engine, sk, ap, rng, sig), _enc_planes(engine, sk, ap, rng, dv), _enc_planes(engine, sk, ap, rng, bv)
        draws = [smodel.draw(rng, kappa, widths, n) for _ in range(count)]
        sd = sel.SelectDraws(r_a=engine.upload([d[0] for d in draws], 2), r_b=stack(lambda d, j: d[1][j], 2, (max(lay.fbits) + 31) // 32, draws),
                             rho_p=engine.upload([d[2] for d in draws], nw), rho_products=stack(lambda d, j: d[3][j], 2, nw, draws))
        got = sel.select_batch(lay, s_t, d_t, b_t, ap, bp, sd)
        want = [smodel.select(sk, kappa, widths, s_c[i], [c[i] for c in d_c], [c[i] for c in b_c], draws[i]) for i in range(count)]
        assert _rows(engine, got) == [want[i][j] for j in range(2) for i in range(count)]
        assert dec(got) == [(av if sig[i] else bv)[j][i] for j in range(2) for i in range(count)]

    def multiplication():
        wx, wy = 16, [16, 9]
        xs = [_value(rng, wx, True) for _ in range(B)]
        ys = [[_value(rng, w, True) for _ in range(B)] for w in wy]
        bs = [[rng.getrandbits(40) for _ in range(B)] for _ in wy]
        (x_c, x_t), (y_c, y_t), (b_c, b_t) = _enc(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys), _enc_planes(engine, sk, ap, rng, bs)
        draws = [mmodel.draw(rng, kappa, wx, wy, n) for _ in range(B)]
        md = MulDraws(r_a=engine.upload([d[0] for d in draws], 2), r_b=stack(lambda d, j: d[1][j], 2, 2, draws),
                      rho_p=engine.upload([d[2] for d in draws], nw), rho_products=stack(lambda d, j: d[3][j], 2, nw, draws))
        got = mul_batch(MulLayout(kappa, wx, tuple(wy), True, nbits), x_t, y_t, ap, bp, md, b_t, -2)
        want = [mmodel.multiply_enc(sk, kappa, wx, wy, True, x_c[i], [c[i] for c in y_c], draws[i], [c[i] for c in b_c], -2) for i in range(B)]
        assert _rows(engine, got) == [want[i][j] for j in range(2) for i in range(B)]
        assert dec(got) == [(bs[j][i] - 2 * xs[i] * ys[j][i]) % n for j in range(2) for i in range(B)]

    def inner_product(wx, wy, square, k, g, M):
        lay = _layout(sk, kappa, wx, wy, True, square, k)
        assert (lay.g, lay.M) == (g, M)
        xs, ys, draws = _case(rng, sk, kappa, wx, wy, True, square, k, B)
        x_c, x_t = _enc_planes(engine, sk, ap, rng, xs)
        y_c, y_t = (None, None) if square else _enc_planes(engine, sk, ap, rng, ys)
        got = dot_batch(lay, x_t, y_t, ap, bp, _upload_draws(engine, ap, lay, draws))
        assert engine.download(got) == [model.dot_enc(sk, kappa, wx, wy, True, square, [c[i] for c in x_c], None if square else [c[i] for c in y_c],
                                                      draws[i]) for i in range(B)]
        assert dec(got) == [sum(xs[j][i] * (xs[j][i] if square else ys[j][i]) for j in range(k)) % n for i in range(B)]

    selection(B)
    multiplication()
    inner_product(64, 48, False, 3, 2, 2)
    inner_product(64, 0, True, 3, 4, 1)
    selection(5)

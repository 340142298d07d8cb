"""Secure one-hot encoding and table lookup on the GPU: every step bit for bit against the pure-Python model
(tests/_onehot_model.py) with injected draws -- the packed masks R, the rotations rot, the messages P, the decrypted fields, the key
holder's E and the rotated result -- on 1024-bit keys for the smallest shapes that reach each path, on a 2048-bit key, a 512-bit key and
with SC_KEY_NO_PAIRS; the verdict word; the refusals; the lookup against plain indexing; the two players over a communicator; the
library's own draws; and the four families in turn on one context.

A batch has 100 rows (not a multiple of a wave) unless a case says otherwise.  The plaintext arrays, the decryptions and the rotation
are checked on every row and position; the model's ciphertexts (plain Python on big integers) on the edge rows and the last random ones,
at the hot position, its neighbours and the ends of the table."""
import asyncio
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _dot_model as dmodel  # noqa: E402
import _draw_replay as dr  # noqa: E402
import _mult_model as mmodel  # noqa: E402
import _onehot_model as model  # noqa: E402
import _select_model as smodel  # noqa: E402
from oracle import chacha_rng as cr  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA, COUNT = 40, 100
KEY = bytes((3 * i + 17) & 0xFF for i in range(32))


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


def _layout(sk, kappa, ib, k, m):
    from protocols.secure_comparison_amd import OnehotLayout

    return OnehotLayout(kappa, ib, k, m, sk.n.bit_length())


def _case(rng, sk, kappa, ib, k, m, count):
    """Plaintext rows and Alice's draws.  Rows 0 .. 8: every index of the row at 0, at k - 1 or at 2^ib - 1 (at or above k where ib
    allows) under every mask at 0, at 2^(ib + kappa) - 1 or with only its high bits set -- the bits from bit 64 up when the mask has
    three words, else its top word -- in a Latin order, so that the first three rows alone meet every index and every mask; then random
    rows.  Returns (idx [m][count], draws [count] = (rs [m], rho_ps [M]))."""
    n = sk.n
    top = (1 << (ib + kappa)) - 1
    high = top & ~((1 << min(64, 32 * ((ib + kappa - 1) // 32))) - 1)
    edges, fills = [0, (k - 1) % (1 << ib), (1 << ib) - 1], [0, top, high]
    rows = []
    for t in range(9):
        d = model.draw(rng, kappa, ib, k, m, n, with_bob=False)
        rows.append(([edges[t % 3]] * m, ([fills[(t + t // 3) % 3]] * m, d[1])))
    while len(rows) < count:
        d = model.draw(rng, kappa, ib, k, m, n, with_bob=False)
        rows.append(([rng.getrandbits(ib) for _ in range(m)], (d[0], d[1])))
    rows = rows[:count]
    return [[r[0][q] for r in rows] for q in range(m)], [r[1] for r in rows]


def _upload_draws(engine, ap, lay, draws, rho_e=None):
    from protocols.secure_comparison_amd import OnehotDraws

    nw = ap.mod_n.nwords
    planes = lambda f, cnt, w: torch.stack([engine.upload([f(d, j) for d in draws], w) for j in range(cnt)]).contiguous()  # noqa: E731
    return OnehotDraws(r=planes(lambda d, q: d[0][q], lay.m, lay.rw), rho_p=planes(lambda d, mm: d[1][mm], lay.M, nw), rho_e=rho_e)


def _model_rows(bits, count):
    if bits <= 1024:
        return sorted(set(list(range(min(9, count))) + list(range(max(0, count - 2), count))))
    return sorted({1, 2, count - 1})


def _prep_raw(engine, sk, ap, lay, md, count):
    """sc_onehot_prep itself (the dev entry): (R, rot) for every row."""
    nw = ap.mod_n.nwords
    _, pn = engine._host_n_words(sk.n, nw)
    R = torch.empty((lay.M, count, nw), dtype=torch.int32, device=engine.device)
    rot = torch.empty((lay.m, count), dtype=torch.int32, device=engine.device)
    engine._sync_stream()
    rc = engine.lib.sc_onehot_prep(engine.ctx, pn, nw, lay.kappa, lay.ib, lay.k, lay.m, engine._ptr(md.r), md.r.shape[-1], engine._ptr(R),
                                   engine._ptr(rot), count)
    assert rc == 0, engine.lib.sc_last_error(engine.ctx)
    return R, rot


def _split_raw(engine, sk, ap, lay, P_plain, count):
    """sc_onehot_split itself on plaintext messages [M][count][nw]: (prod [m][k][count][nw], bad)."""
    nw = ap.mod_n.nwords
    _, pn = engine._host_n_words(sk.n, nw)
    prod = torch.full((lay.m, lay.k, count, nw), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    bad = torch.zeros(1, dtype=torch.int32, device=engine.device)
    engine._sync_stream()
    rc = engine.lib.sc_onehot_split(engine.ctx, pn, nw, lay.kappa, lay.ib, lay.k, lay.m, engine._ptr(P_plain), engine._ptr(prod), engine._ptr(bad),
                                    count)
    assert rc == 0, engine.lib.sc_last_error(engine.ctx)
    engine.synchronize()
    return prod, int(bad.item())


def _steps(engine, sk, ap, bp, kappa, ib, k, m, seed, bits, count=COUNT, rows=None):
    from protocols.secure_comparison_amd.lookup import draw_onehot, onehot_answer, onehot_finish, onehot_pack

    n, nw = sk.n, ap.mod_n.nwords
    nbits = n.bit_length()
    rng = random.Random(seed)
    lay = _layout(sk, kappa, ib, k, m)
    f, g, M = lay.f, lay.g, lay.M
    assert (f, g, M, lay.rw) == model.layout(kappa, ib, k, m, nbits)
    idx, draws = _case(rng, sk, kappa, ib, k, m, count)
    i_c, i_t = _enc_planes(engine, sk, ap, rng, idx)
    rho_e = draw_onehot(count, lay, ap, alice=False).rho_e
    rho_ints = _rows(engine, rho_e)
    md = _upload_draws(engine, ap, lay, draws, rho_e)
    rows = _model_rows(bits, count) if rows is None else rows          # (rows: the rows the model follows, when the caller says)
    iv = lambda b: [i_c[q][b] for q in range(m)]  # noqa: E731

    # the plaintext arrays, every row: sc_onehot_prep's R and rot against the model
    pl = [model.plain(kappa, ib, k, m, nbits, d[0]) for d in draws]
    R_raw, rot_raw = _prep_raw(engine, sk, ap, lay, md, count)
    assert _rows(engine, R_raw) == [pl[b][0][mm] for mm in range(M) for b in range(count)]
    assert rot_raw.cpu().tolist() == [[pl[b][1][q] for b in range(count)] for q in range(m)]
    # sc_onehot_split on the plaintexts the key holder will see: every row of every position, the verdict word clean
    plain_P = [pl[b][0][mm] + sum(idx[q][b] << ((q % g) * f) for q in model.members(mm, m, g)) for mm in range(M) for b in range(count)]
    assert all(0 <= p < n for p in plain_P)
    hot = [[(idx[q][b] + draws[b][0][q]) % k for b in range(count)] for q in range(m)]
    want_prod = torch.zeros((m, k, count, nw), dtype=torch.int32)
    for q in range(m):
        for b in range(count):
            want_prod[q, hot[q][b], b, 0] = 1
    prod, bad = _split_raw(engine, sk, ap, lay, engine.upload(plain_P, nw).reshape(M, count, nw).contiguous(), count)
    assert torch.equal(prod.cpu(), want_prod) and bad == 0
    for b in rows:                                        # the model's own split of the same messages
        d, j, mbad = model.split(kappa, ib, k, m, nbits, [plain_P[mm * count + b] for mm in range(M)])
        assert d == [idx[q][b] + draws[b][0][q] for q in range(m)] and j == [hot[q][b] for q in range(m)] and not mbad

    # the three scheme-level steps
    P, rot = onehot_pack(lay, i_t, md, ap)
    assert P.shape == (M, count, 2 * nw) and torch.equal(rot, rot_raw)
    got_P = _rows(engine, P)
    want_P = {b: model.pack(sk, kappa, ib, k, iv(b), draws[b][0], draws[b][1]) for b in rows}
    assert [got_P[mm * count + b] for mm in range(M) for b in rows] == [want_P[b][mm] for mm in range(M) for b in rows]
    assert engine.download(bp.decrypt_raw_batch(P.reshape(M * count, -1))) == plain_P          # the decrypted fields, every row

    E = onehot_answer(lay, P, bp, rho_e)
    assert E.shape == (m, k, count, 2 * nw)
    flat_hot = [1 if t == hot[q][b] else 0 for q in range(m) for t in range(k) for b in range(count)]
    assert engine.download(bp.decrypt_raw_batch(E.reshape(m * k * count, -1))) == flat_hot
    got_E = _rows(engine, E)
    qs = sorted({0, m - 1, g - 1, g} & set(range(m)))
    out = onehot_finish(lay, E, rot, ap)
    got_out = _rows(engine, out)
    for b in rows:
        rho_b = [[rho_ints[(q * k + t) * count + b] for t in range(k)] for q in range(m)]
        ts = {q: sorted({0, k - 1, hot[q][b], (hot[q][b] + 1) % k, idx[q][b] % k}) for q in qs}
        only = sorted({(q, t) for q in qs for t in ts[q]} | {(q, (t + pl[b][1][q]) % k) for q in qs for t in ts[q]})
        mE, md_, mj, mbad = model.answer(sk, kappa, ib, k, m, want_P[b], rho_b, only)
        assert not mbad and mj == [hot[q][b] for q in range(m)]
        assert all(got_E[(q * k + t) * count + b] == c for (q, t), c in mE.items()), b
        for q in qs:                                      # the rotated rows against the model's E
            assert all(got_out[(q * k + t) * count + b] == mE[(q, (t + pl[b][1][q]) % k)] for t in ts[q]), (b, q)
    # the rotation of every row and position, as a gather of E's rows
    src = (torch.arange(k, device=E.device).view(1, k, 1) + rot.long().unsqueeze(1)) % k
    assert torch.equal(out, torch.gather(E, 1, src.unsqueeze(-1).expand(-1, -1, -1, 2 * nw)))
    want_dec = [1 if t == idx[q][b] % k else 0 for q in range(m) for t in range(k) for b in range(count)]
    assert engine.download(bp.decrypt_raw_batch(out.reshape(m * k * count, -1))) == want_dec
    return lay


# ---- 1024-bit keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,count", [(1, COUNT), (2, COUNT), (3, COUNT), (7, COUNT), (8, COUNT), (1000, 3)])
def test_steps_bit_exact_vs_model(engine, keys, k, count):
    """ib = 10, kappa = 40: masks of 50 bits, two words.  2^32 mod k = 0 for a power of two, so a remainder taken from the low word alone
    passes on k = 1, 2, 8 and fails on 3, 7 and 1000.  2^ib - 1 = 1023 is at or above every k here."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 10, k, 1, 100 + k, 1024, count)
    assert (lay.f, lay.g, lay.M) == (51, 20, 1)


@pytest.mark.parametrize("m,M", [(20, 1), (21, 2)])
def test_steps_full_and_partial_last_message(engine, keys, m, M):
    """g = 20: m = 20 fills one message, m = 21 leaves the second with one field (m = 1 is the case above)."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 10, 3, m, 200 + m, 1024)
    assert (lay.g, lay.M) == (20, M)


def test_steps_widest_field(engine, keys):
    """kappa = 62 with ib = 32: fields of 95 bits at the offsets 0, 95, 190, .. -- unaligned, crossing words -- masks of 94 bits in three
    words, the edge rows with only the bits from bit 64 up.  g = 10; m = 11 takes two messages."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, 62, 32, 7, 11, 300, 1024)
    assert (lay.f, lay.g, lay.M, lay.rw) == (95, 10, 2, 3)


def test_steps_kappa_1(engine, keys):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, 1, 3, 5, 2, 301, 1024)
    assert (lay.f, lay.g) == (5, 204)


def test_steps_on_a_2048_bit_key(engine, keys):
    sk = _key(keys, 2048)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 10, 5, 2, 2048, 2048)
    assert (lay.g, lay.M) == (40, 1)


def test_steps_on_a_512_bit_key(engine, keys):
    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 10, 6, 11, 512, 512)
    assert (lay.g, lay.M) == (10, 2)


def test_steps_three_messages_partial_last(engine, keys):
    """m = 23 at g = 10: three messages, the last with three fields, so the positions 0 .. 2 are held by three messages and 3 .. 9 by
    two -- the last message joins the chain below its own top position, beside two others that came down it."""
    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    lay = _steps(engine, sk, ap, bp, KAPPA, 10, 6, 23, 523, 512, 20)
    assert (lay.g, lay.M) == (10, 3)


def test_steps_with_sc_key_no_pairs(engine, keys):
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk, use_pairs=False)
    _steps(engine, sk, ap, bp, KAPPA, 10, 6, 21, 77, 1024, 20)


# ---- the verdict word: every message against its OWN end -----------------------------------------------------------------------------------
def test_split_checks_every_message_against_its_own_end(engine, keys):
    """g = 20, m = 21: message 0 ends at 20 f = 1020, the partial last message at f = 51.  A bit at 51 of message 1 is past its end and
    far inside message 0's; rows in the first and the second wave of a block."""
    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _layout(sk, KAPPA, 10, 3, 21)
    assert (lay.M, lay.f, lay.g) == (2, 51, 20)
    nw, B = ap.mod_n.nwords, 70
    for row, msg, bit, want_bad in ((0, 1, 50, 0), (69, 1, 51, 1), (33, 0, 1019, 0), (64, 0, 1020, 1), (5, 1, 1021, 1), (7, 1, 700, 1)):
        vals = [0] * (2 * B)
        vals[msg * B + row] = 1 << bit
        _, bad = _split_raw(engine, sk, ap, lay, engine.upload(vals, nw).reshape(2, B, nw).contiguous(), B)
        assert bad == want_bad, (row, msg, bit)


def test_key_holder_refuses_a_planted_bit_through_the_c_entry(engine, keys):
    from protocols.secure_comparison_amd.lookup import draw_onehot, onehot_answer

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    lay = _layout(sk, KAPPA, 10, 3, 21)
    nw, B = ap.mod_n.nwords, 8
    rho_e = draw_onehot(B, lay, ap, alice=False).rho_e

    def messages(bit):
        vals = [0] * (2 * B)
        vals[B + 5] = 1 << bit                               # message 1 of row 5
        return ap.encrypt_raw_batch(engine.upload(vals, nw)).reshape(2, B, -1).contiguous()

    P = messages(lay.f)
    out = torch.empty((21, 3, B, 2 * nw), dtype=torch.int32, device=engine.device)
    engine._sync_stream()
    rc = engine.lib.sc_keyholder_onehot(engine.ctx, bp.key.id, KAPPA, 10, 3, 21, engine._ptr(P), engine._ptr(rho_e), engine._ptr(out), B)
    assert rc == -5                                                     # SC_ERR_LAYOUT
    with pytest.raises(ValueError, match="exceeds the end of its message"):
        onehot_answer(lay, P, bp, rho_e)
    E = onehot_answer(lay, messages(lay.f - 1), bp, rho_e)              # the top bit of the field itself: fine, and the word is clean again
    assert E.shape == (21, 3, B, 2 * nw)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(engine, keys):
    from protocols.secure_comparison_amd import OnehotDraws, secure_onehot_batch
    from protocols.secure_comparison_amd.lookup import draw_onehot, onehot_pack

    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    nw, B = ap.mod_n.nwords, 4
    one = engine.upload([model.enc(sk, 1)] * B, 2 * nw)
    for kw, what in ((dict(k=0), "k = 0"), (dict(k=1025), "k = 1025"), (dict(k=5, index_bits=33), "ib = 33"), (dict(k=5, kappa=63), "kappa = 63")):
        with pytest.raises(ValueError, match=what):
            secure_onehot_batch(one, alice_paillier=ap, bob_paillier=bp, **kw)
    # the library's own copy of the rule, with nothing launched and nothing written
    before = dict(engine.launch_counts())
    sentinel = 0x5A5A5A5A
    full = lambda *shape: torch.full(shape, sentinel, dtype=torch.int32, device=engine.device)  # noqa: E731
    r = engine.upload([1] * B, 3).reshape(1, B, 3).contiguous()
    rho = engine.upload([2] * (5 * B), nw).reshape(1, 5, B, nw).contiguous()
    for args, what in (((40, 10, 0, 1), b"k = 0"), ((40, 10, 1025, 1), b"k = 1025"), ((40, 33, 5, 1), b"ib = 33"), ((40, 0, 5, 1), b"ib = 0"),
                       ((63, 10, 5, 1), b"kappa = 63"), ((40, 10, 5, 0), b"m = 0")):
        P, rot, E = full(1, B, 2 * nw), full(1, B), full(1, 5, B, 2 * nw)
        rc = engine.lib.sc_initiator_onehot_pack(engine.ctx, ap.key.id, *args, engine._ptr(one), engine._ptr(r), 3, engine._ptr(rho), engine._ptr(P),
                                                 engine._ptr(rot), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        rc = engine.lib.sc_keyholder_onehot(engine.ctx, bp.key.id, *args, engine._ptr(P), engine._ptr(rho), engine._ptr(E), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        rc = engine.lib.sc_initiator_onehot_finish(engine.ctx, ap.key.id, *args, engine._ptr(E), engine._ptr(rot), engine._ptr(full(1, 5, B, 2 * nw)), B)
        assert rc == -1 and what in engine.lib.sc_last_error(engine.ctx), args
        engine.synchronize()
        assert all(bool((t == sentinel).all()) for t in (P, rot, E))
    # out == E, and an out that overlaps E's tail: the rotation is not done in place
    E, rot = full(1, 5, B, 2 * nw), torch.zeros((1, B), dtype=torch.int32, device=engine.device)
    with pytest.raises(ValueError, match="overlaps"):
        engine.initiator_onehot_finish(ap.key, 40, 10, 5, 1, E, rot, E)
    big = full(2, 5, B, 2 * nw)
    rc = engine.lib.sc_onehot_rotate(engine.ctx, 2 * nw, 5, 1, engine._ptr(big[0]), engine._ptr(rot), engine._ptr(big.reshape(-1)[2 * nw:]), B)
    assert rc == -1 and b"overlaps" in engine.lib.sc_last_error(engine.ctx)
    rc = engine.lib.sc_onehot_rotate(engine.ctx, 2 * nw, 5, 1, engine._ptr(big[0]), engine._ptr(rot), engine._ptr(big[1]), B)      # adjacent: fine
    assert rc == 0
    engine.synchronize()
    assert torch.equal(big[0], big[1])
    # the arguments in their own order: a missing array is named
    rc = engine.lib.sc_initiator_onehot_pack(engine.ctx, ap.key.id, 40, 10, 5, 1, engine._ptr(one), None, 3, engine._ptr(rho), None, None, B)
    assert rc == -1 and b" r: missing" in engine.lib.sc_last_error(engine.ctx)
    assert dict(engine.launch_counts()) == before
    # draw rows too narrow, and a null rho_p
    lay = _layout(sk, KAPPA, 10, 5, 1)
    d = draw_onehot(B, lay, ap)
    assert d.r.shape[-1] == 2
    with pytest.raises(ValueError, match="too narrow"):
        onehot_pack(lay, one.unsqueeze(0), OnehotDraws(d.r[:, :, :1].contiguous(), d.rho_p, None), ap)
    with pytest.raises(ValueError, match="rho_p is required"):
        onehot_pack(lay, one.unsqueeze(0), OnehotDraws(d.r, None, None), ap)


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 32, 255])
def test_gather_against_plain_lookup(engine, keys, bits):
    """k = 5 entries per row, m = 3 indices of which the last is at or above k (reduced): the decrypted results against table[i mod k],
    on an unsigned and on a signed table whose entries meet both ends of their range."""
    from protocols.secure_comparison_amd import secure_gather_batch, secure_lookup_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, k, m, B = sk.n, 5, 3, 20
    rng = random.Random(500 + bits)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    for signed in (False, True):
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        table = [[(lo, hi)[(j + b) % 2] if b < 4 else rng.randint(lo, hi) for b in range(B)] for j in range(k)]
        idx = [[rng.randrange(k) for _ in range(B)], [(b + 1) % k for b in range(B)], [k + rng.randrange(3) for _ in range(B)]]
        (_, t_t), (_, i_t) = _enc_planes(engine, sk, ap, rng, table), _enc_planes(engine, sk, ap, rng, idx)
        got = secure_gather_batch(t_t, i_t, bits, ap, bp, signed=signed)
        assert got.shape == (m, B, ap.mod_n2.nwords)
        assert dec(got) == [table[idx[q][b] % k][b] % n for q in range(m) for b in range(B)], signed
        one = secure_lookup_batch(t_t, i_t[0].contiguous(), bits, ap, bp, signed=signed)
        assert one.shape == (B, ap.mod_n2.nwords) and dec(one) == [table[idx[0][b]][b] % n for b in range(B)]


# ---- the library's own draws ---------------------------------------------------------------------------------------------------------------
def test_own_draws_follow_the_replay(engine, keys):
    """The generator seeded with a known key and no draws argument: Alice's two calls (r, rho_p), then Bob's one, item layout as DESIGN.md
    8i; sampled ciphertexts compared as integers and the generator left at call 3."""
    from protocols.secure_comparison_amd import secure_onehot_batch

    sk = _key(keys, 1024)
    ap, bp = _paillier(engine, sk)
    n, k, m, ib, B = sk.n, 7, 21, 10, 70
    f, g, M, _ = model.layout(KAPPA, ib, k, m, 1024)
    rng = random.Random(800)
    idx = [[rng.getrandbits(ib) for _ in range(B)] for _ in range(m)]
    i_c, i_t = _enc_planes(engine, sk, ap, rng, idx)
    rows, qs = [0, 63, 64, B - 1], [0, 19, 20]
    try:
        engine.rng_seed(KEY)
        got = _rows(engine, secure_onehot_batch(i_t, k, ap, bp, index_bits=ib))
        rp = dr.Replay(KEY)
        r = rp.bits(ib + KAPPA, m * B, [q * B + b for b in rows for q in range(m)])
        rp.below(n, M * B, True, [0])
        items = [(q * k + t) * B + b for b in rows for q in qs for t in range(k)]
        rho_e = dict(zip(items, rp.below(n, m * k * B, True, items)))
        for x, b in enumerate(rows):
            for q in qs:
                rq = r[x * m + q]
                for t in range(k):
                    s = (t + rq) % k
                    want = model.enc(sk, 1 if s == (idx[q][b] + rq) % k else 0, rho_e[(q * k + s) * B + b])
                    assert got[(q * k + t) * B + b] == want, (b, q, t)
        assert rp.call == 3
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


def test_players_onehot_and_gather(engine, keys):
    sk, ap, bp, alice, bob, his = _two_players(engine, keys, 600.0)
    rng = random.Random(900)
    n, k, m, B, bits = sk.n, 6, 2, 40, 16
    table = [[rng.randint(-(1 << 15), (1 << 15) - 1) for _ in range(B)] for _ in range(k)]
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    (_, t_t), (_, i_t) = _enc_planes(engine, sk, ap, rng, table), _enc_planes(engine, sk, ap, rng, idx)

    async def run():
        oh, _ = await asyncio.gather(alice.perform_secure_onehot_batch(i_t[0].contiguous(), k, engine=engine), bob.perform_secure_onehot_batch(k))
        ga, _ = await asyncio.gather(alice.perform_secure_gather_batch(t_t, i_t, bits, signed=True, engine=engine),
                                     bob.perform_secure_gather_batch(k, m, bits, signed=True, count=B))
        return oh, ga

    oh, ga = asyncio.run(run())
    dec = lambda t: his.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).to(his.device).contiguous()))  # noqa: E731
    assert oh.shape == (k, B, ap.mod_n2.nwords) and ga.shape == (m, B, ap.mod_n2.nwords)
    assert dec(oh) == [1 if t == idx[0][b] else 0 for t in range(k) for b in range(B)]
    assert dec(ga) == [table[idx[q][b]][b] % n for q in range(m) for b in range(B)]


def test_key_holder_refuses_a_different_header(engine, keys):
    sk, ap, bp, alice, bob, _ = _two_players(engine, keys)
    i_t = engine.upload([model.enc(sk, 2)] * 8, ap.mod_n2.nwords)

    async def run():          # the key holder refuses on his own; the initiator, still waiting for E, is cancelled: no time limit runs out
        a = asyncio.ensure_future(alice.perform_secure_onehot_batch(i_t, 6, engine=engine))
        (got,) = await asyncio.gather(bob.perform_secure_onehot_batch(7), return_exceptions=True)
        pending = not a.done()
        a.cancel()
        await asyncio.gather(a, return_exceptions=True)
        return got, pending

    got_b, alice_waits = asyncio.run(run())
    assert isinstance(got_b, ValueError) and "announces" in str(got_b)
    assert alice_waits


# ---- the four families interleaved on one context ------------------------------------------------------------------------------------------
def test_families_interleaved_on_one_context(engine, keys):
    """The selection, the multiplication, the inner product and the one-hot share their temporaries (TMP_SEL_*) and the packing program,
    so they run here in turn on one context and a 512-bit key: a one-hot with m = 11 at g = 10 (two messages: the gather into TMP_SEL_D
    and a Horner chain whose last message joins at the bottom), a two-column selection, a one-hot with m = 2 (one message, no gather), a
    multiplication with coef = -2 and a base, an inner product with k = 3 at g = 2, and the first one-hot again on more rows -- every slot
    grows and shrinks.  Every ciphertext against the models under injected draws, and every decryption against the plain result."""
    from protocols.secure_comparison_amd import selection as sel
    from protocols.secure_comparison_amd.dotproduct import DotDraws, DotLayout, dot_batch
    from protocols.secure_comparison_amd.lookup import onehot_batch
    from protocols.secure_comparison_amd.multiplication import MulDraws, MulLayout, mul_batch

    sk = _key(keys, 512)
    ap, bp = _paillier(engine, sk)
    n, nw, B, kappa = sk.n, ap.mod_n.nwords, 3, KAPPA
    nbits = n.bit_length()
    rng = random.Random(901)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    stack = lambda fn, cols, w, draws: torch.stack([engine.upload([fn(d, j) for d in draws], w) for j in range(cols)]).contiguous()  # noqa: E731
    value = lambda w: rng.getrandbits(w) - (1 << (w - 1))  # noqa: E731

    def onehot(k, m, count):
        ib = 10
        lay = _layout(sk, kappa, ib, k, m)
        idx = [[rng.getrandbits(ib) for _ in range(count)] for _ in range(m)]
        i_c, i_t = _enc_planes(engine, sk, ap, rng, idx)
        draws = [model.draw(rng, kappa, ib, k, m, n) for _ in range(count)]
        md = _upload_draws(engine, ap, lay, draws)
        md.rho_e = torch.stack([stack(lambda d, t: d[2][q][t], k, nw, draws) for q in range(m)]).contiguous()
        got = onehot_batch(lay, i_t, ap, bp, md)
        want = [model.onehot_enc(sk, kappa, ib, k, [i_c[q][b] for q in range(m)], draws[b]) for b in range(count)]
        assert _rows(engine, got) == [want[b][q][t] for q in range(m) for t in range(k) for b in range(count)]
        assert dec(got) == [1 if t == idx[q][b] % k else 0 for q in range(m) for t in range(k) for b in range(count)]

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
        xs = [value(wx) for _ in range(B)]
        ys = [[value(w) for _ in range(B)] for w in wy]
        bs = [[rng.getrandbits(40) for _ in range(B)] for _ in wy]
        (x_c, x_t), (y_c, y_t), (b_c, b_t) = _enc(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys), _enc_planes(engine, sk, ap, rng, bs)
        draws = [mmodel.draw(rng, kappa, wx, wy, n) for _ in range(B)]
        md = MulDraws(r_a=engine.upload([d[0] for d in draws], 2), r_b=stack(lambda d, j: d[1][j], 2, 2, draws),
                      rho_p=engine.upload([d[2] for d in draws], nw), rho_products=stack(lambda d, j: d[3][j], 2, nw, draws))
        got = mul_batch(MulLayout(kappa, wx, tuple(wy), True, nbits), x_t, y_t, ap, bp, md, b_t, -2)
        want = [mmodel.multiply_enc(sk, kappa, wx, wy, True, x_c[i], [c[i] for c in y_c], draws[i], [c[i] for c in b_c], -2) for i in range(B)]
        assert _rows(engine, got) == [want[i][j] for j in range(2) for i in range(B)]
        assert dec(got) == [(bs[j][i] - 2 * xs[i] * ys[j][i]) % n for j in range(2) for i in range(B)]

    def inner_product():
        wx, wy, k = 64, 48, 3
        lay = DotLayout(kappa, wx, wy, k, True, False, nbits)
        assert (lay.g, lay.M) == (2, 2)
        xs, ys = [[value(wx) for _ in range(B)] for _ in range(k)], [[value(wy) for _ in range(B)] for _ in range(k)]
        (x_c, x_t), (y_c, y_t) = _enc_planes(engine, sk, ap, rng, xs), _enc_planes(engine, sk, ap, rng, ys)
        draws = [dmodel.draw(rng, kappa, wx, wy, False, k, n) for _ in range(B)]
        md = DotDraws(r_a=stack(lambda d, j: d[0][j], k, (wx + kappa + 31) // 32, draws), r_b=stack(lambda d, j: d[1][j], k, (wy + kappa + 31) // 32, draws),
                      rho_p=stack(lambda d, j: d[2][j], lay.M, nw, draws), rho_d=engine.upload([d[3] for d in draws], nw))
        got = dot_batch(lay, x_t, y_t, ap, bp, md)
        assert engine.download(got) == [dmodel.dot_enc(sk, kappa, wx, wy, True, False, [c[i] for c in x_c], [c[i] for c in y_c], draws[i])
                                        for i in range(B)]
        assert dec(got) == [sum(xs[j][i] * ys[j][i] for j in range(k)) % n for i in range(B)]

    onehot(3, 11, B)
    selection(B)
    onehot(4, 2, B)
    multiplication()
    inner_product()
    onehot(3, 11, 5)

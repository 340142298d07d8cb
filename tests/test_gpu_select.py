"""Secure selection on the GPU: the per-row pair exponentiation (sc_modexp_var_sq, Paillier.scalar_mul_batch) against Python pow,
the three selection steps bit for bit against the pure-Python model (tests/_select_model.py) with injected draws, and decrypted
minimum / maximum / argmin / argmax against Python on random and edge rows."""
import json
import os
import random
import sys

import pytest
import torch

from conftest import GOLDEN, oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _select_model as model  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(engine, t):
    return engine.download(t.reshape(-1, t.shape[-1]).contiguous())


def _paillier(engine, sk):
    from protocols.secure_comparison_amd import Paillier

    bob = Paillier(sk.n, sk.p, sk.q, engine=engine)
    return bob.public_copy(), bob


def _players(engine, keys, pbits, dname, wide=False):
    from protocols.secure_comparison_amd import DGK

    sk = oracle_paillier(keys, pbits)
    if wide:
        k = json.load(open(os.path.join(GOLDEN, "keys_wide.json")))[dname]
        from oracle import sc_oracle as o

        p, q = int(k["p"], 16), int(k["q"], 16)
        dk = o.DGKKey(p * q, int(k["g"], 16), int(k["h"], 16), int(k["u"], 16), k["t"], p, q, int(k["v_p"], 16), int(k["v_q"], 16))
    else:
        dk = oracle_dgk(keys, dname)
    ap, bp = _paillier(engine, sk)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=engine, randomizer_bits=400)
    return sk, ap, bd.public_copy(), bp, bd


# ---- sc_modexp_var_sq ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048, 3072])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_modexp_var_sq_matches_pow(engine, keys, bits, nb):
    sk = oracle_paillier(keys, bits)
    n, n2 = sk.n, sk.n2
    mod_n, mod_n2 = engine.modulus(n), engine.modulus(n2)
    rng = random.Random(bits * 10 + nb)
    count, ebits = 100, 83                   # not a multiple of a wave's items; ebits not a multiple of any window
    ew = (ebits + 31) // 32
    specials = [0, 1, (1 << ebits) - 1]
    xs = [[rng.randrange(n2) for _ in range(count)] for _ in range(nb)]
    es = [[specials[i] if i < 3 else (specials[(i + j) % 3] if i % 7 == 0 else rng.getrandbits(ebits)) for i in range(count)]
          for j in range(nb)]
    mul = [rng.randrange(n2) for _ in range(count)]
    x = torch.stack([engine.upload(r, 2 * mod_n.nwords) for r in xs]).contiguous()
    e = torch.stack([engine.upload(r, ew) for r in es]).contiguous()
    out = engine.empty(count, mod_n2.nwords)
    assert engine.lib.sc_modexp_var_sq(engine.ctx, mod_n.id, mod_n2.id, nb, engine._ptr(x), x.shape[-1], engine._ptr(e), ew, ebits, None,
                                       engine._ptr(out), count) == 0       # the per-row pair kernel itself, no fallback
    for mi in (None, engine.upload(mul, mod_n2.nwords)):
        got = engine.download(engine.modexp_var_sq(mod_n, mod_n2, x, e, ebits, mul_into=mi))
        for i in range(count):
            want = 1 if mi is None else mul[i]
            for j in range(nb):
                want = want * pow(xs[j][i], es[j][i], n2) % n2
            assert got[i] == want, (i, bits, nb)


def test_modexp_var_sq_ignores_bits_above_ebits_and_zero_ebits(engine, keys):
    sk = oracle_paillier(keys, 2048)
    mod_n, mod_n2 = engine.modulus(sk.n), engine.modulus(sk.n2)
    rng = random.Random(5)
    xs = [rng.randrange(sk.n2) for _ in range(70)]
    es = [rng.getrandbits(64) for _ in range(70)]
    x = engine.upload(xs, mod_n2.nwords).unsqueeze(0).contiguous()
    e = engine.upload(es, 2).unsqueeze(0).contiguous()
    got = engine.download(engine.modexp_var_sq(mod_n, mod_n2, x, e, 40))
    assert got == [pow(a, b & ((1 << 40) - 1), sk.n2) for a, b in zip(xs, es)]
    assert engine.download(engine.modexp_var_sq(mod_n, mod_n2, x, e, 0)) == [1] * 70


def test_modexp_var_sq_fallback_without_pair_kernel(engine):
    """A 512-bit modulus has no per-row pair instance: the same residues through sc_modexp_var modulo m^2 and sc_modmul."""
    from oracle import sc_oracle as o

    rng = random.Random(9)
    m = o.rand_prime(256, rng) * o.rand_prime(256, rng)
    mod_m, mod_m2 = engine.modulus(m), engine.modulus(m * m)
    xs = [[rng.randrange(m * m) for _ in range(33)] for _ in range(2)]
    es = [[rng.getrandbits(50) for _ in range(33)] for _ in range(2)]
    x = torch.stack([engine.upload(r, mod_m2.nwords) for r in xs]).contiguous()
    e = torch.stack([engine.upload(r, 2) for r in es]).contiguous()
    out = engine.empty(33, mod_m2.nwords)
    assert engine.lib.sc_modexp_var_sq(engine.ctx, mod_m.id, mod_m2.id, 2, engine._ptr(x), mod_m2.nwords, engine._ptr(e), 2, 50, None,
                                       engine._ptr(out), 33) == -4          # SC_ERR_UNSUPPORTED
    got = engine.download(engine.modexp_var_sq(mod_m, mod_m2, x, e, 50))
    assert got == [pow(xs[0][i], es[0][i], m * m) * pow(xs[1][i], es[1][i], m * m) % (m * m) for i in range(33)]


@pytest.mark.parametrize("bits", [1024, 2048])
def test_scalar_mul_batch(engine, keys, bits):
    sk = oracle_paillier(keys, bits)
    ap, _ = _paillier(engine, sk)
    rng = random.Random(bits)
    cs = [model.enc(sk, rng.getrandbits(64), rng.randrange(1, sk.n)) for _ in range(90)]
    ks = [0, 1, (1 << 96) - 1] + [rng.getrandbits(96) for _ in range(87)]
    got = engine.download(ap.scalar_mul_batch(engine.upload(cs, ap.mod_n2.nwords), engine.upload(ks, 3)))
    assert got == [pow(c, k, sk.n2) for c, k in zip(cs, ks)]


# ---- the three steps against the model ------------------------------------------------------------------------------------------------
def test_select_steps_bit_exact_vs_model(engine, keys):
    from protocols.secure_comparison_amd.selection import SelectDraws, SelectLayout, select_finish, select_mult, select_pack

    sk = oracle_paillier(keys, 2048)
    ap, bp = _paillier(engine, sk)
    n, kappa, widths, B = sk.n, 40, [32, 5], 37
    lay = SelectLayout(32, kappa, (5,), n.bit_length())
    rng = random.Random(77)
    sig = [rng.randrange(2) for _ in range(B)]
    a = [[rng.getrandbits(w) for _ in range(B)] for w in widths]
    b = [[rng.getrandbits(w) for _ in range(B)] for w in widths]
    sig_c = [model.enc(sk, s_, rng.randrange(1, n)) for s_ in sig]
    d_c = [[model.enc(sk, a[j][i] - b[j][i] + (1 << widths[j]), rng.randrange(1, n)) for i in range(B)] for j in range(2)]
    b_c = [[model.enc(sk, b[j][i], rng.randrange(1, n)) for i in range(B)] for j in range(2)]
    draws = [model.draw(rng, kappa, widths, n) for _ in range(B)]
    nw, nw2 = ap.mod_n.nwords, ap.mod_n2.nwords
    bw = (max(lay.fbits) + 31) // 32
    sd = SelectDraws(r_a=engine.upload([d[0] for d in draws], 2),
                     r_b=torch.stack([engine.upload([d[1][j] for d in draws], bw) for j in range(2)]).contiguous(),
                     rho_p=engine.upload([d[2] for d in draws], nw),
                     rho_products=torch.stack([engine.upload([d[3][j] for d in draws], nw) for j in range(2)]).contiguous())
    s_t = engine.upload(sig_c, nw2)
    d_t = torch.stack([engine.upload(r, nw2) for r in d_c]).contiguous()
    b_t = torch.stack([engine.upload(r, nw2) for r in b_c]).contiguous()
    P, plain = select_pack(lay, s_t, d_t, sd, ap)
    want_P = [model.pack(sk, kappa, widths, sig_c[i], [d_c[0][i], d_c[1][i]], draws[i][0], draws[i][1], draws[i][2]) for i in range(B)]
    assert engine.download(P) == want_P
    prods = select_mult(lay, P, bp, sd.rho_products)
    want = [model.mult(sk, kappa, widths, want_P[i], draws[i][3]) for i in range(B)]
    got_prods = _rows(engine, prods)
    assert got_prods == [want[i][0][j] for j in range(2) for i in range(B)]
    out = select_finish(lay, s_t, d_t, b_t, prods, plain, sd, ap)
    want_out = [model.finish(sk, kappa, widths, sig_c[i], [d_c[0][i], d_c[1][i]], [b_c[0][i], b_c[1][i]], want[i][0], draws[i][0],
                             draws[i][1]) for i in range(B)]
    got = _rows(engine, out)
    assert got == [want_out[i][j] for j in range(2) for i in range(B)]
    assert [model.dec(sk, c) for c in got[:B]] == [a[0][i] if sig[i] else b[0][i] for i in range(B)]


def test_select_mult_refuses_a_foreign_layout(engine, keys):
    from protocols.secure_comparison_amd.selection import SelectLayout, draw_select, select_mult, select_pack

    sk = oracle_paillier(keys, 1024)
    ap, bp = _paillier(engine, sk)
    big, small = SelectLayout(64, 40, (), sk.n.bit_length()), SelectLayout(16, 20, (), sk.n.bit_length())
    B = 8
    s_t = engine.upload([model.enc(sk, 1)] * B, ap.mod_n2.nwords)
    d_t = engine.upload([model.enc(sk, (1 << 64) + 12345)] * B, ap.mod_n2.nwords).unsqueeze(0).contiguous()
    P, _ = select_pack(big, s_t, d_t, draw_select(B, big, ap), ap)
    with pytest.raises(ValueError):
        select_mult(small, P, bp, draw_select(B, small, ap).rho_products)


# ---- decrypted results -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,pbits,dname,wide", [(16, 1024, "dgk_1024_l16", False), (32, 2048, "dgk_2048_l32", False),
                                                 (64, 2048, "dgk_2048_l64", False), (128, 2048, "dgk_2048_l128", True)])
def test_minimum_maximum_decrypt_to_python(engine, keys, l, pbits, dname, wide):
    from protocols.secure_comparison_amd.selection import secure_maximum_batch, secure_minimum_batch

    sk, ap, ad, bp, bd = _players(engine, keys, pbits, dname, wide)
    rng = random.Random(l)
    top = (1 << l) - 1
    xs = [0, 0, top, top, 1, top - 1, 5]
    ys = [0, top, 0, top, 1, top, 5]
    B = 1000 if l <= 64 else 300
    while len(xs) < B:
        x = rng.getrandbits(l)
        xs.append(x)
        ys.append(x if rng.random() < 0.1 else rng.getrandbits(l))
    nw2 = ap.mod_n2.nwords
    x_t = engine.upload([model.enc(sk, x) for x in xs], nw2)
    y_t = engine.upload([model.enc(sk, y) for y in ys], nw2)
    mn, d1 = secure_minimum_batch(x_t, y_t, l, ap, ad, bp, bd)
    mx, d2 = secure_maximum_batch(x_t, y_t, l, ap, ad, bp, bd)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t))  # noqa: E731
    assert dec(mn) == [min(x, y) for x, y in zip(xs, ys)]
    assert dec(mx) == [max(x, y) for x, y in zip(xs, ys)]
    assert dec(d1) == dec(d2) == [int(x <= y) for x, y in zip(xs, ys)]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 17])
def test_argmin_argmax_lowest_index_on_ties(engine, keys, k):
    from protocols.secure_comparison_amd.selection import secure_argmax_batch, secure_argmin_batch

    sk, ap, ad, bp, bd = _players(engine, keys, 1024, "dgk_1024_l16")
    l, B = 16, 64
    rng = random.Random(k)
    rows = []
    for b in range(B):
        pool = [0, 1, (1 << l) - 1, rng.getrandbits(l)] if b % 2 else [rng.getrandbits(l) for _ in range(4)]
        rows.append([rng.choice(pool) for _ in range(k)])        # many ties
    nw2 = ap.mod_n2.nwords
    v = torch.stack([engine.upload([model.enc(sk, x) for x in r], nw2) for r in rows]).contiguous()
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t))  # noqa: E731
    mv, mi = secure_argmin_batch(v, l, ap, ad, bp, bd)
    assert dec(mv) == [min(r) for r in rows]
    assert dec(mi) == [r.index(min(r)) for r in rows]
    xv, xi = secure_argmax_batch(v, l, ap, ad, bp, bd)
    assert dec(xv) == [max(r) for r in rows]
    assert dec(xi) == [r.index(max(r)) for r in rows]


# ---- two players over a communicator ------------------------------------------------------------------------------------------------
def _two_players(engine, keys, l, device_tensors=True, timeout_s=600.0):
    from protocols.secure_comparison_amd import InMemoryCommunicator, Initiator, KeyHolder

    sk, ap, ad, bp, bd = _players(engine, keys, 1024, "dgk_1024_l16")
    comm = InMemoryCommunicator(device_tensors=device_tensors, timeout_s=timeout_s)
    alice = Initiator(l, communicator=comm, other_party="keyholder")
    bob = KeyHolder(l, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    return sk, ap, bp, alice, bob


@pytest.mark.parametrize("device_tensors", [True, False])
def test_players_minimum_maximum(engine, keys, device_tensors):
    import asyncio

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, device_tensors)
    rng = random.Random(31)
    xs = [0, 65535, 7, 7] + [rng.getrandbits(16) for _ in range(96)]
    ys = [65535, 0, 7, 8] + [rng.getrandbits(16) for _ in range(96)]
    nw2 = ap.mod_n2.nwords
    x_t, y_t = engine.upload([model.enc(sk, x) for x in xs], nw2), engine.upload([model.enc(sk, y) for y in ys], nw2)
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.contiguous()))  # noqa: E731

    async def run():
        (mn, d1), _ = await asyncio.gather(alice.perform_secure_minimum_batch(x_t, y_t, engine=engine), bob.perform_secure_minimum_batch())
        (mx, d2), _ = await asyncio.gather(alice.perform_secure_maximum_batch(x_t, y_t, engine=engine), bob.perform_secure_maximum_batch())
        return mn, d1, mx, d2

    mn, d1, mx, d2 = asyncio.run(run())
    assert dec(mn) == [min(x, y) for x, y in zip(xs, ys)]
    assert dec(mx) == [max(x, y) for x, y in zip(xs, ys)]
    assert dec(d1) == dec(d2) == [int(x <= y) for x, y in zip(xs, ys)]


@pytest.mark.parametrize("k", [1, 5])
def test_players_argmin_argmax(engine, keys, k):
    import asyncio

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16)
    rng = random.Random(k)
    rows = [[rng.choice([3, 9, rng.getrandbits(16)]) for _ in range(k)] for _ in range(16)]
    v = torch.stack([engine.upload([model.enc(sk, x) for x in r], ap.mod_n2.nwords) for r in rows]).contiguous()
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.contiguous()))  # noqa: E731

    async def run():
        (mv, mi), _ = await asyncio.gather(alice.perform_secure_argmin_batch(v, engine=engine), bob.perform_secure_argmin_batch(k))
        (xv, xi), _ = await asyncio.gather(alice.perform_secure_argmax_batch(v, engine=engine), bob.perform_secure_argmax_batch(k))
        return mv, mi, xv, xi

    mv, mi, xv, xi = asyncio.run(run())
    assert dec(mv) == [min(r) for r in rows] and dec(mi) == [r.index(min(r)) for r in rows]
    assert dec(xv) == [max(r) for r in rows] and dec(xi) == [r.index(max(r)) for r in rows]


def test_players_refuse_a_different_kappa(engine, keys):
    import asyncio

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, timeout_s=30.0)
    nw2 = ap.mod_n2.nwords
    x_t = engine.upload([model.enc(sk, 5)] * 8, nw2)

    async def run():
        return await asyncio.gather(alice.perform_secure_minimum_batch(x_t, x_t, kappa=40, engine=engine),
                                    bob.perform_secure_minimum_batch(kappa=50), return_exceptions=True)

    got_a, got_b = asyncio.run(run())
    assert isinstance(got_b, ValueError) and "announces" in str(got_b)
    assert isinstance(got_a, Exception)          # the initiator never gets products back
    with pytest.raises(ValueError):
        asyncio.run(alice.perform_secure_minimum_batch(x_t, x_t, chunks=2, engine=engine))


# ---- the four families on one pair ---------------------------------------------------------------------------------------------------
class _Recorder:
    """An endpoint that keeps the message ids both players send, in order, in the shared `ids`."""

    def __init__(self, inner, ids):
        self.inner, self.ids, self.device_tensors = inner, ids, inner.device_tensors

    async def send(self, party, message, msg_id=None):
        self.ids.append(msg_id)
        await self.inner.send(party, message, msg_id=msg_id)

    async def recv(self, party, msg_id=None):
        return await self.inner.recv(party, msg_id=msg_id)


# Launches of the interpreter kernels (the sum of engine.launch_counts()) of minimum, multiply, dot and one-hot at B = 3 on the 1024-bit
# key, both players on one engine, once every key, table and modulus exists: the figures of the commit before the families shared
# exchange.py.  The host's exchange code decides none of them, so they hold exactly.
LAUNCHES = [62, 27, 33, 23]


def test_players_all_families_on_one_pair(engine, keys):
    """Minimum, one-column multiplication, inner product (k = 3 pairs of 200-bit operands: pairs of 482 bits, g = 2, M = 2 messages per
    row) and one-hot (k = 3, m = 2) in sequence on one Initiator / KeyHolder pair, twice: the message ids are those of the CPU transcript
    (tests/test_exchange_cpu.py) around the session's own, every result decrypts to plain Python's, and the second pass launches exactly
    LAUNCHES kernels per call."""
    import asyncio

    from protocols.secure_comparison_amd import DotLayout
    from test_exchange_cpu import TRANSCRIPT

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16)
    ids = []
    alice.communicator, bob.communicator = _Recorder(alice.communicator, ids), _Recorder(bob.communicator, ids)
    B, k_dot, bits, k_hot, m_hot = 3, 3, 200, 3, 2
    assert DotLayout(40, bits, bits, k_dot, nbits=sk.n.bit_length()).M == 2
    rng = random.Random(2027)
    nw2 = ap.mod_n2.nwords
    up = lambda vals: engine.upload([model.enc(sk, v) for v in vals], nw2)  # noqa: E731
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, nw2).contiguous()))  # noqa: E731
    xs, ys = [7, 65535, rng.getrandbits(16)], [7, 0, rng.getrandbits(16)]
    us = [[rng.getrandbits(bits) for _ in range(B)] for _ in range(k_dot)]
    vs = [[rng.getrandbits(bits) for _ in range(B)] for _ in range(k_dot)]
    idx = [[0, 2, 1], [1, 3, 2]]                                     # [m][B]; 3 is at or above k: marks 3 mod 3
    x_t, y_t = up(xs), up(ys)
    u_t, v_t = torch.stack([up(r) for r in us]).contiguous(), torch.stack([up(r) for r in vs]).contiguous()
    i_t = torch.stack([up(r) for r in idx]).contiguous()
    total = lambda: sum(engine.launch_counts().values())  # noqa: E731

    async def both(a, b):
        before = total()
        out, _ = await asyncio.gather(a, b)
        return out, total() - before

    async def run():
        return [await both(alice.perform_secure_minimum_batch(x_t, y_t, engine=engine), bob.perform_secure_minimum_batch()),
                await both(alice.perform_secure_multiply_batch(x_t, y_t, 16, 16, engine=engine), bob.perform_secure_multiply_batch(16, 16)),
                await both(alice.perform_secure_dot_batch(u_t, v_t, bits, bits, engine=engine), bob.perform_secure_dot_batch(k_dot, bits, bits)),
                await both(alice.perform_secure_onehot_batch(i_t, k_hot, engine=engine), bob.perform_secure_onehot_batch(k_hot, m_hot))]

    want_ids = []
    for sid, family in enumerate(["select", "mul", "dot", "onehot"] * 2, start=1):
        want_ids.append(f"schemes_batch_session_{sid}")
        if family == "select":
            want_ids += [f"step_{s}_batch_session_{sid}" for s in ("1", "4b", "4i", "5")]
        want_ids += [e[1].replace("session_1", f"session_{sid}") for e in TRANSCRIPT[family][1] if e[1].startswith(family + "_")]
    for _ in range(2):
        ((mn, le), n_min), (prod, n_mul), (dot, n_dot), (hot, n_hot) = asyncio.run(run())
        assert dec(mn) == [min(x, y) for x, y in zip(xs, ys)] and dec(le) == [int(x <= y) for x, y in zip(xs, ys)]
        assert dec(prod) == [x * y for x, y in zip(xs, ys)]
        assert dec(dot) == [sum(us[j][b] * vs[j][b] for j in range(k_dot)) for b in range(B)]
        assert dec(hot) == [int(t == idx[q][b] % k_hot) for q in range(m_hot) for t in range(k_hot) for b in range(B)]
    print("launches per call (minimum, multiply, dot, one-hot):", [n_min, n_mul, n_dot, n_hot])
    assert ids == want_ids
    assert [n_min, n_mul, n_dot, n_hot] == LAUNCHES

"""Secure sort on the GPU: sc_select_finish_cx bit for bit against Python pow / %, and secure_sort_batch / the two players decrypting
to the plaintext network (tests/_sort_model.py), ascending and descending, with payload and index columns and cut layers."""
import os
import random
import sys

import pytest
import torch

from conftest import oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _select_model as sm  # noqa: E402
import _sort_model as model  # noqa: E402
from test_gpu_select import _players, _two_players  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(engine, t):
    return engine.download(t.reshape(-1, t.shape[-1]).contiguous())


# ---- sc_select_finish_cx ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048, 3072])
@pytest.mark.parametrize("nf", [1, 2, 3, 4])
@pytest.mark.parametrize("indexed", [False, True])
def test_select_finish_cx_matches_pow(engine, keys, bits, nf, indexed):
    sk = oracle_paillier(keys, bits)
    n2 = sk.n2
    mod = engine.modulus(n2)
    nw = mod.nwords
    rng = random.Random(bits + 10 * nf + indexed)
    count = 37
    items = nf * count
    t = [rng.randrange(1, n2) for _ in range(items)]
    ab = [rng.randrange(1, n2) for _ in range(items)]
    f = [rng.randrange(n2) for _ in range(items)]
    g = [rng.randrange(n2) for _ in range(items)]
    t[0], ab[0], f[0], g[0] = 1, 1, n2 - 1, 0                       # edge residues
    u_inv = [pow(a * b % n2, -1, n2) for a, b in zip(t, ab)]
    up = lambda xs: engine.upload(xs, nw)  # noqa: E731
    args = (up(t), up(ab), up(u_inv), up(f).reshape(nf, count, nw).contiguous(), up(g).reshape(nf, count, nw).contiguous())
    want_hi = [x * b % n2 * b % n2 * u % n2 for x, b, u in zip(f, ab, u_inv)]
    want_lo = [y * a % n2 * a % n2 * u % n2 for y, a, u in zip(g, t, u_inv)]
    if not indexed:
        out = engine.select_finish_cx(mod, *args)
        assert tuple(out.shape) == (2, nf, count, nw)
        assert _rows(engine, out) == want_lo + want_hi
        return
    rows = 2 * items + 11                                            # more rows than outputs: some must stay untouched
    dest = rng.sample(range(rows), 2 * items)
    lo_i = torch.tensor(dest[:items], dtype=torch.int64, device=engine.device).reshape(nf, count)
    hi_i = torch.tensor(dest[items:], dtype=torch.int64, device=engine.device).reshape(nf, count)
    sentinel = [rng.randrange(n2) for _ in range(rows)]
    out = up(sentinel)
    engine.select_finish_cx(mod, *args, lo_index=lo_i, hi_index=hi_i, out=out)
    want = list(sentinel)
    for r, v in zip(dest, want_lo + want_hi):
        want[r] = v
    assert engine.download(out) == want


# ---- secure_sort_batch -----------------------------------------------------------------------------------------------------------------
def _rows_with_ties(rng, B, k, l):
    top = (1 << l) - 1
    out = []
    for b in range(B):
        pool = [0, top, 5, rng.getrandbits(l)] if b % 2 else [rng.getrandbits(l) for _ in range(3)]
        out.append([rng.choice(pool) for _ in range(k)])
    return out


def _enc_rows(engine, sk, rows, nw2, rng):
    flat = [sm.enc(sk, x, rng.randrange(1, sk.n)) for r in rows for x in r]
    return engine.upload(flat, nw2).reshape(len(rows), len(rows[0]), nw2).contiguous()


@pytest.mark.parametrize("l,pbits,dname,wide", [(16, 1024, "dgk_1024_l16", False), (32, 2048, "dgk_2048_l32", False),
                                                 (128, 2048, "dgk_2048_l128", True)])
def test_sort_decrypts_to_sorted_rows(engine, keys, l, pbits, dname, wide):
    from protocols.secure_comparison_amd.sorting import secure_sort_batch

    sk, ap, ad, bp, bd = _players(engine, keys, pbits, dname, wide)
    rng = random.Random(l)
    nw2 = ap.mod_n2.nwords
    for k in ((1, 2, 3, 5, 8, 17) if l <= 32 else (2, 5, 17)):
        B = 6
        rows = _rows_with_ties(rng, B, k, l)
        v = _enc_rows(engine, sk, rows, nw2, rng)
        for descending in (False, True):
            out, pay, idx = secure_sort_batch(v, l, ap, ad, bp, bd, descending=descending)
            assert pay is None and idx is None and tuple(out.shape) == (B, k, nw2)
            got = engine.download(bp.decrypt_raw_batch(out.reshape(-1, nw2).contiguous()))
            assert [got[b * k:(b + 1) * k] for b in range(B)] == [sorted(r, reverse=descending) for r in rows], (k, descending)


@pytest.mark.parametrize("k", [1, 5, 8, 17])
def test_sort_payload_and_indices_follow_the_network(engine, keys, k):
    from protocols.secure_comparison_amd.sorting import batcher_network, secure_sort_batch

    sk, ap, ad, bp, bd = _players(engine, keys, 1024, "dgk_1024_l16")
    rng = random.Random(500 + k)
    l, B, wp = 16, 5, (12, 20)
    nw2 = ap.mod_n2.nwords
    rows = _rows_with_ties(rng, B, k, l)
    pays = [[[rng.getrandbits(w) for _ in range(k)] for _ in range(B)] for w in wp]
    v = _enc_rows(engine, sk, rows, nw2, rng)
    p = torch.stack([_enc_rows(engine, sk, pr, nw2, rng) for pr in pays]).contiguous()
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, nw2).contiguous()))  # noqa: E731
    for descending in (False, True):
        results = []
        for max_rows in (65536, 7):                                   # 7: cut layers
            out, pay, idx = secure_sort_batch(v, l, ap, ad, bp, bd, payload=p, payload_bits=wp, descending=descending,
                                              return_indices=True, max_rows=max_rows)
            assert tuple(pay.shape) == (2, B, k, nw2) and tuple(idx.shape) == (B, k, nw2)
            results.append((dec(out), dec(pay), dec(idx)))
        assert results[0] == results[1]
        want = model.apply(batcher_network(k), [[(rows[b][i], pays[0][b][i], pays[1][b][i], i) for i in range(k)] for b in range(B)],
                           descending)
        got_v, got_p, got_i = results[0]
        for b in range(B):
            got = [(got_v[b * k + i], got_p[b * k + i], got_p[B * k + b * k + i], got_i[b * k + i]) for i in range(k)]
            assert got == [tuple(t) for t in want[b]], (k, descending, b)


# ---- two players ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_tensors", [True, False])
def test_players_sort(engine, keys, device_tensors):
    import asyncio

    from protocols.secure_comparison_amd.sorting import batcher_network

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, device_tensors)
    rng = random.Random(61)
    k, B, wp = 5, 8, (9,)
    nw2 = ap.mod_n2.nwords
    rows = _rows_with_ties(rng, B, k, 16)
    pays = [[rng.getrandbits(9) for _ in range(k)] for _ in range(B)]
    v = _enc_rows(engine, sk, rows, nw2, rng)
    p = _enc_rows(engine, sk, pays, nw2, rng).unsqueeze(0).contiguous()
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, nw2).contiguous()))  # noqa: E731

    async def run():
        (a, _, _), _ = await asyncio.gather(alice.perform_secure_sort_batch(v, engine=engine, descending=True),
                                            bob.perform_secure_sort_batch(k))
        (s, sp, si), _ = await asyncio.gather(
            alice.perform_secure_sort_batch(v, payload=p, payload_bits=wp, return_indices=True, max_rows=7, engine=engine),
            bob.perform_secure_sort_batch(k, payload_bits=wp, return_indices=True, max_rows=7))
        return a, s, sp, si

    a, s, sp, si = asyncio.run(run())
    got_a = dec(a)
    assert [got_a[b * k:(b + 1) * k] for b in range(B)] == [sorted(r, reverse=True) for r in rows]
    want = model.apply(batcher_network(k), [[(rows[b][i], pays[b][i], i) for i in range(k)] for b in range(B)])
    gv, gp, gi = dec(s), dec(sp), dec(si)
    assert [[(gv[b * k + i], gp[b * k + i], gi[b * k + i]) for i in range(k)] for b in range(B)] == [[tuple(t) for t in r] for r in want]


@pytest.mark.parametrize("bob_kw", [{"k": 4}, {"k": 5, "payload_bits": (10,)}, {"k": 5, "kappa": 50}])
def test_players_refuse_a_different_sort(engine, keys, bob_kw):
    import asyncio

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, timeout_s=15.0)
    rng = random.Random(3)
    nw2 = ap.mod_n2.nwords
    rows = _rows_with_ties(rng, 4, 5, 16)
    v = _enc_rows(engine, sk, rows, nw2, rng)
    p = _enc_rows(engine, sk, rows, nw2, rng).unsqueeze(0).contiguous()

    async def run():
        return await asyncio.gather(alice.perform_secure_sort_batch(v, payload=p, payload_bits=(9,), engine=engine),
                                    bob.perform_secure_sort_batch(**{"payload_bits": (9,), **bob_kw}), return_exceptions=True)

    got_a, got_b = asyncio.run(run())
    assert isinstance(got_b, ValueError) and "announces" in str(got_b)
    assert isinstance(got_a, Exception)                 # the initiator never gets a comparison session back
    with pytest.raises(ValueError):
        asyncio.run(alice.perform_secure_sort_batch(v, chunks=2, engine=engine))

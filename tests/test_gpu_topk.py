"""Secure top-m on the GPU: secure_topk_batch / secure_kth_batch / secure_median_batch and the two players decrypt to the plaintext
network with keep flags (tests/_topk_model.py) -- values, two payload columns and indices, the smallest and the largest, whole and
cut layers -- and a dead output is never written: the buffer rows no live output goes to stay bit-identical to their input."""
import asyncio
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _topk_model as model  # noqa: E402
from test_gpu_select import _players, _two_players  # noqa: E402
from test_gpu_sort import _enc_rows, _rows_with_ties  # noqa: E402

pytestmark = pytest.mark.gpu

WP = (12, 20)       # the widths of the two payload columns


def _case(engine, sk, ap, rng, B, k, l):
    """Rows with ties, two payload columns, their encryptions, and the model's input tuples (key, payload 0, payload 1, index)."""
    nw2 = ap.mod_n2.nwords
    rows = _rows_with_ties(rng, B, k, l)
    pays = [[[rng.getrandbits(w) for _ in range(k)] for _ in range(B)] for w in WP]
    v = _enc_rows(engine, sk, rows, nw2, rng)
    p = torch.stack([_enc_rows(engine, sk, pr, nw2, rng) for pr in pays]).contiguous()
    tuples = [[(rows[b][i], pays[0][b][i], pays[1][b][i], i) for i in range(k)] for b in range(B)]
    return rows, v, p, tuples


def _dec(engine, bp, t):
    return engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))


def _got(engine, bp, out, pay, idx, B, m):
    """[B][m] tuples (key, payload 0, payload 1, index) of a result ([B][m][2nw], [2][B][m][2nw], [B][m][2nw])."""
    gv, gp, gi = _dec(engine, bp, out), _dec(engine, bp, pay), _dec(engine, bp, idx)
    return [[(gv[b * m + i], gp[b * m + i], gp[B * m + b * m + i], gi[b * m + i]) for i in range(m)] for b in range(B)]


def _check_topk(engine, keys, k, m, l, pbits, dname, largest=False, max_rows=65536, seed=0):
    from protocols.secure_comparison_amd.sorting import secure_topk_batch, topk_network

    sk, ap, ad, bp, bd = _players(engine, keys, pbits, dname)
    B = 6
    rows, v, p, tuples = _case(engine, sk, ap, random.Random(1000 * k + m + seed), B, k, l)
    nw2 = ap.mod_n2.nwords
    out, pay, idx = secure_topk_batch(v, m, l, ap, ad, bp, bd, payload=p, payload_bits=WP, largest=largest, return_indices=True,
                                      max_rows=max_rows)
    assert tuple(out.shape) == (B, m, nw2) and tuple(pay.shape) == (2, B, m, nw2) and tuple(idx.shape) == (B, m, nw2)
    want = model.apply(topk_network(k, m), tuples, largest)
    assert _got(engine, bp, out, pay, idx, B, m) == [[tuple(t) for t in r[:m]] for r in want]
    assert [[t[0] for t in r[:m]] for r in want] == [sorted(r, reverse=largest)[:m] for r in rows]


# (5, 2): truncated merges, a half-cleaner with a dropped index; (9, 3): k no power of two, the pruned full sort wins by one
# comparator (22 against 23); (9, 4): the same k where the truncated merges win, two merge rounds; (8, 8): the sort; (17, 1): every
# comparator has one live output
@pytest.mark.parametrize("k,m", [(5, 2), (9, 3), (9, 4), (8, 8), (17, 1)])
def test_topk_values_payload_and_indices_follow_the_network(engine, keys, k, m):
    _check_topk(engine, keys, k, m, 16, 1024, "dgk_1024_l16")


def test_topk_l32_2048_bits(engine, keys):
    _check_topk(engine, keys, 5, 2, 32, 2048, "dgk_2048_l32")            # 7 comparators: the wide keys cost seconds per layer


@pytest.mark.parametrize("k,m", [(9, 3), (5, 2)])
def test_topk_largest(engine, keys, k, m):
    _check_topk(engine, keys, k, m, 16, 1024, "dgk_1024_l16", largest=True)


def test_topk_cut_layer_mixes_live_and_dead_outputs(engine, keys):
    from protocols.secure_comparison_amd.sorting import topk_schedule

    B, k, m, max_rows = 6, 9, 3, 4
    mixed = [(layer, cuts) for layer, cuts in topk_schedule(k, m, False, B, max_rows)
             if any(ki and kj for _, _, ki, kj in layer) and any(not (ki and kj) for _, _, ki, kj in layer)]
    assert mixed and all(len(cuts) > 1 for _, cuts in mixed)             # such layers exist and every one of them is cut
    # max_rows < B: a sub-batch never holds a whole comparator, so some hold rows of a live and of a dead one
    _check_topk(engine, keys, k, m, 16, 1024, "dgk_1024_l16", max_rows=max_rows, seed=1)
    _check_topk(engine, keys, k, m, 16, 1024, "dgk_1024_l16", largest=True, max_rows=7, seed=2)


# positions no live output ever goes to.  (9, 3): none -- its dead outputs land on positions written earlier, so there the decrypted
# buffer is the witness; (17, 1) is a tournament: position 0 collects the minimum and no loser is ever written
@pytest.mark.parametrize("k,m,never_written", [(9, 3, []), (17, 1, [1, 3, 5, 7, 9, 11, 13, 15, 16])])
def test_dead_outputs_are_not_written(engine, keys, k, m, never_written):
    """The whole buffer after a run: every position decrypts to what the model leaves there when a dead output is not written (a
    position whose last output is dead keeps the value of its last live one), and the rows no live output ever goes to are the
    input ciphertexts bit for bit, while every written row is a fresh ciphertext."""
    from protocols.secure_comparison_amd.sorting import _topk_buffer, topk_network

    sk, ap, ad, bp, bd = _players(engine, keys, 1024, "dgk_1024_l16")
    B, l = 6, 16
    rows, v, p, tuples = _case(engine, sk, ap, random.Random(93 + k), B, k, l)
    nw2 = ap.mod_n2.nwords
    layers = topk_network(k, m)
    untouched = sorted(set(range(k)) - model.written(layers, k))
    assert untouched == never_written and any(not (ki and kj) for layer in layers for _, _, ki, kj in layer)
    v_before, p_before = v.clone(), p.clone()
    buf = _topk_buffer(v, m, False, l, ap, ad, bp, bd, p, WP, False, True, 40, 65536)
    assert tuple(buf.shape) == (4, B * k, nw2)
    assert torch.equal(v, v_before) and torch.equal(p, p_before)         # the inputs themselves are never written
    cols = [_dec(engine, bp, buf[c]) for c in range(4)]
    got = [[tuple(cols[c][b * k + i] for c in range(4)) for i in range(k)] for b in range(B)]
    assert got == [[tuple(t) for t in r] for r in model.apply(layers, tuples)]
    before = torch.cat([v_before.reshape(1, B * k, nw2), p_before.reshape(2, B * k, nw2)])
    at = torch.tensor([b * k + i for b in range(B) for i in untouched], dtype=torch.int64, device=buf.device)
    assert torch.equal(buf[:3].index_select(1, at), before.index_select(1, at))
    touched = torch.tensor([b * k + i for b in range(B) for i in sorted(model.written(layers, k))], dtype=torch.int64, device=buf.device)
    assert not (buf[:3].index_select(1, touched) == before.index_select(1, touched)).all(dim=-1).any()


def test_kth_and_median(engine, keys):
    from protocols.secure_comparison_amd.sorting import secure_kth_batch, secure_median_batch, topk_network

    sk, ap, ad, bp, bd = _players(engine, keys, 1024, "dgk_1024_l16")
    B, k, l = 6, 9, 16
    rows, v, p, tuples = _case(engine, sk, ap, random.Random(94), B, k, l)
    nw2 = ap.mod_n2.nwords
    for kth, largest in ((6, False), (2, True)):
        out, pay, idx = secure_kth_batch(v, kth, l, ap, ad, bp, bd, payload=p, payload_bits=WP, largest=largest, return_indices=True)
        assert tuple(out.shape) == (B, nw2) and tuple(pay.shape) == (2, B, nw2) and tuple(idx.shape) == (B, nw2)
        want = model.apply(topk_network(k, kth + 1, True), tuples, largest)
        assert [r[0] for r in _got(engine, bp, out, pay, idx, B, 1)] == [tuple(r[kth]) for r in want]
        assert _dec(engine, bp, out) == [sorted(r, reverse=largest)[kth] for r in rows]
    out, pay, idx = secure_median_batch(v, l, ap, ad, bp, bd, return_indices=True)
    assert pay is None and tuple(out.shape) == (B, nw2)
    med, at = _dec(engine, bp, out), _dec(engine, bp, idx)
    assert med == [sorted(r)[4] for r in rows] and [rows[b][at[b]] for b in range(B)] == med
    out, pay, idx = secure_median_batch(v[:, :8].contiguous(), l, ap, ad, bp, bd)               # k even: the lower median
    assert pay is None and idx is None and _dec(engine, bp, out) == [sorted(r[:8])[3] for r in rows]


# ---- two players ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_tensors", [True, False])
def test_players_topk(engine, keys, device_tensors):
    from protocols.secure_comparison_amd.sorting import topk_network

    sk, ap, bp, alice, bob = _two_players(engine, keys, 16, device_tensors)
    B, k, m = 6, 9, 3
    rows, v, p, tuples = _case(engine, sk, ap, random.Random(95), B, k, 16)
    nw2 = ap.mod_n2.nwords

    async def run():
        top, _ = await asyncio.gather(
            alice.perform_secure_topk_batch(v, m, payload=p, payload_bits=WP, return_indices=True, max_rows=7, engine=engine),
            bob.perform_secure_topk_batch(k, m, payload_bits=WP, return_indices=True, max_rows=7))
        (last, _, _), _ = await asyncio.gather(alice.perform_secure_topk_batch(v, m, largest=True, only_last=True, engine=engine),
                                               bob.perform_secure_topk_batch(k, m, only_last=True))
        return top, last

    (out, pay, idx), last = asyncio.run(run())
    want = model.apply(topk_network(k, m), tuples)
    assert _got(engine, bp, out, pay, idx, B, m) == [[tuple(t) for t in r[:m]] for r in want]
    assert tuple(last.shape) == (B, nw2) and _dec(engine, bp, last) == [sorted(r, reverse=True)[m - 1] for r in rows]


@pytest.mark.parametrize("bob_kw", [{"m": 2}, {"only_last": True}, {"payload_bits": (10,)}, {"return_indices": True}])
def test_key_holder_refuses_a_different_topk(engine, keys, bob_kw):
    sk, ap, bp, alice, bob = _two_players(engine, keys, 16)
    rng = random.Random(3)
    nw2 = ap.mod_n2.nwords
    rows = _rows_with_ties(rng, 4, 9, 16)
    v = _enc_rows(engine, sk, rows, nw2, rng)
    p = _enc_rows(engine, sk, rows, nw2, rng).unsqueeze(0).contiguous()

    async def run():
        a = asyncio.ensure_future(alice.perform_secure_topk_batch(v, 3, payload=p, payload_bits=(9,), engine=engine))
        b = asyncio.ensure_future(bob.perform_secure_topk_batch(**{"k": 9, "m": 3, "payload_bits": (9,), **bob_kw}))
        await asyncio.wait([b])
        done = a.done()                                 # the initiator still waits for an answer that never comes: stop her
        a.cancel()
        await asyncio.gather(a, return_exceptions=True)
        return b.exception(), done

    err, alice_done = asyncio.run(run())
    assert isinstance(err, ValueError) and "topk: the initiator announces" in str(err)
    assert not alice_done
    with pytest.raises(ValueError):
        asyncio.run(alice.perform_secure_topk_batch(v, 3, chunks=2, engine=engine))

"""The wrap-row table (tests/_wrap_rows.py) without a GPU: it reaches what it promises for every (key, l) the GPU module runs, its
prediction -- written from the carries, not from a run -- is what oracle.compare decrypts to on every row, and the product's
Python layer on the stand-in engine equals the oracle on those rows residue for residue."""
import collections

import pytest
import torch

import _wrap_oracle as WO
import _wrap_rows as W
from oracle import sc_oracle as o


@pytest.mark.parametrize("name", sorted(WO.WORLDS))
def test_the_table_reaches_what_it_promises(keys, name):
    sk, dgk, l, _ = WO.world(keys, name)
    n, table, promise = sk.n, W.rows(sk.n, l), W.promised(sk.n, l)
    assert dgk.u > 1 << (l + 2) and (1 << (l + 2)) < n // 2            # the keys satisfy the guards of steps 1 and 4a
    assert len(set(promise)) == len(promise) and W.reached(n, l, table) == set(promise), W.reached(n, l, table) ^ set(promise)
    assert all(0 <= r.r < n and 0 <= r.x < 1 << l and 0 <= r.y < 1 << l and r.delta_a in (0, 1) for r in table)
    edges = {**W.r_edges(n, l), **W.z_edges(n, l)}
    assert len(edges) == len(W.R_EDGES) + len(W.Z_EDGES) and set(edges) <= set(promise)      # every boundary lies in [0, N) for these keys
    for skip in (0, 501):
        sub = W.cover(n, l, 40, skip)
        assert len(sub) <= 40 and len(set(sub)) == len(sub) and W.reached(n, l, sub) == set(promise)
    assert set(W.cover(n, l, 40, 0)) != set(W.cover(n, l, 40, 501)) or len(table) <= 200
    # the wrap cell is r in [N - 2^(l+1), N) with z below 2^(l+1); the protocol is wrong nowhere else, and where it is wrong
    # the value is the complement or no bit at all
    seen = collections.Counter()
    for row in table:
        c, v = W.conditions(n, l, row), W.protocol_value(n, l, row)
        assert c.wrap == int(row.r >= n - (2 << l) and (1 << l) + row.r + row.y - row.x >= n)
        assert W.protocol_is_right(n, l, row) == (v == c.le) and (c.wrap or v == c.le) and v in (0, 1, 2, n - 1)
        seen[(c.wrap, v if v < 3 else -1)] += 1
    assert {v for (w, v) in seen if w} == {0, 1, 2, -1}
    # the counts DESIGN.md §5 states: rows, rows the protocol gets wrong, of which the value is no bit (2, -1)
    wrong = W.wrong_rows(n, l)
    assert (len(table), len(wrong), seen[(1, 2)], seen[(1, -1)]) == {1: (128, 7, 1, 2), 128: (1680, 78, 9, 16)}.get(l, (1260, 58, 7, 12))
    with pytest.raises(ValueError):
        W.cover(n, l, 10)
    with pytest.raises(ValueError):
        W.promised(n, 3)


# rows the issue's probe named (l = 16): (x, y, N - r, delta_a) -> the plaintext
@pytest.mark.parametrize("x, y, k, delta_a, value", [(5, 6, 1, 0, 0), (5, 6, 1, 1, 0), (5, 6, 2, 1, 0), (5, 6, 2, 0, 1), (65535, 0, 1, 0, -1),
                                                     (0, 65535, 65536, 0, 2), (0, 65535, 65536, 1, 2)])
def test_the_prediction_on_the_rows_that_started_this(keys, x, y, k, delta_a, value):
    sk, dgk, l, rbits = WO.world(keys, "tiny_l16")
    row = W.Row(x, y, sk.n - k, delta_a)
    assert W.conditions(sk.n, l, row).wrap and W.protocol_value(sk.n, l, row) == value % sk.n
    got = WO.traces([row], l, sk, dgk, WO.planted_draws([row], l, sk, dgk, rbits, 0), True)[0]["result"]
    assert sk.dec_raw(got) == value % sk.n


@pytest.mark.parametrize("name", ["tiny_l16", "l1", "l5"])
def test_oracle_decrypts_to_the_prediction_on_every_row(keys, name):
    """The static step chain on the whole table (the plaintext does not depend on the randomizers)."""
    sk, dgk, l, rbits = WO.world(keys, name)
    table = W.rows(sk.n, l)
    got = WO.traces(table, l, sk, dgk, WO.planted_draws(table, l, sk, dgk, rbits, 1), False, workers=16)
    for row, t in zip(table, got):
        assert t["z"] == ((1 << l) + row.r + row.y - row.x) % sk.n
        assert sk.dec_raw(t["result"]) == W.protocol_value(sk.n, l, row), row


@pytest.mark.parametrize("name", ["1024_l16", "2048_l32", "l65", "l128"])
def test_oracle_decrypts_to_the_prediction_on_the_rows_the_gpu_runs(keys, name):
    sk, dgk, l, rbits = WO.world(keys, name)
    table = tuple(dict.fromkeys(W.cover(sk.n, l, 40, 0) + W.cover(sk.n, l, 40, 501) + W.wrong_rows(sk.n, l)))
    got = WO.traces(table, l, sk, dgk, WO.planted_draws(table, l, sk, dgk, rbits, 2), False, workers=16)
    assert [sk.dec_raw(t["result"]) for t in got] == [W.protocol_value(sk.n, l, row) for row in table]


@pytest.mark.parametrize("name, use_crt", [("tiny_l16", True), ("tiny_l16", False), ("l1", True), ("l5", True)])
def test_python_layer_on_the_stand_in_engine_equals_the_oracle(keys, name, use_crt):
    """secure_comparison_batch on tests/_oracle_engine.py (one flag word: l <= 64), with and without randomizers, every traced
    value against oracle.compare's."""
    from _oracle_engine import OracleEngine
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.batch import BatchTrace, secure_comparison_batch
    from test_host_logic_cpu import make_draws

    sk, dgk, l, rbits = WO.world(keys, name)
    eng = OracleEngine()
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=eng, use_crt=use_crt)
    bob_d = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=eng, randomizer_bits=rbits)
    table = W.cover(sk.n, l, 40, 0)
    assert W.reached(sk.n, l, table) == set(W.promised(sk.n, l))
    drs = WO.planted_draws(table, l, sk, dgk, rbits, 3)
    nw = bob_p.mod_n.nwords
    draws = make_draws(eng, drs, l, nw, (dgk.u.bit_length() + 31) // 32, (rbits + 31) // 32)
    for randomize in (True, False):
        want = WO.traces(table, l, sk, dgk, drs, randomize, workers=16)
        tr = BatchTrace()
        got = secure_comparison_batch(eng.upload([sk.enc_raw(r.x) for r in table], 2 * nw), eng.upload([sk.enc_raw(r.y) for r in table], 2 * nw),
                                      l, bob_p.public_copy(), bob_d.public_copy(), bob_p, bob_d, draws, randomize, tr)
        assert eng.download(got) == [t["result"] for t in want]
        assert eng.download(tr.z_enc) == [t["z_enc"] for t in want] and eng.download(tr.z) == [t["z"] for t in want]
        assert eng.download(tr.d_enc) == [t["d_sent"] for t in want]
        assert [eng.download(tr.beta_enc[:, b]) for b in range(len(table))] == [t["beta_enc"] for t in want]
        assert [eng.download(tr.c_sent[:, b]) for b in range(len(table))] == [t["c_enc"] for t in want]
        assert [int(v) for v in tr.delta_b.tolist()] == [t["delta_b"] for t in want]
        assert eng.download(tr.zeta_1_enc) == [t["zeta1"] for t in want] and eng.download(tr.zeta_2_enc) == [t["zeta2"] for t in want]
        assert eng.download(tr.delta_b_enc) == [t["delta_b_enc"] for t in want]
        assert [sk.dec_raw(v) for v in eng.download(got)] == [W.protocol_value(sk.n, l, row) for row in table]
    assert isinstance(got, torch.Tensor)


def test_planted_sessions_on_the_stand_in_engine(keys):
    """Sixteen concurrent single comparisons whose streams are planted to wrap, through the coalescer and one by one."""
    from _oracle_engine import OracleEngine
    from protocols.secure_comparison_amd import DGK, Paillier

    sk, dgk, l, rbits = WO.world(keys, "tiny_l16")
    eng = OracleEngine()
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=eng)
    bob_d = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=eng, randomizer_bits=rbits)
    stats = WO.check_sessions(WO.session_rows(sk.n, l), l, sk, dgk, bob_p, bob_d)
    assert stats["alice"]["largest"] == 16 and stats["alice"]["fallbacks"] == 0

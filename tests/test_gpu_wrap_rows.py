"""Whole comparisons on the GPU at the rows of tests/_wrap_rows.py: r planted so that 2^l + r + y - x wraps around N, [d] = Enc(1)
survives step 4c, alpha~ decides, w_i can be -1, the c_i are negative residues modulo u and step 7 takes zeta_2 = (z + N) >> l.
Every case is bit for bit against oracle.compare and its trace, and every decrypted result is the value predicted from the carries
(_wrap_rows.protocol_value) -- on some of these rows that is not [x <= y], and the library has to be wrong in the same way."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _wrap_oracle as WO  # noqa: E402
import _wrap_rows as W  # noqa: E402
from test_gpu_parity import _draw_tensors, _schemes  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0x5A5A5A5A
_REFERENCE = {}


def _reference(keys, name, randomize, skip=0):
    """(sk, dgk, l, rbits, rows, oracle draws, oracle traces) of a named case, computed once for every test that runs it."""
    key = (name, randomize, skip)
    if key not in _REFERENCE:
        sk, dgk, l, rbits = WO.world(keys, name)
        rows = W.cover(sk.n, l, 40, skip)
        assert len(rows) <= 40 and W.reached(sk.n, l, rows) == set(W.promised(sk.n, l))       # dropping rows kept every condition
        drs = WO.planted_draws(rows, l, sk, dgk, rbits, skip)
        _REFERENCE[key] = (sk, dgk, l, rbits, rows, drs, WO.traces(rows, l, sk, dgk, drs, randomize, workers=16))
    return _REFERENCE[key]


def _run_batch(engine, ref, use_crt, randomize):
    from protocols.secure_comparison_amd.batch import BatchTrace, secure_comparison_batch

    sk, dgk, l, rbits, rows, drs, want = ref
    B, n = len(rows), sk.n
    alice_p, alice_d, bob_p, bob_d = _schemes(engine, sk, dgk, rbits, use_crt)
    nw = bob_p.mod_n.nwords
    draws = _draw_tensors(engine, drs, l, nw, (dgk.u.bit_length() + 31) // 32, (rbits + 31) // 32, engine.device)
    tx, ty = engine.upload([sk.enc_raw(r.x) for r in rows], 2 * nw), engine.upload([sk.enc_raw(r.y) for r in rows], 2 * nw)
    inputs = [tx, ty] + [getattr(draws, f) for f in ("r", "delta_a", "rhos", "permutation", "rho_z", "r_bob_dgk", "r_alice_dgk", "rho_zeta_1",
                                                      "rho_zeta_2", "rho_delta_b")]
    clones = [t.clone() for t in inputs]
    buf = torch.full((B + 2, 2 * nw), GUARD, dtype=torch.int32, device=engine.device)
    tr = BatchTrace()
    res = secure_comparison_batch(tx, ty, l, alice_p, alice_d, bob_p, bob_d, draws, randomize, tr, out=buf[1:B + 1])
    torch.cuda.synchronize()
    assert res.data_ptr() == buf[1].data_ptr() and bool((buf[0] == GUARD).all()) and bool((buf[B + 1] == GUARD).all())
    assert all(torch.equal(a, b) for a, b in zip(inputs, clones))
    got = engine.download(res)
    assert engine.download(tr.z) == [t["z"] for t in want] == [((1 << l) + r.r + r.y - r.x) % n for r in rows]
    assert engine.download(tr.z_enc) == [t["z_enc"] for t in want]
    assert engine.download(tr.d_enc) == [t["d_sent"] for t in want]
    assert [engine.download(tr.beta_enc[:, b]) for b in range(B)] == [t["beta_enc"] for t in want]
    assert [engine.download(tr.c_sent[:, b]) for b in range(B)] == [t["c_enc"] for t in want]
    assert [int(v) for v in tr.delta_b.tolist()] == [t["delta_b"] for t in want]
    assert engine.download(tr.zeta_1_enc) == [t["zeta1"] for t in want] and engine.download(tr.zeta_2_enc) == [t["zeta2"] for t in want]
    assert engine.download(tr.delta_b_enc) == [t["delta_b_enc"] for t in want]
    assert got == [t["result"] for t in want]
    value = [sk.dec_raw(c) for c in got]
    assert value == [W.protocol_value(n, l, r) for r in rows]
    assert [v == int(r.x <= r.y) for v, r in zip(value, rows)] == [W.protocol_is_right(n, l, r) for r in rows]
    dec = engine.download(bob_p.decrypt_raw_batch(res.contiguous()))                # the library's own decryption reads the same values
    assert dec == value


@pytest.mark.parametrize("use_crt, randomize", [(True, True), (False, True), (True, False), (False, False)])
def test_batch_1024_l16(engine, keys, use_crt, randomize):
    """secure_comparison_batch, 1024-bit Paillier with dgk_1024_l16: the key holder's CRT and literal paths, randomized and static."""
    _run_batch(engine, _reference(keys, "1024_l16", randomize, 0 if randomize else 501), use_crt, randomize)


@pytest.mark.parametrize("name", ["l1", "l5", "2048_l32", "l65", "l128"])
def test_batch_other_bit_lengths(engine, keys, name):
    """l = 1 (a single bit: alpha~ is the complement of alpha) and l = 5 on a DGK key made for u = next_prime(2^(l+2)), 2048-bit keys
    with l = 32, and l = 65 and 128 on the flag-row path."""
    _run_batch(engine, _reference(keys, name, True), True, True)


def test_batch_small_batch_kernels(latency_engine, keys):
    _run_batch(latency_engine, _reference(keys, "2048_l32", True), True, True)


def test_batch_one_lane_kernels(onelane_engine, keys):
    _run_batch(onelane_engine, _reference(keys, "2048_l32", True), True, True)


def test_sessions_planted_to_wrap(engine, keys):
    """perform_secure_comparison: sixteen concurrent sessions whose streams are planted to wrap, through the coalescer, and the same
    sessions one after the other through the fused single comparison -- every message equal, z, [d], the beta bits and the zetas
    the rows' own, and every result the predicted value."""
    from protocols.secure_comparison_amd import DGK, Paillier

    sk, dgk, l, rbits = WO.world(keys, "1024_l16")
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=engine)
    bob_d = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=engine, randomizer_bits=rbits)
    engine.set_latency_mode(1)
    try:
        stats = WO.check_sessions(WO.session_rows(sk.n, l), l, sk, dgk, bob_p, bob_d)
    finally:
        engine.set_latency_mode(0)
        bob_p.shut_down()
    for side in ("alice", "bob"):
        assert stats[side]["largest"] == 16 and stats[side]["fallbacks"] == 0


def test_minimum_and_maximum_on_wrap_draws(engine, keys):
    """secure_minimum_batch / secure_maximum_batch take the comparison's draws: one batch of the wrap cell's rows on which the
    comparison returns a bit, against the selection's model at the level of plaintexts (min, max and the bit)."""
    import random

    import _select_model as model
    from protocols.secure_comparison_amd.selection import secure_maximum_batch, secure_minimum_batch

    sk, dgk, l, rbits, rows, drs, _ = _reference(keys, "1024_l16", True)
    keep = [i for i, r in enumerate(rows) if W.conditions(sk.n, l, r).wrap and W.protocol_is_right(sk.n, l, r)]
    assert len(keep) >= 6
    rows, drs = [rows[i] for i in keep], [drs[i] for i in keep]
    alice_p, alice_d, bob_p, bob_d = _schemes(engine, sk, dgk, rbits)
    nw = bob_p.mod_n.nwords
    draws = _draw_tensors(engine, drs, l, nw, (dgk.u.bit_length() + 31) // 32, (rbits + 31) // 32, engine.device)
    tx, ty = engine.upload([sk.enc_raw(r.x) for r in rows], 2 * nw), engine.upload([sk.enc_raw(r.y) for r in rows], 2 * nw)
    mn, d1 = secure_minimum_batch(tx, ty, l, alice_p, alice_d, bob_p, bob_d, draws)
    mx, d2 = secure_maximum_batch(tx, ty, l, alice_p, alice_d, bob_p, bob_d, draws)
    dec = lambda t: engine.download(bob_p.decrypt_raw_batch(t.contiguous()))  # noqa: E731
    rng = random.Random(5)
    assert dec(mn) == [model.minimum(sk, r.x, r.y, l, rng) for r in rows] == [min(r.x, r.y) for r in rows]
    assert dec(mx) == [model.maximum(sk, r.x, r.y, l, rng) for r in rows] == [max(r.x, r.y) for r in rows]
    assert dec(d1) == dec(d2) == [int(r.x <= r.y) for r in rows]


@pytest.mark.parametrize("flags", [0, 1])
def test_scheme_level_c_abi(keys, flags):
    """The five scheme-level entry points of include/sc_amd.h driven with ctypes alone (flags 1 = SC_KEY_NO_CRT), every output of
    every call against the rows' plain values and the oracle's trace."""
    import ctypes as C

    import numpy as np

    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.limbs import ints_to_words, words_to_ints

    sk, dgk, l, rbits, rows, drs, want = _reference(keys, "1024_l16", True)
    lib = _lib.load()
    B, n = len(rows), sk.n
    nw = nd = 32
    ew, er = (dgk.u.bit_length() + 31) // 32, (rbits + 31) // 32

    def words(v, w):
        a = ints_to_words([v], w)
        return a, a.ctypes.data_as(C.c_void_p)

    ctx = C.c_void_p()
    assert lib.sc_ctx_create(0, C.byref(ctx)) == 0
    live = []

    def dev(host):
        p = C.c_void_p()
        assert lib.sc_malloc(ctx, max(host.nbytes, 4), C.byref(p)) == 0
        assert lib.sc_memcpy_h2d(ctx, p, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0
        live.append(p)
        return p

    def empty(*shape, dtype=np.uint32):
        return dev(np.zeros(shape, dtype=dtype))

    def back(p, *shape, dtype=np.uint32):
        out = np.zeros(shape, dtype=dtype)
        assert lib.sc_memcpy_d2h(ctx, out.ctypes.data_as(C.c_void_p), p, out.nbytes) == 0
        return out

    def planes(per_row, w):      # [l+1][B][w] bit-major from per-comparison lists
        return np.stack([ints_to_words([per_row[b][i] for b in range(B)], w) for i in range(l + 1)])

    try:
        keep = [words(n, nw), words(sk.p, nw // 2), words(sk.q, nw // 2)]
        a_key, b_key = C.c_int(), C.c_int()
        assert lib.sc_paillier_key_create(ctx, keep[0][1], nw, None, None, 0, 0, C.byref(a_key)) == 0, lib.sc_last_error(ctx)
        assert lib.sc_paillier_key_create(ctx, keep[0][1], nw, keep[1][1], keep[2][1], nw // 2, flags, C.byref(b_key)) == 0, lib.sc_last_error(ctx)
        dk = [words(dgk.n, nd), words(dgk.g, nd), words(dgk.h, nd), words(dgk.u, ew), words(dgk.p, nd // 2), words(dgk.q, nd // 2),
              words(dgk.v_p, 5), words(dgk.v_q, 5)]
        a_dgk, b_dgk = C.c_int(), C.c_int()
        assert lib.sc_dgk_key_create(ctx, dk[0][1], dk[1][1], dk[2][1], nd, dk[3][1], ew, dgk.t, None, None, 0, None, None, 0, rbits, 8, 0,
                                     None, -1, C.byref(a_dgk)) == 0, lib.sc_last_error(ctx)
        assert lib.sc_dgk_key_create(ctx, dk[0][1], dk[1][1], dk[2][1], nd, dk[3][1], ew, dgk.t, dk[4][1], dk[5][1], nd // 2, dk[6][1], dk[7][1], 5,
                                     rbits, 8, flags, None, -1, C.byref(b_dgk)) == 0, lib.sc_last_error(ctx)
        # Alice: steps 1, 3 (+ the randomization of [[z]])
        d_x, d_y = dev(ints_to_words([sk.enc_raw(r.x) for r in rows], 2 * nw)), dev(ints_to_words([sk.enc_raw(r.y) for r in rows], 2 * nw))
        d_r, d_rho_z = dev(ints_to_words([d.r for d in drs], nw)), dev(ints_to_words([d.rho_z for d in drs], nw))
        d_z, d_alpha, d_alpha_t, d_rsmall, d_rshift = empty(B, 2 * nw), empty(B, dtype=np.uint64), empty(B, dtype=np.uint64), \
            empty(B, dtype=np.uint64), empty(B, nw)
        assert lib.sc_initiator_step1(ctx, a_key, l, d_x, d_y, d_r, d_rho_z, 0, d_z, d_alpha, d_alpha_t, d_rsmall, d_rshift, B) == 0, lib.sc_last_error(ctx)
        assert words_to_ints(back(d_z, B, 2 * nw)) == [t["z_enc"] for t in want]
        assert back(d_alpha, B, dtype=np.uint64).tolist() == [r.r % (1 << l) for r in rows]
        assert back(d_alpha_t, B, dtype=np.uint64).tolist() == [(r.r - n) % (1 << l) for r in rows]
        assert back(d_rsmall, B, dtype=np.uint64).tolist() == [W.conditions(n, l, r).rsmall for r in rows]
        assert words_to_ints(back(d_rshift, B, nw)) == [r.r >> l for r in rows]
        # Bob: steps 2, 4a, 4b (+ l + 1 randomizations)
        d_rb = dev(planes([[d.r_d] + d.r_beta for d in drs], er))
        d_zp, d_beta, d_dbit, d_z1, d_z2, d_db = empty(B, nw), empty(B, dtype=np.uint64), empty(B, dtype=np.uint64), empty(B, nw), \
            empty(B, nw), empty(l + 1, B, nd)
        assert lib.sc_keyholder_step2_4b(ctx, b_key, b_dgk, l, d_z, d_rb, er, 0, d_zp, d_beta, d_dbit, d_z1, d_z2, d_db, B) == 0, lib.sc_last_error(ctx)
        zs = [t["z"] for t in want]
        assert words_to_ints(back(d_zp, B, nw)) == zs
        assert back(d_beta, B, dtype=np.uint64).tolist() == [z % (1 << l) for z in zs]
        assert back(d_dbit, B, dtype=np.uint64).tolist() == [W.conditions(n, l, r).d for r in rows]
        assert words_to_ints(back(d_z1, B, nw)) == [z >> l for z in zs]
        assert words_to_ints(back(d_z2, B, nw)) == [((z + n) >> l) if z < (n - 1) // 2 else z >> l for z in zs]
        got_db = back(d_db, l + 1, B, nd)
        assert words_to_ints(got_db[0]) == [t["d_sent"] for t in want]
        assert [words_to_ints(got_db[1:, b]) for b in range(B)] == [t["beta_enc"] for t in want]
        # Alice: steps 4c-4i (+ l + 1 randomizations, shuffle)
        rc_pre = [[None] * (l + 1) for _ in range(B)]      # the oracle randomizes output k = c_{perm[k]} after the shuffle
        for b, d in enumerate(drs):
            for k, src in enumerate(d.perm):
                rc_pre[b][src] = d.r_c[k]
        d_rhos, d_ra = dev(planes([d.rhos for d in drs], ew)), dev(planes(rc_pre, er))
        d_perm = dev(np.array([d.perm for d in drs], dtype=np.int64))
        d_da = dev(np.array([d.delta_a for d in drs], dtype=np.uint64))
        d_c = empty(l + 1, B, nd)
        beta_ptr = C.c_void_p(d_db.value + B * nd * 4)      # [beta_i] = planes 1.. of the same array
        assert lib.sc_initiator_step4(ctx, a_dgk, l, d_db, beta_ptr, d_alpha, d_alpha_t, d_rsmall, d_da, d_rhos, ew, d_perm, d_ra, er, 0, None,
                                      d_c, B) == 0, lib.sc_last_error(ctx)
        got_c = back(d_c, l + 1, B, nd)
        assert [words_to_ints(got_c[:, b]) for b in range(B)] == [t["c_enc"] for t in want]
        # Bob: steps 4j, 5 (+ 3 randomizations)
        d_rho3 = dev(np.concatenate([ints_to_words([getattr(d, f) for d in drs], nw) for f in ("rho_zeta1", "rho_zeta2", "rho_delta_b")]))
        d_delta_b, d_out3 = empty(B, dtype=np.uint64), empty(3, B, 2 * nw)
        assert lib.sc_keyholder_step4j_5(ctx, b_key, b_dgk, l, d_c, d_z1, d_z2, d_rho3, 0, d_delta_b, d_out3, B) == 0, lib.sc_last_error(ctx)
        assert back(d_delta_b, B, dtype=np.uint64).tolist() == [t["delta_b"] for t in want]
        out3 = back(d_out3, 3, B, 2 * nw)
        assert [words_to_ints(out3[k]) for k in range(3)] == [[t[f] for t in want] for f in ("zeta1", "zeta2", "delta_b_enc")]
        # Alice: steps 6, 7
        d_res = empty(B, 2 * nw)
        z1p, z2p, dbp = d_out3, C.c_void_p(d_out3.value + B * 2 * nw * 4), C.c_void_p(d_out3.value + 2 * B * 2 * nw * 4)
        assert lib.sc_initiator_step67(ctx, a_key, d_da, dbp, z1p, z2p, d_rsmall, d_rshift, 0, d_res, B) == 0, lib.sc_last_error(ctx)
        got = words_to_ints(back(d_res, B, 2 * nw))
        assert got == [t["result"] for t in want]
        assert [sk.dec_raw(v) for v in got] == [W.protocol_value(n, l, r) for r in rows]
    finally:
        for p in live:
            lib.sc_free(ctx, p)
        lib.sc_ctx_destroy(ctx)

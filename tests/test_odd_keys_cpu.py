"""The Paillier keys that do not fill their words (tests/golden/keys_odd.json, tests/_odd_keys.py), checked without a GPU: the keys
themselves, the conditions each one meets and that every condition has a key, the widths chosen for the family tests and the refusal
one bit past each fit limit, the family models on these keys, and one batch of whole comparisons on the stand-in engine with the
1025-bit key, whose primes differ in length and in words."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _dot_model as dmodel  # noqa: E402
import _instance_matrix as M  # noqa: E402
import _linear_model as LM  # noqa: E402
import _mult_model as mmodel  # noqa: E402
import _odd_keys as K  # noqa: E402
import _onehot_model as omodel  # noqa: E402
import _reduce_model as R  # noqa: E402
import _scan_model as S  # noqa: E402
import _select_model as smodel  # noqa: E402
from oracle import sc_oracle as o  # noqa: E402

KEYS = K.load()
SIZES = sorted(KEYS)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_declared_sizes_and_primes_only():
    import json

    raw = json.load(open(os.path.join(K.GOLDEN, "keys_odd.json")))
    assert tuple(SIZES) == K.SIZES
    assert all(set(v) == {"bits", "seed", "p", "q"} for v in raw.values())
    assert os.path.getsize(os.path.join(K.GOLDEN, "keys_odd.json")) < 8192


@pytest.mark.parametrize("bits", SIZES)
def test_key_has_its_length_and_prime_factors(bits):
    k = KEYS[bits]
    assert k.n.bit_length() == bits and k.p != k.q
    assert k.p.bit_length() == bits // 2 and k.q.bit_length() == bits - bits // 2
    assert o.is_probable_prime(k.p) and o.is_probable_prime(k.q)
    sk = k.oracle()
    assert sk.dec_raw(sk.randomize(sk.enc_raw(bits), 3)) == bits


@pytest.mark.parametrize("bits", SIZES[:2])
def test_key_regenerates_from_its_seed(bits):
    """The two smallest keys, always (a fraction of a second of prime search in plain Python); the larger ones are never regenerated
    here -- tests/golden/gen_keys_odd.py does that."""
    k = KEYS[bits]
    again = o.PaillierKey.generate(bits, random.Random(k.seed))
    assert (again.p, again.q) == (k.p, k.q)


# ---- conditions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CONDITIONS + K.EXTRA_CONDITIONS)
def test_every_condition_has_a_key(name):
    assert [b for b in SIZES if K.conditions(KEYS[b])[name]], name


def test_conditions_are_complete_and_boolean():
    for b in SIZES:
        c = K.conditions(KEYS[b])
        assert set(c) == set(K.CONDITIONS + K.EXTRA_CONDITIONS) and all(isinstance(v, bool) for v in c.values())


# N bits: (nw, N's configuration, N's pair route, N^2 in 2 nw words, N^2 by its bits alone, N^2's top word zero) -- the table the
# keys were chosen by; the helper computes, this pins
TABLE = {521: (17, (2, 18), (2, 18), (2, 27), (2, 27), True), 1025: (33, (2, 27), (4, 14), (4, 27), (4, 18), True),
         1040: (33, (2, 27), (4, 14), (4, 27), (4, 18), True), 1041: (33, (2, 27), (4, 14), (4, 27), (4, 27), False),
         1100: (35, (2, 27), (4, 14), (4, 27), (4, 27), True), 1540: (49, (4, 14), (4, 14), (8, 14), (4, 27), True)}


@pytest.mark.parametrize("bits", SIZES)
def test_configurations_match_the_table(bits):
    k = KEYS[bits]
    cfg, c = K.configs(k), K.conditions(k)
    assert (k.nw, cfg["n"], K.pair_config(k.n, k.nw), cfg["n2"], K.config(k.n2), c["n2_top_word_zero"]) == TABLE[bits]
    assert c["partial_top_word"]
    assert c["n2_moved_by_whole_words"] == (TABLE[bits][3] != TABLE[bits][4])


def test_the_padding_of_the_shorter_prime_joins_the_two_squares():
    """sc_paillier_key_create stores both primes in hw = nwords(max(bits(p), bits(q))) words and both squares in 2 hw words.  The
    whole-words rule (32 nwords <= 29 G L) then picks the configuration before the lengths can: no two squares in 2 hw words differ in
    configuration, for any hw the library holds.  So the 1025-bit key -- p of 512 bits in 16 words of its own, p^2 on (2,18) by its
    length; q of 513 bits in 17 words, q^2 on (2,27) -- runs both CRT halves on ONE instance, and p itself moves from (1,18) to (2,18)."""
    assert K.padded_squares_can_differ() == []
    for b in SIZES:
        cfg = K.configs(KEYS[b])
        assert cfg["p2"] == cfg["q2"] and cfg["p"] == cfg["q"]
    k = KEYS[1025]
    assert (K.config(k.p * k.p), K.config(k.q * k.q)) == ((2, 18), (2, 27))
    assert (K.config(k.p), K.configs(k)["p"], K.configs(k)["p2"]) == ((1, 18), (2, 18), (2, 27))


def test_instances_a_call_must_launch():
    ins = K.instances(KEYS[1025])
    assert ins["randomizer_public"] == {("pvm", 4, 14, 29, True, False, False), ("vm", 4, 27, 29, False, False, False)}
    assert ("pvm", 2, 18, 29, False, False, False) in ins["decrypt_crt"] and ("vm", 2, 27, 29, False, False, False) in ins["decrypt_crt"]
    assert ("vm", 8, 14, 29, False, False, False) in K.instances(KEYS[1540])["decrypt_no_crt"]
    for b in SIZES:
        ins = K.instances(KEYS[b])
        assert all(v <= ins["allowed"] for name, v in ins.items() if name != "allowed")
        assert all(inst in M.INSTANCES for inst in ins["allowed"]), "a predicted instance is not a compiled one"


def test_every_key_has_axis_instances():
    """The keys whose N^2 lands on a configuration without k_prod_axis / k_scan_axis / k_lin_axis: none (only (1,18) has none, and no
    N^2 of these sizes is that small).  The GPU tier asserts the documented refusal for a key listed here."""
    assert [b for b in SIZES if not K.has_axis_instance(KEYS[b])] == []
    assert (1, 18) not in R.INSTANCES


# ---- widths ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", SIZES)
def test_chosen_layouts_are_admitted_and_one_bit_more_is_refused(bits):
    from protocols.secure_comparison_amd.dotproduct import DotLayout
    from protocols.secure_comparison_amd.linear import check_fit
    from protocols.secure_comparison_amd.multiplication import MulLayout
    from protocols.secure_comparison_amd.selection import SelectLayout

    k = KEYS[bits]
    nbits = k.n.bit_length()
    ends, wide = [], []
    for cols in ((1, 4) if bits == SIZES[0] else (4,)):
        mw = K.mul_widths(k, cols)
        assert mw["layout"].end == nbits - 2 and mmodel.layout(mw["kappa"], mw["wx"], mw["wy"], nbits)[3] == nbits - 2
        kappa, wx, wy = mw["refused"]
        with pytest.raises(ValueError, match=f"column {cols - 1}"):
            MulLayout(kappa, wx, wy, True, nbits)
        with pytest.raises(ValueError):
            mmodel.layout(kappa, wx, list(wy), nbits)
        ends.append(mw["ends_at_nbits_minus_2"])
        wide.append(mw["three_word_field"])
    assert any(o_ % 32 for o_ in K.mul_widths(k)["unaligned_offsets"])
    for square in (False, True):
        dw = K.dot_widths(k, square)
        lay = dw["layout"]
        assert dmodel.layout(dw["kappa"], dw["wx"], dw["wy"], square, lay.k, nbits)[2:5] == (lay.pb, lay.g, lay.M)
        assert dw["ends_at_nbits_minus_2"] == (lay.g * lay.pb == nbits - 2)
        if dw["fit"]:
            DotLayout(*dw["fit"]["admitted"][:3], dw["fit"]["admitted"][3], True, False, nbits)
            with pytest.raises(ValueError):
                DotLayout(*dw["fit"]["refused"][:3], dw["fit"]["refused"][3], True, False, nbits)
            with pytest.raises(ValueError):
                kp, wx, wy, kk = dw["fit"]["refused"]
                dmodel.layout(kp, wx, wy, False, kk, nbits)
        ends.append(dw["ends_at_nbits_minus_2"])
        wide.append(dw["three_word_field"])
    ow = K.onehot_widths(k)
    assert omodel.layout(ow["kappa"], ow["index_bits"], ow["k"], ow["m"], nbits)[:3] == (ow["layout"].f, ow["g"], 2)
    for nf in (1, 2, 3, 4):
        sw = K.select_widths(k, nf)
        assert sw["layout"].end == nbits - 2 and smodel.layout(sw["kappa"], sw["widths"], nbits)[3] == nbits - 2
        with pytest.raises(ValueError):
            SelectLayout(sw["refused"][0], sw["kappa"], tuple(sw["refused"][1:]), nbits)
        with pytest.raises(ValueError):
            smodel.layout(sw["kappa"], sw["refused"], nbits)
        wide.append(sw["three_word_field"])
    assert any(ends) and any(wide)
    # the last admitted bit, nbits - 3, lies in the partial top word unless that word holds one or two bits only (1025 bits)
    assert ((nbits - 3) // 32 == k.nw - 1) == (nbits % 32 not in (1, 2))
    rows = [[3, -5, (1 << 64) - 1], [0, 0, 0], [-1, 1, 1]]
    xb = K.linear_x_bits(k, rows)
    check_fit(rows, xb, nbits)
    assert all(LM.fits(rows, xb, nbits)) and not all(LM.fits(rows, xb + 1, nbits))
    with pytest.raises(ValueError, match="row 0"):
        check_fit(rows, xb + 1, nbits)


def test_the_smallest_key_meets_the_dot_fit_rule():
    """Only below 2 * 255 + 2 * 63 + 2 bits can one pair reach the end of N: the 521-bit key records that limit, the others none."""
    assert [b for b in SIZES if K.dot_widths(KEYS[b])["fit"]] == [SIZES[0]]


# ---- the family models on these keys ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", SIZES)
def test_models_decrypt_to_the_plain_result(bits):
    k = KEYS[bits]
    sk, n = k.oracle(), k.n
    rng = random.Random(bits)
    mw = K.mul_widths(k)
    x = -(1 << (mw["wx"] - 1))
    ys = [(1 << (w - 1)) - 1 for w in mw["wy"]]
    assert mmodel.multiply(sk, x, ys, mw["wx"], mw["wy"], rng, True, mw["kappa"]) == [x * y % n for y in ys]
    dw = K.dot_widths(k)
    xs = [rng.getrandbits(dw["wx"]) - (1 << (dw["wx"] - 1)) for _ in range(dw["g"] + 1)]
    ys = [rng.getrandbits(dw["wy"]) - (1 << (dw["wy"] - 1)) for _ in range(dw["g"] + 1)]
    assert dmodel.dot(sk, xs, ys, dw["wx"], dw["wy"], rng, True, dw["kappa"]) == sum(a * b for a, b in zip(xs, ys)) % n
    dq = K.dot_widths(k, True)
    xs = [(1 << (dq["wx"] - 1)) - 1] * (dq["g"] + 1)
    assert dmodel.dot(sk, xs, None, dq["wx"], 0, rng, True, dq["kappa"]) == sum(a * a for a in xs) % n
    ow = K.onehot_widths(k)
    idx = [rng.getrandbits(ow["index_bits"]) for _ in range(ow["m"] if ow["g"] <= 11 else 3)]      # (two messages where g <= 11; the GPU tier runs every m)
    assert omodel.onehot(sk, idx, ow["k"], ow["index_bits"], rng, ow["kappa"]) == [[int(t == i % ow["k"]) for t in range(ow["k"])] for i in idx]
    sw = K.select_widths(k, 2)
    cols = [((1 << w) - 1, 0, w) for w in sw["widths"]]
    for sigma in (0, 1):
        assert smodel._select_plain(sk, sw["kappa"], rng, sigma, cols) == [a if sigma else b for a, b, _ in cols]
    assert smodel.argext(sk, [7, 3, 3], 16, rng) == (3, 1) and smodel.argext(sk, [7, 9, 9], 16, rng, want_max=True) == (9, 1)
    # the axis families: products of ciphertexts modulo N^2 decrypt to sums, running sums and signed linear maps
    vals = [[rng.randrange(n), n - 1, 0, 1][j % 4] for j in range(6)]                   # [K = 3][inner = 2]
    cs = [sk.randomize(sk.enc_raw(v), rng.randrange(1, n)) for v in vals]
    assert [sk.dec_raw(c) for c in R.prod_axis(sk.n2, cs, 1, 3, 2)] == [(vals[0] + vals[2] + vals[4]) % n, (vals[1] + vals[3] + vals[5]) % n]
    run = [sk.dec_raw(c) for c in S.scan_axis(sk.n2, cs, 1, 3, 2)]
    assert run == [vals[0], vals[1], (vals[0] + vals[2]) % n, (vals[1] + vals[3]) % n, (vals[0] + vals[2] + vals[4]) % n, (vals[1] + vals[3] + vals[5]) % n]
    W = [[3, -5, (1 << 64) - 1], [0, 0, 0], [-1, 1, 1]]
    members, nonneg = LM.split_signed(W)
    planes = [[cs[2 * kk + i] if not neg else sk.neg(cs[2 * kk + i]) for i in range(2)] for kk, neg in members]
    got = LM.lin_axis(sk.n2, [c for pl in planes for c in pl], 1, len(members), 2, nonneg)
    want = LM.signed_map(W, None, [[vals[0], vals[1]], [vals[2], vals[3]], [vals[4], vals[5]]])
    assert [sk.dec_raw(c) for c in got] == [v % n for row in want for v in row]


# ---- whole comparisons on the stand-in engine: unequal primes without a GPU ------------------------------------------------------------------
def test_stand_in_engine_compares_on_the_1025_bit_key(keys):
    import torch

    from _oracle_engine import OracleEngine
    from conftest import oracle_dgk
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.batch import BatchDraws, secure_comparison_batch

    k = KEYS[1025]
    c = K.conditions(k)
    assert c["unequal_prime_bits"] and c["unequal_prime_words"]
    osk, od = k.oracle(), oracle_dgk(keys, "dgk_tiny_l16")
    eng = OracleEngine()
    l, rbits, B = 16, 50, 6
    bob_p = Paillier(osk.n, osk.p, osk.q, engine=eng)
    bob_d = DGK(od.n, od.g, od.h, od.u, od.t, od.p, od.q, od.v_p, od.v_q, engine=eng, randomizer_bits=rbits)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    rng = random.Random(1025)
    xs = [0, (1 << l) - 1, 5, 5] + [rng.randrange(1 << l) for _ in range(B - 4)]
    ys = [(1 << l) - 1, 0, 5, 4] + [rng.randrange(1 << l) for _ in range(B - 4)]
    drs = [o.draw(rng, l, osk, od, rbits, shuffle=False) for _ in range(B)]
    x_enc = [osk.randomize(osk.enc_raw(x), rng.randrange(1, osk.n)) for x in xs]
    y_enc = [osk.randomize(osk.enc_raw(y), rng.randrange(1, osk.n)) for y in ys]
    expect = [o.compare(a, b, l, osk, od, d, True) for a, b, d in zip(x_enc, y_enc, drs)]
    nw, ew, er = alice_p.mod_n.nwords, (od.u.bit_length() + 31) // 32, (rbits + 31) // 32
    assert nw == k.nw
    up = eng.upload
    bm = lambda rows, w: torch.stack([up([rows[b][i] for b in range(B)], w) for i in range(l + 1)])  # noqa: E731
    draws = BatchDraws(r=up([d.r for d in drs], nw), delta_a=eng.upload_u64([d.delta_a for d in drs]),
                       rhos=bm([d.rhos for d in drs], ew), permutation=None, rho_z=up([d.rho_z for d in drs], nw),
                       r_bob_dgk=bm([[d.r_d] + d.r_beta for d in drs], er), r_alice_dgk=bm([d.r_c for d in drs], er),
                       rho_zeta_1=up([d.rho_zeta1 for d in drs], nw), rho_zeta_2=up([d.rho_zeta2 for d in drs], nw),
                       rho_delta_b=up([d.rho_delta_b for d in drs], nw))
    got = eng.download(secure_comparison_batch(up(x_enc, 2 * nw), up(y_enc, 2 * nw), l, alice_p, alice_d, bob_p, bob_d, draws))
    assert got == expect
    assert [osk.dec_raw(c) for c in got] == [int(x <= y) for x, y in zip(xs, ys)]

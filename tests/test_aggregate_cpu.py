"""CPU tier of the sums along an axis: the level plan of sc_modprod_axis against a member-by-member count, the fit rule of
the group-by sum, the segment rule of sum_rows_batch, the model itself, and the table of compiled k_prod_axis instances against the
launcher source."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _reduce_model as R  # noqa: E402

KS = (1, 2, 3, 4, 5, 31, 32, 33, 1025)


def _auto_chunk(outer, inner, resident):
    return lambda level, K: min(32, max(4, -(-(outer * K * inner) // resident)))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("forced", (0, 2, 3, 32))
def test_level_plan_matches_the_member_count(K, forced):
    from protocols.secure_comparison_amd.aggregate import reduce_plan

    for outer, inner, resident in ((1, 1, 256 * 8 * 16), (3, 7, 256 * 8 * 16), (2, 70000, 256 * 8 * 8), (1, 1 << 20, 304 * 8 * 4)):
        plan = reduce_plan(outer, K, inner, resident, forced)
        chunk_of = (lambda level, k: forced) if forced else _auto_chunk(outer, inner, resident)
        assert [nch for _, _, nch in plan] == R.chains_per_level(K, chunk_of)
        assert plan[0][0] == K and plan[-1][2] == 1
        for (k0, c0, n0), (k1, _, _) in zip(plan, plan[1:]):
            assert k1 == n0 and n0 > 1
        for k, c, nch in plan:
            assert 1 <= c <= min(32, k) and (c >= 2 or k == 1) and (nch - 1) * c < k <= nch * c
            if forced:
                assert c == min(forced, k)
            else:
                assert c == k or c >= 4


def test_level_plan_examples():
    from protocols.secure_comparison_amd.aggregate import reduce_plan

    res = 256 * 8 * 16
    assert reduce_plan(1, 1, 5, res) == [(1, 1, 1)]
    assert reduce_plan(1, 33, 1, res) == [(33, 4, 9), (9, 4, 3), (3, 3, 1)]
    assert reduce_plan(1, 1025, 1, res, 32) == [(1025, 32, 33), (33, 32, 2), (2, 2, 1)]
    assert reduce_plan(1, 8, 1, res, 2) == [(8, 2, 4), (4, 2, 2), (2, 2, 1)]
    assert reduce_plan(1, 16, 1 << 22, res) == [(16, 16, 1)]                     # a full chip: one chain per output
    for bad in (1, 33, -2):
        with pytest.raises(ValueError):
            reduce_plan(1, 4, 1, res, bad)
    with pytest.raises(ValueError):
        reduce_plan(1, 0, 1, res)


def test_model_product_along_the_axis():
    rng = random.Random(5)
    n = (rng.getrandbits(200) | 1) | (1 << 199)
    outer, K, inner = 2, 3, 5
    x = [rng.randrange(n) for _ in range(outer * K * inner)]
    got = R.prod_axis(n, x, outer, K, inner)
    assert got[1 * inner + 2] == x[(1 * K + 0) * inner + 2] * x[(1 * K + 1) * inner + 2] * x[(1 * K + 2) * inner + 2] % n
    assert R.prod_axis(n, x, outer * K, 1, inner) == x                           # K = 1: a copy
    assert R.prod_axis(n, x, 1, outer * K, inner) != R.prod_axis(n, x, 1, inner, outer * K)[:inner]   # the axes are not interchangeable


def test_segment_rule():
    from protocols.secure_comparison_amd.aggregate import check_segment

    assert check_segment(12, None) == 12 and check_segment(12, 1) == 1 and check_segment(12, 4) == 4 and check_segment(12, 12) == 12
    for bad in (0, -1, 5, 24):
        with pytest.raises(ValueError):
            check_segment(12, bad)


class _Pub:
    def __init__(self, n):
        self.n = n


class _Key:
    def __init__(self, bits):
        self.public_key = _Pub((1 << (bits - 1)) | 1)


def test_groupby_sum_fit_rule():
    from protocols.secure_comparison_amd.aggregate import groupby_sum_layout

    key = _Key(1024)
    lay = groupby_sum_layout(32, 100, False, 40, key)
    assert (lay.wx, lay.wy, lay.signed) == (32, (1,), False)
    assert groupby_sum_layout(32, 100, True, 40, key).wy == (2,)
    # bits + bits(B) (+ 1) must stay below bits(N) - 1 = 1023: B = 100 has 7 bits
    small = _Key(64)                                                             # the sum's own rule, apart from the multiplication's
    groupby_sum_layout(8, 100, False, 4, small)                                  # 8 + 7 = 15 < 63
    with pytest.raises(ValueError, match="does not fit"):
        groupby_sum_layout(56, 100, False, 4, small)                             # 56 + 7 = 63
    with pytest.raises(ValueError, match="does not fit"):
        groupby_sum_layout(55, 100, True, 4, small)                              # 55 + 7 + 1 = 63
    with pytest.raises(ValueError):
        groupby_sum_layout(0, 100, False, 40, key)


def test_every_compiled_instance_has_a_row():
    text = open(R.SOURCE).read()
    assert R.compiled_instances(text) == R.INSTANCES
    assert R.missing_rows(text) == []
    # the parse notices an instance the table does not know
    grown = text.replace("X(16, 18)", "X(16, 18) X(16, 27)")
    assert R.missing_rows(grown) == [(16, 27)]
    assert R.missing_rows(text, R.INSTANCES[:-1]) == [R.INSTANCES[-1]]
    with pytest.raises(ValueError):
        R.compiled_instances("no list here")


def test_public_names_are_exported():
    import protocols.secure_comparison_amd as pkg

    for name in ("sum_planes_batch", "sum_rows_batch", "secure_histogram_batch", "secure_majority_batch", "secure_groupby_count_batch",
                 "secure_groupby_sum_batch"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


# ---- the compositions on the stand-in engine, and their draw order --------------------------------------------------------------------
import torch  # noqa: E402

import _draw_replay as dr  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402

KEY = bytes((13 * i + 3) & 0xFF for i in range(32))


class StandIn(OracleEngine):
    """The CPU stand-in engine with the three families the compositions use as IDEAL functionalities -- the key holder's step decrypts
    the caller's operands (kept aside by the initiator's step; P itself is a placeholder of the right shape), computes the indicator or
    the product in plain integers and encrypts it under the randomizer it was handed; no blinding, no rotation -- and the sum along
    an axis as a plain product.  What runs for real is aggregate.py: its geometry, its reshapes, its rules and its draws.  Every
    generator call is recorded."""

    def __init__(self):
        super().__init__()
        self.calls, self.kept = [], None
        self.rng_seed(KEY)

    def rng_bits(self, bits, count):
        self.calls.append(("bits", bits, count, False))
        return super().rng_bits(bits, count)

    def rng_below(self, n, count, nonzero=False):
        self.calls.append(("below", n, count, bool(nonzero)))
        return super().rng_below(n, count, nonzero)

    def rng_coins(self, count):
        self.calls.append(("coins", None, count, False))
        return super().rng_coins(count)

    def rng_permutations(self, k, count):
        self.calls.append(("perms", k, count, False))
        return super().rng_permutations(k, count)

    def _fresh(self, key, plain, rho):
        n, n2 = key.mod_n.n, key.mod_n2.n
        return self.upload([(1 + (v % n) * n) * pow(r, n, n2) % n2 for v, r in zip(plain, self._ints(rho.reshape(-1, rho.shape[-1])))],
                           key.mod_n2.nwords)

    def initiator_onehot_pack(self, key, kappa, ib, k, m, M, planes, r, rho_p):
        assert tuple(r.shape[:2]) == tuple(planes.shape[:2]) and tuple(rho_p.shape[:2]) == (M, planes.shape[1])
        self.kept = planes
        return torch.zeros((M, planes.shape[1], key.mod_n2.nwords), dtype=torch.int32), torch.zeros(planes.shape[:2], dtype=torch.int32)

    def keyholder_onehot(self, key, kappa, ib, k, m, M, P, rho_e):
        B = P.shape[1]
        idx = [key.sk.dec_raw(c) for c in self._ints(self.kept.reshape(m * B, -1))]
        plain = [1 if idx[q * B + b] % k == t else 0 for q in range(m) for t in range(k) for b in range(B)]
        return self._fresh(key, plain, rho_e).reshape(m, k, B, -1)

    def initiator_onehot_finish(self, key, kappa, ib, k, m, E, rot, out=None):
        return E

    def initiator_mul_pack(self, key, kappa, wx, wy, signed, x_enc, cols, r_a, r_b, rho_p, ew):
        self.kept = (x_enc, cols)
        return torch.zeros_like(x_enc), None, None

    def keyholder_mul(self, key, kappa, wx, wy, P, rho_products):
        x_enc, cols = self.kept
        n = key.mod_n.n
        xs = [key.sk.dec_raw(c) for c in self._ints(x_enc)]
        plain = [x * key.sk.dec_raw(c) % n for j in range(cols.shape[0]) for x, c in zip(xs, self._ints(cols[j]))]
        return self._fresh(key, plain, rho_products).reshape(cols.shape[0], len(xs), -1)

    def initiator_mul_finish(self, key, kappa, wx, wy, x_enc, cols, products, e, rab, base, coef):
        return products

    def paillier_sum_axis(self, key, c, outer, K, inner, out=None):
        flat = self._ints(c.reshape(-1, c.shape[-1]))
        return self.upload(R.prod_axis(key.mod_n2.n, flat, outer, K, inner), key.mod_n2.nwords)


@pytest.fixture(scope="module")
def sk():
    from oracle import sc_oracle as o

    return o.PaillierKey.generate(512, random.Random(20263))


def _players(sk):
    from protocols.secure_comparison_amd import Paillier

    eng = StandIn()
    bob = Paillier(sk.n, sk.p, sk.q, engine=eng)
    return eng, Paillier(sk.n, engine=eng), bob


def _encrypt(eng, sk, rng, values):
    return eng.upload([(1 + (v % sk.n) * sk.n) * pow(rng.randrange(1, sk.n), sk.n, sk.n2) % sk.n2 for v in values], 2 * ((sk.n.bit_length() + 31) // 32))


def _decrypt(eng, sk, t, signed=False):
    vals = [sk.dec_raw(c) for c in eng.download(t.reshape(-1, t.shape[-1]))]
    return [v - sk.n if signed and v > sk.n // 2 else v for v in vals]


@pytest.mark.parametrize("k,m", [(1, 1), (2, 3), (3, 5), (7, 1), (7, 3)])
def test_histogram_composition_and_draws(sk, k, m):
    """[k][B] counts against plain Python; the draws are the one-hot's alone: r, rho_p, then Bob's rho_e."""
    from protocols.secure_comparison_amd import OnehotLayout, secure_histogram_batch
    from protocols.secure_comparison_amd.lookup import default_index_bits

    eng, ap, bp = _players(sk)
    rng, B, ib = random.Random(f"h{k}{m}"), 6, default_index_bits(k)
    idx = [[rng.getrandbits(ib) for _ in range(B)] for _ in range(m)]
    enc = _encrypt(eng, sk, rng, [v for row in idx for v in row]).reshape(m, B, -1)
    out = secure_histogram_batch(enc, k, ap, bp)
    assert tuple(out.shape)[:2] == (k, B)
    assert _decrypt(eng, sk, out) == [sum(1 for q in range(m) if idx[q][b] % k == t) for t in range(k) for b in range(B)]
    lay = OnehotLayout(40, ib, k, m, sk.n.bit_length())
    rp = dr.Replay(KEY)
    rp.bits(ib + 40, m * B, [0]); rp.below(sk.n, lay.M * B, True, [0]); rp.below(sk.n, m * k * B, True, [0])
    assert eng.calls == rp.log and eng._rng_call == rp.call == 3


def test_groupby_compositions_and_draws(sk):
    """Group-by count and sum (signed and unsigned) against plain Python; the sum draws the one-hot's three calls, then the
    multiplication's over k B rows: r_a, the column's r_b, rho_p, then Bob's rho_products."""
    from protocols.secure_comparison_amd import secure_groupby_count_batch, secure_groupby_sum_batch

    rng, B, k, bits, n = random.Random("g"), 10, 3, 12, sk.n
    idx = [rng.randrange(k) for _ in range(B)]
    eng, ap, bp = _players(sk)
    out = secure_groupby_count_batch(_encrypt(eng, sk, rng, idx), k, ap, bp)
    assert tuple(out.shape)[0] == k and _decrypt(eng, sk, out) == [idx.count(t) for t in range(k)]
    assert [c[0] for c in eng.calls] == ["bits", "below", "below"]
    for signed in (False, True):
        eng, ap, bp = _players(sk)
        vals = [rng.randint(-(1 << 11), (1 << 11) - 1) if signed else rng.getrandbits(bits) for _ in range(B)]
        out = secure_groupby_sum_batch(_encrypt(eng, sk, rng, vals), _encrypt(eng, sk, rng, idx), k, bits, ap, bp, signed=signed)
        assert _decrypt(eng, sk, out, signed) == [sum(v for v, i in zip(vals, idx) if i == t) for t in range(k)]
        rp = dr.Replay(KEY)
        rp.bits(2 + 40, B, [0]); rp.below(n, B, True, [0]); rp.below(n, k * B, True, [0])              # the one-hot: ib = 2, m = M = 1
        dr.multiplication(rp, [0], k * B, 40, bits, (2 if signed else 1,), n)                          # then the multiplication
        assert eng.calls == rp.log and eng._rng_call == rp.call == 7
    with pytest.raises(ValueError, match="does not fit"):
        secure_groupby_sum_batch(_encrypt(eng, sk, rng, vals), _encrypt(eng, sk, rng, idx), k, 507, ap, bp)   # 507 + bits(10) = 511
    assert eng._rng_call == 7                                                                          # refused before any draw


def test_majority_composition_and_draw_order(sk, monkeypatch):
    """The majority is the histogram handed to secure_argmax_batch as [B][k] counts with l = bits(m); the one-hot's draws come before
    the argmax's first.  (The argmax itself runs on the GPU tier; here it is replaced by a plain decrypt-and-encrypt that records
    where the generator stood.)"""
    from protocols.secure_comparison_amd import aggregate, selection

    eng, ap, bp = _players(sk)
    rng, B, k, m = random.Random("v"), 8, 4, 5
    labels = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    for q in range(m):
        labels[q][0] = q % 2                                        # labels 0 and 1 three and two times
        labels[q][1] = (q % 2) + 2 if q < 4 else 0                  # 2 and 3 twice each, 0 once: a tie for the lowest of them
    seen = {}

    def argmax(v_enc, l, a, ad, b, bd, kappa=40):
        seen.update(l=l, shape=tuple(v_enc.shape[:2]), call=eng._rng_call)
        rows = [_decrypt(eng, sk, v_enc[i]) for i in range(v_enc.shape[0])]
        return (eng.upload([1 + max(r) * sk.n for r in rows], ap.mod_n2.nwords), eng.upload([1 + r.index(max(r)) * sk.n for r in rows], ap.mod_n2.nwords))

    monkeypatch.setattr(selection, "secure_argmax_batch", argmax)
    label, top = aggregate.secure_majority_batch(_encrypt(eng, sk, rng, [v for r in labels for v in r]).reshape(m, B, -1), k, ap, None, bp, None)
    cols = [[sum(1 for q in range(m) if labels[q][b] == t) for t in range(k)] for b in range(B)]
    assert seen == {"l": 3, "shape": (B, k), "call": 3}
    assert _decrypt(eng, sk, top) == [max(c) for c in cols] and _decrypt(eng, sk, label) == [c.index(max(c)) for c in cols]
    assert _decrypt(eng, sk, label)[:2] == [0, 2]

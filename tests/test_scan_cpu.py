"""CPU tier of the running sums along an axis: the launch plan of sc_modscan_axis against a member-by-member count, the
table of compiled k_scan_axis instances against the launcher source, the exclusive shift and the segment rule, the cumulative
distribution and the quantile on the stand-in engine against plain Python for every rank with their generator calls held to the replay's
order (the one-hot's, then the comparison's), the refusals, and the two new symbols."""
import ctypes
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _draw_replay as dr  # noqa: E402
import _reduce_model as R  # noqa: E402
import _scan_model as S  # noqa: E402
from test_aggregate_cpu import KEY, StandIn  # noqa: E402

GEOMETRIES = ((1, 1, 256 * 8 * 16), (3, 7, 256 * 8 * 16), (2, 70000, 256 * 8 * 8), (1, 1 << 20, 304 * 8 * 4), (4, 1023, 256 * 8 * 16),
              (4, 1024, 256 * 8 * 16), (1, 1, 1), (2, 1, 3))


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", (0, 2, 3, 32))
def test_plan_matches_the_member_count(forced):
    from protocols.secure_comparison_amd.aggregate import scan_plan

    for K in list(range(1, 71)) + [1025]:
        for outer, inner, resident in GEOMETRIES:
            plan = scan_plan(outer, K, inner, resident, forced)
            assert plan == S.launches(outer, K, inner, resident, forced), (K, outer, inner, resident)
            scans, totals = [p for p in plan if p[0] == "scan"], [p for p in plan if p[0] == "totals"]
            assert len(scans) == len(totals) + 1 and plan[:len(totals)] == totals          # totals on the way down, scans on the way up
            assert plan[-1][1] == K and scans[0][2] == scans[0][1]                         # the deepest scan is direct
            if forced:
                assert all(c == forced and k > forced for _, k, c, _ in totals) and scans[0][1] <= forced
            elif outer * inner >= resident:
                assert plan == [("scan", K, K, outer * inner)]
            for (_, k, c, chains), (_, k2, c2, chains2) in zip(totals, scans[:0:-1]):
                assert (k, c) == (k2, c2) and chains2 - chains == outer * inner              # one total per chunk but the last


def test_plan_examples_on_both_sides_of_the_boundary():
    from protocols.secure_comparison_amd.aggregate import scan_plan

    res = 256 * 8 * 16
    assert scan_plan(1, 1, 5, res) == [("scan", 1, 1, 5)]
    assert scan_plan(1, 4, 1, res) == [("scan", 4, 4, 1)]                                   # the minimum chunk
    assert scan_plan(1, 5, 1, res) == [("totals", 5, 4, 1), ("scan", 1, 1, 1), ("scan", 5, 4, 2)]
    assert scan_plan(1, 1000, res - 1, res) == [("totals", 1000, 32, 31 * (res - 1)), ("scan", 31, 31, res - 1), ("scan", 1000, 32, 32 * (res - 1))]
    assert scan_plan(1, 1000, res, res) == [("scan", 1000, 1000, res)]                      # the chains fill the slots: direct
    assert scan_plan(2, 1000, res // 2, res) == [("scan", 1000, 1000, res)]
    assert scan_plan(1, 1000, res, res, 32)[0] == ("totals", 1000, 32, 31 * res)            # a forced chunk blocks all the same
    assert scan_plan(1, 33, 1, res, 32) == [("totals", 33, 32, 1), ("scan", 1, 1, 1), ("scan", 33, 32, 2)]
    assert scan_plan(1, 1025, 3, res, 32) == [("totals", 1025, 32, 96), ("scan", 32, 32, 3), ("scan", 1025, 32, 99)]
    assert scan_plan(1, 9, 1, res, 2) == [("totals", 9, 2, 4), ("totals", 4, 2, 1), ("scan", 1, 1, 1), ("scan", 4, 2, 2), ("scan", 9, 2, 5)]
    assert S.products(scan_plan(1, 9, 1, res, 2)) == 4 + 1 + 2 * (1 + 4 + 9)
    assert S.products(scan_plan(1, 1000, res, res)) == 2 * 1000 * res
    for bad in (1, 33, -2):
        with pytest.raises(ValueError):
            scan_plan(1, 4, 1, res, bad)
    with pytest.raises(ValueError):
        scan_plan(1, 0, 1, res)


def test_model_scan_along_the_axis():
    rng = random.Random(6)
    n = (rng.getrandbits(200) | 1) | (1 << 199)
    outer, K, inner = 2, 3, 5
    x = [rng.randrange(1, n) for _ in range(outer * K * inner)]
    got = S.scan_axis(n, x, outer, K, inner)
    at = lambda o, j, i: (o * K + j) * inner + i  # noqa: E731
    assert got[at(1, 0, 2)] == x[at(1, 0, 2)] and got[at(1, 2, 2)] == x[at(1, 0, 2)] * x[at(1, 1, 2)] * x[at(1, 2, 2)] % n
    assert [got[at(o, K - 1, i)] for o in range(outer) for i in range(inner)] == R.prod_axis(n, x, outer, K, inner)
    assert S.scan_axis(n, x, outer * K, 1, inner) == x                                      # K = 1: a copy
    assert S.scan_axis(n, x, 1, outer * K, inner) != S.scan_axis(n, x, 1, inner, outer * K)
    x[at(0, 1, 3)] = 0                                                                      # a zero blanks the rest of its scan only
    got = S.scan_axis(n, x, outer, K, inner)
    assert [got[at(0, j, 3)] for j in range(K)] == [x[at(0, 0, 3)], 0, 0] and all(got[at(o, j, i)] for o in range(outer) for j in range(K)
                                                                                   for i in range(inner) if (o, i) != (0, 3))


def test_every_compiled_instance_has_a_row():
    text = open(S.SOURCE).read()
    assert S.compiled_instances(text) == S.INSTANCES == R.INSTANCES                         # the ten instances of k_prod_axis
    assert S.missing_rows(text) == []
    grown = text.replace("X(16, 18)", "X(16, 18) X(16, 27)")
    assert S.missing_rows(grown) == [(16, 27)]
    assert S.missing_rows(text, S.INSTANCES[:-1]) == [S.INSTANCES[-1]]
    with pytest.raises(ValueError):
        S.compiled_instances("no list here")
    from protocols.secure_comparison_amd.build import UNITS

    assert ("sc_launch_scan", "sc_launch_scan.hip", []) in UNITS and len(UNITS) == 13
    assert ("sc_launch_reduce", "sc_launch_reduce.hip", []) in UNITS
    assert S.units_share_the_list()                                                         # one list, in the header both units include


def test_symbols_are_exported_and_bound():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.build import build_lib
    from protocols.secure_comparison_amd.engine import Engine

    lib = ctypes.CDLL(build_lib(verbose=False))
    for name in ("sc_modscan_axis", "sc_paillier_cumsum_axis"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(_lib.load(), name).argtypes is not None and len(getattr(_lib.load(), name).argtypes) == 7
    assert callable(Engine.modscan_axis) and callable(Engine.paillier_cumsum_axis)
    assert _lib.ABI_VERSION == 5
    import protocols.secure_comparison_amd as pkg

    for name in ("cumsum_planes_batch", "cumsum_rows_batch", "secure_cdf_batch", "secure_quantile_batch", "secure_histogram_median_batch"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for cls, names in ((pkg.Initiator, ("perform_secure_cdf_batch", "perform_secure_quantile_batch")),
                       (pkg.KeyHolder, ("perform_secure_cdf_batch", "perform_secure_quantile_batch"))):
        assert all(callable(getattr(cls, n)) for n in names)


# ---- the Python layer on the stand-in engine ------------------------------------------------------------------------------------------
class ScanStandIn(StandIn):
    """The stand-in engine of the sums with the running sum as the plain model; the geometry of every scan call is recorded."""

    def __init__(self):
        super().__init__()
        self.scans = []

    def paillier_cumsum_axis(self, key, c, outer, K, inner, out=None):
        self.scans.append((outer, K, inner))
        flat = self._ints(c.reshape(-1, c.shape[-1]))
        return self.upload(S.scan_axis(key.mod_n2.n, flat, outer, K, inner), key.mod_n2.nwords)


@pytest.fixture(scope="module")
def gold(keys):
    return oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_tiny_l16")


def _players(gold):
    from protocols.secure_comparison_amd import DGK, Paillier

    sk, od = gold
    eng = ScanStandIn()
    bp = Paillier(sk.n, sk.p, sk.q, engine=eng)
    bd = DGK(od.n, od.g, od.h, od.u, od.t, od.p, od.q, od.v_p, od.v_q, full_decryption=True, engine=eng, randomizer_bits=50)
    return eng, bp.public_copy(), bd.public_copy(), bp, bd


def _encrypt(eng, sk, rng, values):
    return eng.upload([(1 + (v % sk.n) * sk.n) * pow(rng.randrange(1, sk.n), sk.n, sk.n2) % sk.n2 for v in values], 2 * ((sk.n.bit_length() + 31) // 32))


def _decrypt(eng, sk, t):
    return [sk.dec_raw(c) for c in eng.download(t.reshape(-1, t.shape[-1]))]


def test_exclusive_shift_and_segment_rule(gold):
    from protocols.secure_comparison_amd.aggregate import cumsum_planes_batch, cumsum_rows_batch

    sk = gold[0]
    eng, ap, _, bp, _ = _players(gold)
    rng, k, B = random.Random("shift"), 3, 10
    plain = [[rng.randrange(1000) for _ in range(B)] for _ in range(k)]
    x = _encrypt(eng, sk, rng, [v for row in plain for v in row]).reshape(k, B, -1)
    flat = eng.download(x.reshape(k * B, -1))
    inc = cumsum_planes_batch(x, ap)
    assert tuple(inc.shape) == tuple(x.shape) and eng.scans[-1] == (1, k, B)
    assert eng.download(inc.reshape(k * B, -1)) == S.scan_axis(sk.n2, flat, 1, k, B)
    exc = eng.download(cumsum_planes_batch(x, ap, exclusive=True).reshape(k * B, -1))
    assert exc == [1] * B + S.scan_axis(sk.n2, flat, 1, k, B)[:-B]
    for seg in (None, 1, 2, 5, 10):
        s = B if seg is None else seg
        got = cumsum_rows_batch(x, ap, segment=seg)
        assert tuple(got.shape) == tuple(x.shape) and eng.scans[-1] == (k * (B // s), s, 1)
        want = S.scan_axis(sk.n2, flat, k * (B // s), s, 1)
        assert eng.download(got.reshape(k * B, -1)) == want
        exc = eng.download(cumsum_rows_batch(x, ap, segment=seg, exclusive=True).reshape(k * B, -1))
        assert exc == [1 if t % s == 0 else want[t - 1] for t in range(k * B)]
        assert _decrypt(eng, sk, eng.upload(exc, x.shape[-1])) == [sum(plain[t // B][(t % B) // s * s:t % B]) for t in range(k * B)]
    for bad in (0, 3, 20):
        with pytest.raises(ValueError, match="divisor"):
            cumsum_rows_batch(x, ap, segment=bad)
    with pytest.raises(ValueError):
        cumsum_planes_batch(x[0], ap)
    rho = eng.upload([rng.randrange(1, sk.n) for _ in range(k * B)], ap.mod_n.nwords).reshape(k, B, -1)
    fresh = eng.download(cumsum_planes_batch(x, ap, exclusive=True, rho=rho).reshape(k * B, -1))
    assert fresh == [c * pow(r, sk.n, sk.n2) % sk.n2 for c, r in zip([1] * B + S.scan_axis(sk.n2, flat, 1, k, B)[:-B], eng.download(rho.reshape(k * B, -1)))]


def _bins(idx, k, b):
    return sorted(row[b] % k for row in idx)


@pytest.mark.parametrize("k,m", [(1, 2), (2, 3), (3, 4), (7, 1), (5, 3)])
def test_cdf_and_quantile_compositions_and_draws(gold, k, m):
    """[k][B] cumulative counts and the bin of every rank against plain Python; the generator calls are the one-hot's three, then -- for
    the quantile, unless k = 1 -- the comparison's eight over (k - 1) B rows at l = bits(m), Alice's before Bob's."""
    from protocols.secure_comparison_amd import OnehotLayout, secure_cdf_batch, secure_histogram_median_batch, secure_quantile_batch
    from protocols.secure_comparison_amd.aggregate import count_bits
    from protocols.secure_comparison_amd.lookup import default_index_bits

    sk, od = gold
    rng, B, ib = random.Random(f"q{k}{m}"), 2, default_index_bits(k)
    idx = [[rng.getrandbits(ib) for _ in range(B)] for _ in range(m)]
    for q in range(m):
        idx[q][0], idx[q][1] = k - 1, 0                                # all in the last bin, all in the first
    eng, ap, ad, bp, bd = _players(gold)
    enc = _encrypt(eng, sk, rng, [v for row in idx for v in row]).reshape(m, B, -1)
    lay = OnehotLayout(40, ib, k, m, sk.n.bit_length())

    def replay(with_comparison):
        rp = dr.Replay(KEY)
        rp.bits(ib + 40, m * B, [0]); rp.below(sk.n, lay.M * B, True, [0]); rp.below(sk.n, m * k * B, True, [0])
        if with_comparison:
            dr.comparison(rp, [0], (k - 1) * B, count_bits(m), sk.n, od.u, 50, alice=True, bob=False)
            dr.comparison(rp, [0], (k - 1) * B, count_bits(m), sk.n, od.u, 50, alice=False, bob=True)
        return rp

    cdf = secure_cdf_batch(enc, k, ap, bp)
    assert tuple(cdf.shape)[:2] == (k, B) and eng.scans == [(1, k, B)]
    assert _decrypt(eng, sk, cdf) == [sum(1 for q in range(m) if idx[q][b] % k <= t) for t in range(k) for b in range(B)]
    assert eng.calls == replay(False).log and eng._rng_call == 3
    for kth in range(m):
        eng, ap, ad, bp, bd = _players(gold)
        enc = _encrypt(eng, sk, rng, [v for row in idx for v in row]).reshape(m, B, -1)
        got = secure_quantile_batch(enc, k, kth, ap, ad, bp, bd)
        assert tuple(got.shape) == (B, enc.shape[-1])
        assert _decrypt(eng, sk, got) == [_bins(idx, k, b)[kth] for b in range(B)], kth
        rp = replay(k > 1)
        assert eng.calls == rp.log and eng._rng_call == rp.call == (11 if k > 1 else 3)
    ranks = [b % m for b in range(B)]                                  # encrypted ranks, one per row
    got = secure_quantile_batch(enc, k, _encrypt(eng, sk, rng, ranks), ap, ad, bp, bd)
    assert _decrypt(eng, sk, got) == [_bins(idx, k, b)[ranks[b]] for b in range(B)]
    got = secure_histogram_median_batch(enc, k, ap, ad, bp, bd)
    assert _decrypt(eng, sk, got) == [_bins(idx, k, b)[(m - 1) // 2] for b in range(B)]
    if k == 1:
        assert eng.download(got) == [1] * B                            # [[0]], unrandomized


def test_quantile_refuses_before_any_draw(gold):
    from protocols.secure_comparison_amd.aggregate import check_rank, secure_quantile_batch

    sk = gold[0]
    eng, ap, ad, bp, bd = _players(gold)
    rng, m, B = random.Random("refuse"), 3, 2
    enc = _encrypt(eng, sk, rng, [0] * (m * B)).reshape(m, B, -1)
    for bad in (-1, m, 10 ** 9):
        with pytest.raises(ValueError, match="expected 0 .. 2"):
            secure_quantile_batch(enc, 4, bad, ap, ad, bp, bd)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError, match="integer"):
            secure_quantile_batch(enc, 4, bad, ap, ad, bp, bd)
    with pytest.raises(ValueError, match="encrypted ranks"):
        secure_quantile_batch(enc, 4, enc[0][:1], ap, ad, bp, bd)       # ranks for one row, two rows of indices
    with pytest.raises(ValueError, match="255"):
        check_rank(0, 1 << 255, B, enc.shape[-1])                      # bits(m) = 256
    assert check_rank(0, (1 << 255) - 1, B, enc.shape[-1]) == 0
    assert eng.calls == [] and eng.scans == []

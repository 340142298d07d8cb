"""Secure sort without a GPU: the package's Batcher network sorts every 0/1 row and random rows, has Batcher's layer and comparator
counts and disjoint layers; both players derive the same schedule; the compare-exchange model (shared inversion) returns min and
max with payload and index columns following their key; secure_sort_batch refuses bad arguments before any launch; and the library
exports sc_select_finish_cx."""
import ctypes
import itertools
import os
import random
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _select_model as sm  # noqa: E402
import _sort_model as model  # noqa: E402


def _flat(layers):
    return [c for layer in layers for c in layer]


# ---- the network ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 17))
def test_network_sorts_every_zero_one_row(k):
    from protocols.secure_comparison_amd.sorting import batcher_network

    layers = batcher_network(k)
    for bits in itertools.product((0, 1), repeat=k):
        (out,) = model.apply(layers, [[(b,) for b in bits]])
        assert [t[0] for t in out] == sorted(bits)


def test_network_sorts_random_rows_up_to_64():
    from protocols.secure_comparison_amd.sorting import batcher_network

    rng = random.Random(1)
    for k in range(1, 65):
        layers = batcher_network(k)
        rows = [[(rng.randrange(8 if t % 2 else 1 << 20),) for _ in range(k)] for t in range(6)]
        for row, out in zip(rows, model.apply(layers, rows)):
            assert [t[0] for t in out] == sorted(t[0] for t in row)
        for row, out in zip(rows, model.apply(layers, rows, descending=True)):
            assert [t[0] for t in out] == sorted((t[0] for t in row), reverse=True)


def test_network_counts_and_disjoint_layers():
    from protocols.secure_comparison_amd.sorting import MAX_K, batcher_network

    counts = {k: (len(batcher_network(k)), len(_flat(batcher_network(k)))) for k in (2, 8, 16, 32, 17)}
    assert counts == {2: (1, 1), 8: (6, 19), 16: (10, 63), 32: (15, 191), 17: (15, 85)}
    for m in range(0, 11):
        layers = batcher_network(1 << m)
        assert (len(layers), len(_flat(layers))) == (model.batcher_counts(m) if m else (0, 0))
    for k in list(range(1, 70)) + [100, 255, 256, 257, 1000, MAX_K]:
        layers = batcher_network(k)
        assert all(layers), k                                    # no empty layer
        for layer in layers:
            seen = [x for c in layer for x in c]
            assert len(seen) == len(set(seen)), (k, layer)       # no index twice in a layer
            assert all(0 <= i < j < k for i, j in layer)
        assert sorted(_flat(layers)) == sorted(model.comparators(k)), k    # the same comparators as the recursive construction
    for bad in (0, MAX_K + 1):
        with pytest.raises(ValueError):
            batcher_network(bad)


@pytest.mark.parametrize("k,B,max_rows", [(2, 1, 65536), (5, 3, 2), (8, 100, 7), (17, 64, 65536), (17, 64, 100), (32, 5, 1)])
def test_both_players_derive_the_same_schedule(k, B, max_rows):
    from protocols.secure_comparison_amd.sorting import _topk_steps, batcher_network, schedule_counts, sort_schedule

    nf = 2
    buf = torch.arange(nf * B * k, dtype=torch.int32).reshape(nf, B * k, 1)
    steps = list(_topk_steps(buf, B, k, k, False, max_rows, False))       # what the initiator runs: the m = k network
    counts = schedule_counts(k, B, max_rows)                              # what the key holder expects
    assert [f.shape[1] for f, _, _, _ in steps] == counts
    assert all(0 < c <= max_rows for c in counts)
    assert sum(counts) == B * len(_flat(batcher_network(k)))
    if B * max(len(layer) for layer in batcher_network(k)) > max_rows:
        assert len(counts) > len(batcher_network(k))                      # a layer is cut
    for layer, cuts in sort_schedule(k, B, max_rows):                     # every layer's rows, each once, disjoint
        touched = []
        for f, g, lo, hi in steps[:len(cuts)]:
            assert torch.equal(lo[1] - lo[0], torch.full_like(lo[0], B * k))   # column j's rows are column 0's plus j B k
            assert torch.equal(f[:, :, 0].long(), lo)                     # F is read from the row lo goes to
            assert torch.equal(g[:, :, 0].long(), hi)
            touched += lo[0].tolist() + hi[0].tolist()
        steps = steps[len(cuts):]
        assert len(touched) == len(set(touched)) == 2 * B * len(layer)
        assert sorted(touched) == sorted(b * k + x for b in range(B) for c in layer for x in c)


def test_descending_swaps_the_operands():
    from protocols.secure_comparison_amd.sorting import _topk_steps

    buf = torch.arange(2 * 3, dtype=torch.int32).reshape(1, 6, 1)            # B = 2 rows of k = 3
    asc = [(lo.tolist(), hi.tolist()) for _, _, lo, hi in _topk_steps(buf, 2, 3, 3, False, 100, False)]
    desc = [(lo.tolist(), hi.tolist()) for _, _, lo, hi in _topk_steps(buf, 2, 3, 3, False, 100, True)]
    assert desc == [(hi, lo) for lo, hi in asc]


def test_sort_steps_equal_the_rows_of_the_replay_model():
    """A sort's sub-batches against rows written out in plain Python from tests/_draw_replay.py's sort_layers and cuts, a model made
    from the network's definition: comparison t = c B + b of a layer compares positions i and j of row b, F at i ascending and at j
    descending; column c's row is c B k further on; every output is live, so no row is the one past the buffer."""
    import _draw_replay as dr
    from protocols.secure_comparison_amd.sorting import _topk_steps, schedule_counts

    for k, B, nf in itertools.product((1, 2, 3, 5, 8, 9, 17), (1, 3), (1, 3)):
        buf = torch.arange(nf * B * k * 2, dtype=torch.int32).reshape(nf, B * k, 2)
        layers = dr.sort_layers(k)
        for max_rows, descending in itertools.product((1, 4, 7, 65536), (False, True)):
            want_lo, want_hi = [], []
            for layer in layers:
                pairs = [(b * k + (j if descending else i), b * k + (i if descending else j)) for i, j in layer for b in range(B)]
                for a, z in dr.cuts(B * len(layer), max_rows):
                    want_lo.append([[c * B * k + f for f, _ in pairs[a:z]] for c in range(nf)])
                    want_hi.append([[c * B * k + g for _, g in pairs[a:z]] for c in range(nf)])
            steps = list(_topk_steps(buf, B, k, k, False, max_rows, descending))
            assert [lo.tolist() for _, _, lo, _ in steps] == want_lo and [hi.tolist() for _, _, _, hi in steps] == want_hi
            assert schedule_counts(k, B, max_rows) == [len(rows[0]) for rows in want_lo]
            flat = buf.reshape(-1, 2)
            for f, g, lo, hi in steps:
                assert lo.dtype == hi.dtype == torch.int64 and lo.is_contiguous() and hi.is_contiguous()
                assert max(lo.max().item(), hi.max().item()) < nf * B * k
                assert torch.equal(f, flat[lo]) and torch.equal(g, flat[hi])
            if k == 1:
                assert steps == [] and schedule_counts(k, B, max_rows) == []


# ---- the compare-exchange model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 32, 255])
def test_model_compare_exchange_min_max(keys, l):
    from protocols.secure_comparison_amd.selection import SelectLayout, index_bits

    sk = oracle_paillier(keys, 1024)
    rng = random.Random(l)
    kappa, n = 40, sk.n
    wp, wi = 8, index_bits(17)
    widths = [l, wp, wi]
    SelectLayout(l, kappa, (wp, wi), n.bit_length())                          # fits
    top = (1 << l) - 1
    pairs = [(0, 0), (top, top), (0, top), (top, 0), (5 % (top + 1), 5 % (top + 1))]
    pairs += [(rng.getrandbits(l), rng.getrandbits(l)) for _ in range(4)]
    for x, y in pairs:
        fp, gp, fi, gi = rng.getrandbits(wp), rng.getrandbits(wp), rng.randrange(17), rng.randrange(17)
        f_cs = [sm.enc(sk, v, rng.randrange(1, n)) for v in (x, fp, fi)]
        g_cs = [sm.enc(sk, v, rng.randrange(1, n)) for v in (y, gp, gi)]
        delta = sm.enc(sk, int(x <= y), rng.randrange(1, n))
        draws = sm.draw(rng, kappa, widths, n)
        lo, hi = model.compare_exchange(sk, kappa, widths, delta, f_cs, g_cs, draws)
        lo2, hi2 = model.compare_exchange(sk, kappa, widths, delta, f_cs, g_cs, draws, shared_inversion=False)
        assert (lo, hi) == (lo2, hi2)                                        # the shared inversion is exact, not just equivalent
        want_lo, want_hi = ((x, fp, fi), (y, gp, gi)) if x <= y else ((y, gp, gi), (x, fp, fi))
        assert [sm.dec(sk, c) for c in lo] == list(want_lo)                  # ties: lo = F, hi = G (never exchanged)
        assert [sm.dec(sk, c) for c in hi] == list(want_hi)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_model_sort_with_payload_and_indices(keys, k):
    """The encrypted network (model compare-exchanges) equals the plaintext one, ascending and descending, ties included."""
    from protocols.secure_comparison_amd.selection import index_bits
    from protocols.secure_comparison_amd.sorting import batcher_network

    sk = oracle_paillier(keys, 1024)
    rng = random.Random(40 + k)
    l, wp, kappa, n = 16, 12, 40, sk.n
    widths = [l, wp, index_bits(k)]
    row = [(rng.choice([3, 3, 9, rng.getrandbits(l)]), rng.getrandbits(wp), i) for i in range(k)]
    layers = batcher_network(k)
    for descending in (False, True):
        cur = [[sm.enc(sk, v, rng.randrange(1, n)) for v in t] for t in row]
        for layer in layers:
            for i, j in layer:
                fi, gi = (j, i) if descending else (i, j)
                F, G = cur[fi], cur[gi]
                delta = sm.enc(sk, int(sm.dec(sk, F[0]) <= sm.dec(sk, G[0])), rng.randrange(1, n))
                lo, hi = model.compare_exchange(sk, kappa, widths, delta, F, G, sm.draw(rng, kappa, widths, n))
                cur[fi], cur[gi] = lo, hi
        got = [tuple(sm.dec(sk, c) for c in t) for t in cur]
        (want,) = model.apply(layers, [row], descending)
        assert got == [tuple(t) for t in want]
        keys_sorted = sorted((t[0] for t in row), reverse=descending)
        assert [t[0] for t in got] == keys_sorted
        assert sorted(t[2] for t in got) == list(range(k)) and all(row[t[2]] == t for t in got)


def test_ties_never_exchange():
    from protocols.secure_comparison_amd.sorting import batcher_network

    for k in (2, 5, 8, 17):
        row = [(7, i) for i in range(k)]                                       # all keys equal: the identity, both directions
        for descending in (False, True):
            assert model.apply(batcher_network(k), [row], descending)[0] == row


# ---- validation before any launch ----------------------------------------------------------------------------------------------------
def _stub(nbits=1024):
    """A Paillier stand-in with no engine: any upload or launch would fail with AttributeError, not ValueError."""
    n = (1 << (nbits - 1)) + 1
    return SimpleNamespace(public_key=SimpleNamespace(n=n), mod_n2=SimpleNamespace(nwords=2 * nbits // 32), engine=None)


def _sort(v, l=16, **kw):
    from protocols.secure_comparison_amd.sorting import secure_sort_batch

    ap = _stub()
    return secure_sort_batch(v, l, ap, None, ap, None, **kw)


def test_sort_refuses_bad_arguments_before_any_launch():
    nw2 = 64
    v = torch.zeros((3, 5, nw2), dtype=torch.int32)
    with pytest.raises(ValueError):
        _sort(torch.zeros((3, nw2), dtype=torch.int32))                        # not [B][k][2nw]
    with pytest.raises(ValueError):
        _sort(torch.zeros((3, 5, nw2 - 1), dtype=torch.int32))                 # wrong ciphertext width
    with pytest.raises(ValueError):
        _sort(torch.zeros((3, 0, nw2), dtype=torch.int32))                     # k = 0
    with pytest.raises(ValueError):
        _sort(torch.zeros((1, 1025, nw2), dtype=torch.int32))                  # k > 1024
    with pytest.raises(ValueError):
        _sort(v, l=0)                                                          # l outside check_l
    with pytest.raises(ValueError):
        _sort(v, l=256)
    with pytest.raises(ValueError):
        _sort(v, max_rows=0)
    with pytest.raises(ValueError):
        _sort(v, payload=torch.zeros((1, 3, 4, nw2), dtype=torch.int32), payload_bits=(8,))    # payload shape
    with pytest.raises(ValueError):
        _sort(v, payload=torch.zeros((2, 3, 5, nw2), dtype=torch.int32), payload_bits=(8,))    # widths vs columns
    with pytest.raises(ValueError):
        _sort(v, payload_bits=(8,))                                            # widths without payload
    with pytest.raises(ValueError):
        _sort(v, payload=torch.zeros((3, 3, 5, nw2), dtype=torch.int32), payload_bits=(8, 8, 8), return_indices=True)   # 5 columns
    with pytest.raises(ValueError):
        _sort(v, l=255, payload=torch.zeros((2, 3, 5, nw2), dtype=torch.int32), payload_bits=(400, 400))    # does not fit N
    with pytest.raises(ValueError):
        _sort(v, kappa=0)
    with pytest.raises(AttributeError):                                        # valid arguments reach the (absent) engine
        _sort(v, return_indices=True)


def test_library_exports_the_compare_exchange_finish():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.build import build_lib

    lib = ctypes.CDLL(build_lib(verbose=False))
    assert hasattr(lib, "sc_select_finish_cx")
    assert "sc_select_finish_cx" in _lib.SYMBOLS

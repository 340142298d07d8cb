"""Secure top-m without a GPU: every truncated network for k <= 12 passes the exhaustive 0-1 check with dead outputs left unwritten,
larger ones pass random rows with ties; layers are disjoint, no comparator is all dead and nothing reads a dead output; m = k is
Batcher's network; the comparator counts stay at or below DESIGN 8d's table and the full sort's; both players derive the same
sub-batches; bad arguments are refused before any launch; and the library's sc_topk_network equals the Python network field by field."""
import ctypes
import os
import random
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _topk_model as model  # noqa: E402


def _flat(layers):
    return [c for layer in layers for c in layer]


def _outputs(m, only_last):
    return [m - 1] if only_last else list(range(m))


# ---- the network ---------------------------------------------------------------------------------------------------------------------
def _zero_one_ok(layers, k, m, only_last):
    """All 2^k rows of zeros and ones at once: position p is the integer whose bit r is the value of position p in row r (row r's
    inputs are the bits of r); the minimum of two positions is their AND, the maximum their OR.  Sorted ascending, position p of row
    r holds a one iff the row has more than p zeros short of k ones, i.e. popcount(r) >= k - p."""
    rows = 1 << k
    pos = [sum(((r >> p) & 1) << r for r in range(rows)) for p in range(k)]
    for layer in layers:
        for i, j, keep_i, keep_j in layer:
            lo, hi = pos[i] & pos[j], pos[i] | pos[j]
            if keep_i:
                pos[i] = lo
            if keep_j:
                pos[j] = hi
    ones = [bin(r).count("1") for r in range(rows)]
    return all(pos[p] == sum((ones[r] >= k - p) << r for r in range(rows)) for p in _outputs(m, only_last))


@pytest.mark.parametrize("k", range(1, 13))
def test_every_network_passes_the_zero_one_check_with_dead_outputs_unwritten(k):
    from protocols.secure_comparison_amd.sorting import topk_network

    for m in range(1, k + 1):
        for only_last in (False, True):
            assert _zero_one_ok(topk_network(k, m, only_last), k, m, only_last), (k, m, only_last)


@pytest.mark.parametrize("k,m", [(100, 5), (256, 8), (1000, 10), (1024, 8)])
def test_random_rows_with_ties(k, m):
    from protocols.secure_comparison_amd.sorting import topk_network

    rng = random.Random(k + m)
    rows = []
    for b in range(6):
        pool = [0, 5, 1 << 31, rng.getrandbits(32)] if b % 2 else [rng.getrandbits(32) for _ in range(k // 3 + 1)]
        rows.append([(rng.choice(pool), i) for i in range(k)])
    rows.append([(7, i) for i in range(k)])                                     # all keys equal
    for only_last in (False, True):
        layers = topk_network(k, m, only_last)
        for largest in (False, True):
            for row, out in zip(rows, model.apply(layers, rows, largest)):
                want = sorted((t[0] for t in row), reverse=largest)
                for p in _outputs(m, only_last):
                    assert out[p][0] == want[p] and row[out[p][1]] == out[p], (only_last, largest, p)
                if not only_last:
                    assert len({t[1] for t in out[:m]}) == m                    # m different elements of the row


def test_all_equal_keys_are_never_exchanged():
    from protocols.secure_comparison_amd.sorting import topk_network

    for k, m in ((5, 2), (9, 3), (17, 1), (17, 9)):
        row = [(7, i) for i in range(k)]
        for largest in (False, True):
            assert model.apply(topk_network(k, m), [row], largest)[0] == row


@pytest.mark.parametrize("k", list(range(1, 41)) + [1000, 1024])
def test_structure(k):
    from protocols.secure_comparison_amd.sorting import batcher_network, topk_network

    full = len(_flat(batcher_network(k)))
    for m in (range(1, k + 1) if k <= 40 else (1, 8, 10, k - 1)):
        counts = {}
        for only_last in (False, True):
            layers = topk_network(k, m, only_last)
            assert layers == topk_network(k, m, only_last)                      # a pure function
            for layer in layers:
                assert layer
                touched = [p for c in layer for p in c[:2]]
                assert len(set(touched)) == len(touched)                        # disjoint
                for i, j, keep_i, keep_j in layer:
                    assert 0 <= i < j < k
                    assert keep_i or keep_j                                     # never both dead
            assert model.stale_reads(layers, k, _outputs(m, only_last)) == []
            counts[only_last] = len(_flat(layers))
            assert counts[only_last] <= full
        assert counts[True] <= counts[False]


@pytest.mark.parametrize("k", range(1, 34))
def test_m_equal_k_is_batchers_network(k):
    from protocols.secure_comparison_amd.sorting import batcher_network, topk_network

    layers = topk_network(k, k)
    assert [[(i, j) for i, j, _, _ in layer] for layer in layers] == batcher_network(k)
    assert all(keep_i and keep_j for _, _, keep_i, keep_j in _flat(layers))


# (k, m): (comparators, layers, comparators with one live output) of DESIGN 8d's table
TABLE = {(16, 4): (44, 9, 12), (32, 4): (96, 12, 28), (64, 8): (292, 18, 56), (256, 8): (1228, 26, 248), (1000, 10): (6893, 40, 990),
         (1024, 8): (4972, 34, 1016), (1024, 1): (1023, 10, 1023)}


def test_comparator_counts_stay_below_the_table():
    from protocols.secure_comparison_amd.sorting import topk_network

    for (k, m), (comparators, layers, half) in TABLE.items():
        net = topk_network(k, m)
        assert len(_flat(net)) <= comparators and len(net) <= layers, (k, m)
        assert sum(1 for c in _flat(net) if not (c[2] and c[3])) <= half, (k, m)
    # where the truncated merges lose to the pruned full sort, the minimum of the two is what counts
    assert len(_flat(topk_network(9, 5))) <= 28
    assert len(_flat(topk_network(17, 9))) <= 85


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,only_last,B,max_rows", [(5, 2, False, 3, 2), (17, 3, False, 64, 100), (9, 5, True, 7, 10), (8, 8, False, 4, 5),
                                                       (17, 1, False, 6, 65536)])
@pytest.mark.parametrize("largest", [False, True])
def test_counts_agree_with_the_initiators_steps(k, m, only_last, B, max_rows, largest):
    from protocols.secure_comparison_amd.sorting import _topk_steps, topk_counts, topk_network, topk_schedule

    nf = 2
    buf = torch.arange(nf * B * k * 2, dtype=torch.int32).reshape(nf, B * k, 2)
    steps = list(_topk_steps(buf, B, k, m, only_last, max_rows, largest))
    counts = topk_counts(k, m, only_last, B, max_rows)
    assert [f.shape[1] for f, _, _, _ in steps] == counts and all(1 <= c <= max_rows for c in counts)
    assert sum(counts) == B * len(_flat(topk_network(k, m, only_last)))
    # every comparison t = c * B + b of a layer reads rows b k + i / b k + j and writes them, or the row past the buffer when dead
    dead = nf * B * k
    it = iter(steps)
    for layer, cuts in topk_schedule(k, m, only_last, B, max_rows):
        want = []
        for i, j, keep_i, keep_j in layer:
            for b in range(B):
                (fp, fk), (gp, gk) = ((j, keep_j), (i, keep_i)) if largest else ((i, keep_i), (j, keep_j))
                want.append((b * k + fp, b * k + gp, fk, gk))
        for a, z in cuts:
            f, g, lo, hi = next(it)
            for t, (fr, gr, fk, gk) in enumerate(want[a:z]):
                for c in range(nf):
                    assert torch.equal(f[c, t], buf[c, fr]) and torch.equal(g[c, t], buf[c, gr])
                    assert lo[c, t].item() == (c * B * k + fr if fk else dead)
                    assert hi[c, t].item() == (c * B * k + gr if gk else dead)
    assert next(it, None) is None


# ---- validation before any launch ----------------------------------------------------------------------------------------------------
def test_network_and_schedule_refuse_bad_arguments():
    from protocols.secure_comparison_amd.sorting import topk_counts, topk_network, topk_schedule

    for k, m in ((0, 1), (1025, 1), (5, 0), (5, 6), (5, -1)):
        with pytest.raises(ValueError):
            topk_network(k, m)
        with pytest.raises(ValueError):
            topk_network(k, m, True)
    with pytest.raises(ValueError):
        topk_schedule(5, 2, False, 3, 0)
    with pytest.raises(ValueError):
        topk_counts(5, 6, False, 3, 10)


def _stub(nbits=1024):
    """A Paillier stand-in with no engine: any upload or launch would fail with AttributeError, not ValueError."""
    n = (1 << (nbits - 1)) + 1
    return SimpleNamespace(public_key=SimpleNamespace(n=n), mod_n2=SimpleNamespace(nwords=2 * nbits // 32), engine=None)


def test_topk_refuses_bad_arguments_before_any_launch():
    from protocols.secure_comparison_amd import sorting

    ap = _stub()
    nw2 = 64
    v = torch.zeros((3, 5, nw2), dtype=torch.int32)
    topk = lambda v, m, l=16, **kw: sorting.secure_topk_batch(v, m, l, ap, None, ap, None, **kw)  # noqa: E731
    kth = lambda v, r, l=16, **kw: sorting.secure_kth_batch(v, r, l, ap, None, ap, None, **kw)  # noqa: E731
    for m in (0, 6, -1, 2.5):
        with pytest.raises(ValueError):
            topk(v, m, return_indices=True)
    for r in (-1, 5, 1.5):
        with pytest.raises(ValueError):
            kth(v, r, return_indices=True)
    with pytest.raises(ValueError):
        topk(torch.zeros((3, nw2), dtype=torch.int32), 1)                      # not [B][k][2nw]
    with pytest.raises(ValueError):
        topk(torch.zeros((3, 5, nw2 - 1), dtype=torch.int32), 2)               # wrong ciphertext width
    with pytest.raises(ValueError):
        topk(torch.zeros((1, 1025, nw2), dtype=torch.int32), 2)                # k > 1024
    with pytest.raises(ValueError):
        topk(v, 2, l=0)
    with pytest.raises(ValueError):
        topk(v, 2, max_rows=0)
    with pytest.raises(ValueError):
        topk(v, 2, payload_bits=(8,))                                          # widths without payload
    with pytest.raises(ValueError):
        topk(v, 2, payload=torch.zeros((3, 3, 5, nw2), dtype=torch.int32), payload_bits=(8, 8, 8), return_indices=True)   # 5 columns
    with pytest.raises(ValueError):
        sorting.secure_median_batch(torch.zeros((3, 0, nw2), dtype=torch.int32), 16, ap, None, ap, None, return_indices=True)   # k = 0
    with pytest.raises(ValueError):
        sorting.secure_median_batch(torch.zeros((3, nw2), dtype=torch.int32), 16, ap, None, ap, None)
    for call in (lambda: topk(v, 2, return_indices=True), lambda: kth(v, 4, return_indices=True),
                 lambda: sorting.secure_median_batch(v, 16, ap, None, ap, None, return_indices=True)):
        with pytest.raises(AttributeError):                                    # valid arguments reach the (absent) engine
            call()


# ---- the library's network -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.build import build_lib

    path = build_lib(verbose=False)
    assert hasattr(ctypes.CDLL(path), "sc_topk_network") and "sc_topk_network" in _lib.SYMBOLS
    return _lib.load()


def _c_network(lib, k, m, only_last):
    """(rc of the size query, layers as Python would give them) through the two-call sequence of a C host."""
    n, nl = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sc_topk_network(k, m, int(only_last), 0, None, None, None, ctypes.byref(n), ctypes.byref(nl))
    if rc != 0:
        return rc, None
    cap = max(n.value, 1)
    ij, keep, ends = (ctypes.c_int32 * (2 * cap))(), (ctypes.c_uint8 * (2 * cap))(), (ctypes.c_int32 * cap)()
    n2, nl2 = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.sc_topk_network(k, m, int(only_last), cap, ij, keep, ends, ctypes.byref(n2), ctypes.byref(nl2)) == 0
    assert (n2.value, nl2.value) == (n.value, nl.value) and nl.value <= n.value
    assert all(v in (0, 1) for v in keep[:2 * n.value])
    flat = [(ij[2 * t], ij[2 * t + 1], bool(keep[2 * t]), bool(keep[2 * t + 1])) for t in range(n.value)]
    bounds = [0] + list(ends[:nl.value])
    assert bounds[-1] == n.value
    return 0, [flat[a:b] for a, b in zip(bounds, bounds[1:])]


@pytest.mark.parametrize("k", list(range(1, 41)) + [1000, 1024])
def test_library_network_equals_python(lib, k):
    from protocols.secure_comparison_amd.sorting import topk_network

    for m in (range(1, k + 1) if k <= 40 else ((10, k) if k == 1000 else (8, 1))):
        for only_last in (False, True):
            rc, layers = _c_network(lib, k, m, only_last)
            assert rc == 0 and layers == topk_network(k, m, only_last), (k, m, only_last)


def test_library_network_size_query_and_refusals(lib):
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.sorting import topk_network

    n, nl = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.sc_topk_network(16, 4, 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(nl)) == 0       # cap = 0, null arrays
    net = topk_network(16, 4)
    assert (n.value, nl.value) == (len(_flat(net)), len(net)) == (44, 9)
    assert lib.sc_topk_network(1, 1, 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(nl)) == 0 and (n.value, nl.value) == (0, 0)
    err = -1                                                                    # SC_ERR_ARG
    for k, m in ((0, 1), (1025, 1), (5, 0), (5, 6), (5, -1)):
        assert lib.sc_topk_network(k, m, 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(nl)) == err
    assert lib.sc_topk_network(16, 4, 2, 0, None, None, None, ctypes.byref(n), ctypes.byref(nl)) == err
    assert lib.sc_topk_network(16, 4, 0, 0, None, None, None, None, None) == err
    ij, keep, ends = (ctypes.c_int32 * 86)(), (ctypes.c_uint8 * 86)(), (ctypes.c_int32 * 43)()
    ij[0] = keep[0] = ends[0] = 77
    assert lib.sc_topk_network(16, 4, 0, 43, ij, keep, ends, ctypes.byref(n), ctypes.byref(nl)) == err      # one entry short
    assert (n.value, nl.value) == (44, 9) and (ij[0], keep[0], ends[0]) == (77, 77, 77)                     # sizes, arrays untouched
    assert lib.sc_topk_network(16, 4, 0, 44, None, None, None, ctypes.byref(n), ctypes.byref(nl)) == err    # cap > 0 needs the arrays
    assert _lib.ABI_VERSION == lib.sc_abi_version() == 5                                                     # an addition

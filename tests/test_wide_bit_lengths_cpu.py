"""CPU tier of the wide comparisons (65 <= l <= 255): the host draws of bounds of any width, the flag-row layout, the range check."""
import hashlib
import random

import numpy as np
import pytest
import torch

from oracle import sc_oracle as o
from protocols.secure_comparison_amd.flags import (MAX_L, check_l, flag_bit_planes, flag_rows_of, flag_shape, flag_words, pack_flags,
                                                   unpack_flags)
from protocols.secure_comparison_amd.host_draws import HostDraws


def _seeded(seed):
    rng = random.Random(seed)
    return HostDraws(lambda n: rng.randbytes(n))


def _ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


@pytest.mark.parametrize("bits", [131, 258])
def test_below_rows_nonzero_wide_bounds(bits):
    """rho_i = 1 + randbelow(u - 1) for u of 131 bits (l = 128) and 258 bits (l = 255): every value in [1, u), rows of
    ceil(bits / 32) words, and every 64-bit column of the candidates used (the top one up to u's top bit)."""
    u = o.next_prime(1 << (bits - 1))
    d = _seeded(bits)
    rows = d.below_rows_nonzero(u, 4000)
    assert rows.shape == (4000, (bits + 31) // 32) and rows.dtype == np.dtype("<u4")
    vals = _ints(rows)
    assert min(vals) >= 1 and max(vals) < u
    for j in range((bits + 63) // 64):
        assert any((v >> (64 * j)) & ((1 << 64) - 1) for v in vals), j
    assert max(vals).bit_length() == bits - 1 or max(vals).bit_length() == bits
    assert len(set(vals)) == len(vals)
    # u itself 2^259 wide (l = 255 with the largest bound the issue names): still in range
    big = (1 << 259) - 1
    vals = _ints(_seeded(1).below_rows_nonzero(big, 2000))
    assert min(vals) >= 1 and max(vals) < big and max(vals).bit_length() == 259


# Outputs of the <= 62-bit and <= 126-bit branches for a fixed byte stream, recorded from the code before bounds above 126 bits
# were accepted: (bound, sha256 prefix of the 1000 rows, the first two values).
_PINNED = [
    ((1 << 18) + 3, "f71eef51733d85d1fdb53ee149896b72", [238673, 208692]),
    ((1 << 40) + 15, "f8a4260cfcce05bdf93fb330d9a9b142", [154929934132, 75316039724]),
    ((1 << 62) + 1, "c7b800663691331e185e98d3776493d3", [890727360438182993, 1736392818365009964]),
    (1 << 62, "c229625fe56fa15705f21c2fe9fa9bba", [3649971666045809721, 2671521945691753784]),
    ((1 << 66) + 5, "45d78e4b3bfc14335d40f11e7a29f5a6", [56230959581566837841, 1736392818365009964]),
    ((1 << 100) - 3, "3e18633149bb8651e88bacde3e33db4f", [1121145778275231181411501651001, 322651643815667365059456377937]),
]


@pytest.mark.parametrize("bound, digest, first", _PINNED)
def test_narrow_branches_unchanged(bound, digest, first):
    rows = _seeded(7)._below_rows_nonzero(bound, 1000)
    assert hashlib.sha256(rows.tobytes()).hexdigest()[:32] == digest
    assert _ints(rows[:2]) == first


@pytest.mark.parametrize("n", [0, 1, -5])
def test_degenerate_bounds_raise(n):
    d = HostDraws(lambda k: bytes(k))          # an all-zero stream: a loop that never ends would hang here, not fail
    with pytest.raises(ValueError):
        d.below_rows_nonzero(n, 3)
    with pytest.raises(ValueError):
        d._below_rows_nonzero(n, 3)
    if n < 1:
        with pytest.raises(ValueError):
            d.randbelow(n)


def test_randbelow_wide():
    d = _seeded(3)
    for bound in ((1 << 259) - 1, o.next_prime(1 << 257), (1 << 200) + 1):
        vals = [d.randbelow(bound) for _ in range(200)]
        assert all(0 <= v < bound for v in vals) and max(vals).bit_length() >= bound.bit_length() - 8


@pytest.mark.parametrize("l", [63, 64, 65, 127, 128, 129, 255])
def test_flag_rows_pack_unpack(l):
    rng = random.Random(l)
    vals = [0, 1, (1 << l) - 1, (1 << (l - 1)), ((1 << l) - 1) ^ 1] + [rng.randrange(1 << l) for _ in range(40)]
    if l > 64:
        vals += [(1 << 64) - 1, 1 << 64, ((1 << l) - 1) >> 1]
    arr = pack_flags(vals, l)
    assert arr.dtype == np.uint64 and arr.shape == flag_shape(len(vals), l)
    assert arr.shape == ((len(vals),) if l <= 64 else (len(vals), flag_words(l)))
    assert unpack_flags(arr, l) == vals
    assert unpack_flags(torch.from_numpy(arr.view(np.int64)), l) == vals
    for i, v in enumerate(vals):         # little-endian words, bits above l zero
        words = arr.reshape(len(vals), -1)[i]
        assert [int(w) for w in words] == [(v >> (64 * j)) & ((1 << 64) - 1) for j in range(flag_words(l))]
    # the coalesced path's per-session entries (`.tolist()` of the int64 array) joined again
    assert np.array_equal(flag_rows_of(torch.from_numpy(arr.view(np.int64)).tolist(), l), arr)
    planes = flag_bit_planes(torch.from_numpy(arr.view(np.int64)), l)
    assert planes.shape == (l, len(vals))
    assert planes.tolist() == [[(v >> i) & 1 for v in vals] for i in range(l)]
    with pytest.raises(ValueError):
        pack_flags([1 << l], l)


@pytest.mark.parametrize("l", [0, -1, 256, 1000, 2.0, True])
def test_check_l_range(l):
    with pytest.raises(ValueError, match="1 <= l <= 255"):
        check_l(l)


def test_check_l_accepts_the_range():
    assert [check_l(v) for v in (1, 64, 65, MAX_L)] == [1, 64, 65, 255]

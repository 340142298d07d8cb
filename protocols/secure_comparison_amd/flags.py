"""Flag rows: the plaintext bit fields alpha, alpha~ (Alice) and beta (Bob) of a batch of l-bit comparisons.

A flag row is lw = ceil(l / 64) little-endian uint64 words per comparison, laid out [count][lw], the bits above l zero
(include/sc_amd.h, FLAG ROWS).  For l <= 64 the array is [count] -- one word per comparison, the layout of every earlier
release.  The library takes comparisons of 1 <= l <= 255 bits: l + 1 bit planes fit the device shuffle (byte entries) and the
8-bit flag-bit fields of the interpreter's programs.  r_small, delta_A, d and delta_B stay one word per comparison.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np
import torch

MAX_L = 255


def check_l(l: int) -> int:
    """l itself when the batched library can compare l-bit integers; ValueError naming the range otherwise."""
    if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not 1 <= int(l) <= MAX_L:
        raise ValueError(f"1 <= l <= {MAX_L} is required for the batched comparison (l + 1 bit planes), got l = {l!r}")
    return int(l)


def flag_words(l: int) -> int:
    """uint64 words per flag row."""
    return (int(l) + 63) // 64


def flag_shape(count: int, l: int) -> tuple[int, ...]:
    """Shape of a batch's flag array: [count] for l <= 64, [count][ceil(l / 64)] above."""
    return (count,) if l <= 64 else (count, flag_words(l))


def pack_flags(values: Iterable[int], l: int) -> np.ndarray:
    """Non-negative integers below 2^l as a uint64 flag array of flag_shape(len(values), l)."""
    values = [int(v) for v in values]
    lw = flag_words(l)
    for v in values:
        if v < 0 or v >> l:
            raise ValueError(f"flag value {v} does not fit {l} bits")
    buf = b"".join(v.to_bytes(8 * lw, "little") for v in values)
    arr = np.frombuffer(buf, dtype="<u8").reshape(len(values), lw).copy()
    return arr.reshape(flag_shape(len(values), l))


def unpack_flags(arr, l: int) -> list[int]:
    """The integers of a flag array ([count] or [count][lw] of uint64 or int64, numpy or torch)."""
    if isinstance(arr, torch.Tensor):
        arr = arr.detach().cpu().numpy()
    a = np.ascontiguousarray(arr).view("<u8").reshape(arr.shape[0] if arr.ndim else 1, -1)
    if a.shape[1] != flag_words(l):
        raise ValueError(f"flag rows of {a.shape[1]} words, expected {flag_words(l)} for l = {l}")
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def flag_rows_of(rows: list, l: int) -> np.ndarray:
    """Per-comparison entries of a flag array (ints from `.tolist()` of a [count] array, or lists of words from a [count][lw] one)
    joined again into one uint64 array of flag_shape(len(rows), l)."""
    if l <= 64:
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in rows], dtype=np.uint64)
    return np.array([[int(w) & 0xFFFFFFFFFFFFFFFF for w in r] for r in rows], dtype=np.uint64).reshape(len(rows), flag_words(l))


def flag_bit_planes(flags: torch.Tensor, l: int) -> torch.Tensor:
    """int64 [l][count]: bit i of every comparison's flag row (plane i), 0 or 1."""
    count = flags.shape[0]
    f = flags.reshape(count, flag_words(l))
    i = torch.arange(l, device=flags.device, dtype=torch.int64)
    words = f[:, i // 64].T                                         # [l][count]: the word that holds bit i
    return (words >> (i % 64).reshape(l, 1)) & 1

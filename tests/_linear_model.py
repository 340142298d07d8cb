"""Plain-Python model of the linear map with public weights along an axis (sc_modlin_axis): the residues, the signed
split into members and non-negative weights, the fit rule, and the weight rows every test matrix holds."""
from __future__ import annotations

U64 = (1 << 64) - 1


def lin_axis(n: int, ops: list[int], outer: int, K: int, inner: int, W: list[list[int]]) -> list[int]:
    """out[o][j][i] = prod_k x[o][k][i]^W[j][k] mod n for x flat in [outer][K][inner] order and W [J][K] >= 0; flat [outer][J][inner]."""
    assert len(ops) == outer * K * inner and all(len(row) == K and all(v >= 0 for v in row) for row in W)
    out = []
    for o in range(outer):
        for row in W:
            for i in range(inner):
                acc = 1 % n
                for k, wk in enumerate(row):
                    acc = acc * pow(ops[(o * K + k) * inner + i], wk, n) % n
                out.append(acc)
    return out


def split_signed(W: list[list[int]]) -> tuple[list[tuple[int, bool]], list[list[int]]]:
    """(members, W'): the members the kernel sees -- (k, False) for every plane, then (k, True), the negated plane, for every k some row
    weighs negatively -- and the non-negative weights of those members, member by member."""
    K = len(W[0])
    members = [(k, False) for k in range(K)] + [(k, True) for k in range(K) if any(row[k] < 0 for row in W)]
    return members, [[(-row[k] if neg else row[k]) if (row[k] < 0) == neg else 0 for k, neg in members] for row in W]


def fits(W: list[list[int]], x_bits: int, nbits: int) -> list[bool]:
    """Per row: bits(sum_k |W[j][k]|) + x_bits + 1 < nbits - 1."""
    return [sum(abs(v) for v in row).bit_length() + x_bits + 1 < nbits - 1 for row in W]


def signed_map(W: list[list[int]], bias: list[int] | None, x: list[list[int]]) -> list[list[int]]:
    """y[j][b] = sum_k W[j][k] x[k][b] + bias[j] over the integers, x [K][B]."""
    B = len(x[0])
    return [[sum(wk * x[k][b] for k, wk in enumerate(row)) + (bias[j] if bias else 0) for b in range(B)] for j, row in enumerate(W)]


def edge_rows(K: int, salt: int = 0) -> list[list[int]]:
    """The five weight rows a test matrix must hold, K entries each: all zero; a single 1; a single 2^63; all 2^64 - 1; mixed widths
    (1, 8, 16, 33 and 64 bits in turn), so that rows sharing a launch differ in their widest weight.  `salt` moves the single entries."""
    at = salt % K
    single = lambda v: [v if k == at else 0 for k in range(K)]  # noqa: E731
    widths = (1, 8, 16, 33, 64)
    mixed = [((0x9E3779B97F4A7C15 * (k + 1 + salt)) & U64) >> (64 - widths[(k + salt) % 5]) | 1 << (widths[(k + salt) % 5] - 1) | 1 for k in range(K)]
    return [[0] * K, single(1), single(1 << 63), [U64] * K, mixed]


def matrix(K: int, J: int, salt: int = 0) -> list[list[int]]:
    """J rows out of edge_rows(K), starting at row `salt` and wrapping; for J >= 5 all of them."""
    rows = edge_rows(K, salt)
    return [rows[(salt + j) % 5] for j in range(J)]

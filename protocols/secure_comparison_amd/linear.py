"""Linear maps with public weights over encrypted vectors.

y_j = sum_k W[j][k] x_k + b_j with W and b known to the party that holds [[x]]: c_k^W[j][k] multiplied over k, modulo N^2.
linear_planes_batch / linear_rows_batch run it along one axis of an array with the dedicated kernel k_lin_axis
(sc_paillier_linear_axis, include/sc_amd.h): every member is lifted to Montgomery form once, the K members of an output share one
squaring chain, and the weight bits -- the same for every row of the batch -- steer a branch the whole wave takes.  No interaction and
no randomness: the result is a deterministic function of the inputs, so a caller who hands it on passes `rho` to re-randomize it.

Signed weights cost one batched inversion: the planes that carry a negative weight are negated once (neg_batch) and appended as extra
members, so the kernel sees at most 2K members and non-negative weights only.  A bias is added as the unrandomized [[b_j]].
"""
from __future__ import annotations

import torch

from .aggregate import _planes_geometry, _rerandomize, _rows_geometry
from .schemes import Paillier

MAX_AXIS = 1024                     # K and J of one library call (sc_modlin_axis)
WEIGHT_LIMIT = 1 << 64              # |w| stays below it


def check_weights(weights, K: int | None = None) -> list[list[int]]:
    """`weights` as J >= 1 rows of K >= 1 Python ints: nested sequences of ints or a CPU int64 tensor [J][K].  ValueError for anything
    else, a ragged matrix, a row length other than `K` (when given), and |w| >= 2^64."""
    if isinstance(weights, torch.Tensor):
        if weights.dim() != 2 or weights.dtype != torch.int64 or weights.device.type != "cpu":
            raise ValueError("weights: expected a CPU int64 tensor [J][K] or nested lists of integers")
        weights = weights.tolist()
    try:
        rows = [list(row) for row in weights]
    except TypeError:
        raise ValueError("weights: expected [J][K] integers") from None
    if not rows or not rows[0]:
        raise ValueError("weights: expected at least one row and one column")
    width = len(rows[0]) if K is None else int(K)
    for j, row in enumerate(rows):
        if len(row) != width:
            raise ValueError(f"weights: row {j} has {len(row)} entries, expected {width}")
        for v in row:
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"weights: row {j} holds {v!r}, expected integers")
            if abs(v) >= WEIGHT_LIMIT:
                raise ValueError(f"weights: row {j} holds {v}, expected |w| < 2^64")
    return rows


def split_signed(rows: list[list[int]]) -> tuple[list[int], list[list[int]]]:
    """The signed split of a weight matrix [J][K]: (negated, W') with `negated` the members k that carry at least one negative weight,
    in ascending order, and W' [J][K + len(negated)] non-negative: column k holds max(w, 0), column K + t holds max(-w, 0) of member
    negated[t].  sum_k W[j][k] x_k = sum_k W'[j][k] x_k + sum_t W'[j][K + t] (-x_negated[t])."""
    K = len(rows[0])
    negated = [k for k in range(K) if any(row[k] < 0 for row in rows)]
    return negated, [[max(v, 0) for v in row] + [max(-row[k], 0) for k in negated] for row in rows]


def check_fit(rows: list[list[int]], x_bits: int, nbits: int) -> None:
    """The fit rule, dot_layout's convention: a row's result of up to bits(sum_k |W[j][k]|) + x_bits bits and its sign must stay below
    bits(N) - 1.  ValueError naming the first row j for which bits(sum_k |W[j][k]|) + x_bits + 1 < nbits - 1 does not hold."""
    x_bits = int(x_bits)
    if x_bits < 1:
        raise ValueError("x_bits: expected at least 1")
    for j, row in enumerate(rows):
        need = sum(abs(v) for v in row).bit_length() + x_bits + 1
        if not need < nbits - 1:
            raise ValueError(f"row {j}: weights of {need - x_bits - 1} bits in sum times inputs of {x_bits} bits ({need} bits with the sign) "
                             f"do not fit below a {nbits}-bit N")


def check_bias(bias, J: int, n: int) -> list[int] | None:
    """`bias` as J residues modulo N (a negative b as N - |b|), or None.  ValueError for a wrong length, a non-integer, |b| >= N."""
    if bias is None:
        return None
    if isinstance(bias, torch.Tensor):
        bias = bias.tolist()
    try:
        bias = list(bias)
    except TypeError:
        raise ValueError(f"bias: expected {J} integers") from None
    if len(bias) != J:
        raise ValueError(f"bias: {len(bias)} entries, expected one per row of the weights ({J})")
    for b in bias:
        if isinstance(b, bool) or not isinstance(b, int) or abs(b) >= n:
            raise ValueError(f"bias: {b!r}, expected an integer with |b| < N")
    return [b if b >= 0 else n - (-b) for b in bias]


def _prepare(weights, K: int, paillier: Paillier, bias, x_bits):
    """Every check that needs no launch, in one order: the matrix, the axis limits, the bias, the fit rule; then the signed split."""
    rows = check_weights(weights, K)
    J = len(rows)
    if J > MAX_AXIS:
        raise ValueError(f"weights: {J} rows, at most {MAX_AXIS} per call")
    n = paillier.public_key.n
    residues = check_bias(bias, J, n)
    if x_bits is not None:
        check_fit(rows, x_bits, n.bit_length())
    negated, nonneg = split_signed(rows)
    if K + len(negated) > MAX_AXIS:
        raise ValueError(f"{K} members and {len(negated)} negated ones: at most {MAX_AXIS} per call")
    return J, residues, negated, nonneg


def _add_bias(out: torch.Tensor, residues: list[int] | None, repeat_inner: int, repeat_outer: int, paillier: Paillier) -> torch.Tensor:
    """out [outer * J * inner][2nw] times the unrandomized [[b_j]] of its row j."""
    if residues is None:
        return out
    nw = paillier.mod_n.nwords
    flat = [b for _ in range(repeat_outer) for b in residues for _ in range(repeat_inner)]
    return paillier.add_batch(out, paillier.encrypt_raw_batch(paillier.engine.upload(flat, nw)))


def linear_planes_batch(x_enc: torch.Tensor, weights, paillier: Paillier, bias=None, x_bits: int | None = None,
                        rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_k W[j][k] x[k][b] + bias[j]]] for x_enc [K][B][2nw] and public W [J][K] -> [J][B][2nw]: a linear map over the planes,
    geometry (outer, K, inner) = (1, K, B).  weights: signed integers with |w| < 2^64, nested lists or a CPU int64 tensor; bias: J
    public integers (optional).  x_bits (optional) turns the fit rule on: ValueError naming row j unless
    bits(sum_k |W[j][k]|) + x_bits + 1 < bits(N) - 1.  rho [J][B][nw] (optional) re-randomizes the result."""
    x, (_, K, B) = _planes_geometry(x_enc)
    J, residues, negated, nonneg = _prepare(weights, K, paillier, bias, x_bits)
    if B < 1:
        raise ValueError("x_enc: expected at least one row")
    w = x.shape[-1]
    if negated:
        minus = paillier.neg_batch(x[negated].reshape(len(negated) * B, w).contiguous()).reshape(len(negated), B, w)
        x = torch.cat([x, minus], dim=0).contiguous()
    out = paillier.engine.paillier_linear_axis(paillier.key, x, 1, x.shape[0], B, nonneg)
    out = _add_bias(out, residues, B, 1, paillier)
    return _rerandomize(out.reshape(J, B, w), paillier, rho)


def linear_rows_batch(x_enc: torch.Tensor, weights, paillier: Paillier, segment: int | None = None, bias=None, x_bits: int | None = None,
                      rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_b W[j][b] x[..][b] + bias[j]]] over the rows of every plane of x_enc [..., B][2nw] with public W [J][B] -> [..., J][2nw];
    with `segment` one map per run of `segment` consecutive rows, W [J][segment] -> [..., B / segment, J][2nw] (segment must divide B:
    ValueError).  Geometry (planes * B / segment, segment, 1).  weights, bias, x_bits as in linear_planes_batch; rho (one [nw] row per
    result, optional) re-randomizes the results."""
    x, (outer, seg, _) = _rows_geometry(x_enc, segment)
    J, residues, negated, nonneg = _prepare(weights, seg, paillier, bias, x_bits)
    w = x.shape[-1]
    members = x.reshape(outer, seg, w)
    if negated:
        minus = paillier.neg_batch(members[:, negated].reshape(outer * len(negated), w).contiguous()).reshape(outer, len(negated), w)
        members = torch.cat([members, minus], dim=1)
    members = members.contiguous()
    out = paillier.engine.paillier_linear_axis(paillier.key, members, outer, members.shape[1], 1, nonneg)
    out = _add_bias(out, residues, 1, outer, paillier)
    shape = tuple(x.shape[:-2]) + (() if segment is None else (x.shape[-2] // seg,)) + (J, w)
    return _rerandomize(out.reshape(shape), paillier, rho)


__all__ = ["check_bias", "check_fit", "check_weights", "linear_planes_batch", "linear_rows_batch", "split_signed"]

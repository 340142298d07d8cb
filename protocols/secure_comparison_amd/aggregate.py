"""Sums of encrypted arrays along an axis, and the histogram, majority vote and group-by that follow from them.

The sum of Paillier ciphertexts is their product modulo N^2.  sum_planes_batch / sum_rows_batch run it along one axis of an array with the
dedicated kernel k_prod_axis (sc_paillier_sum_axis, include/sc_amd.h): a tree of chains of at most 32 members, one Montgomery product per
member, one launch per level, no interaction and no randomness -- the result is a deterministic function of the inputs, so a caller who
hands it on passes `rho` to re-randomize it.

The two-party operations add no protocol of their own.  secure_histogram_batch is the one-hot encoding (lookup.py) summed over the indices
of a row, secure_majority_batch the argmax (selection.py) of that histogram, secure_groupby_count_batch / secure_groupby_sum_batch the
one-hot encoding (times the value: multiplication.py) summed over the rows.  Their draws are the one-hot's, the multiplication's and the
comparison's, in that order.
"""
from __future__ import annotations

import torch

from .lookup import OnehotDraws, _as_planes, _layout as _onehot_layout, draw_onehot, onehot_batch
from .multiplication import MulDraws, MulLayout, draw_mul, mul_batch
from .schemes import DGK, Paillier

MIN_CHUNK, MAX_CHUNK = 4, 32        # automatic chunk lengths of a level (reduce_plan in csrc/sc_lib.hip)


def reduce_plan(outer: int, K: int, inner: int, resident_groups: int, forced: int = 0) -> list[tuple[int, int, int]]:
    """The levels (K, chunk, chains per output) of sc_modprod_axis' tree, as reduce_plan in csrc/sc_lib.hip computes them: a level cuts
    the K members of an output into ceil(K / chunk) chains and hands that many partials to the next level, until one is left.  chunk: the
    shortest of 4 .. 32 members whose chains still fill `resident_groups` group slots (num_cu * 8 * 64 / G), or `forced` (2 .. 32,
    Engine.set_reduce_chunk) at every level; never more than K."""
    outer, K, inner, forced = int(outer), int(K), int(inner), int(forced)
    if K < 1 or outer < 1 or inner < 1 or resident_groups < 1:
        raise ValueError("reduce_plan: expected positive sizes")
    if forced != 0 and not 2 <= forced <= MAX_CHUNK:
        raise ValueError(f"forced chunk {forced}: expected 0 or 2 .. {MAX_CHUNK}")
    levels = []
    while True:
        c = forced if forced else min(MAX_CHUNK, max(MIN_CHUNK, -(-outer * K * inner // resident_groups)))
        c = min(c, K)
        nch = -(-K // c)
        levels.append((K, c, nch))
        if nch == 1:
            return levels
        K = nch


def _rerandomize(out: torch.Tensor, paillier: Paillier, rho: torch.Tensor | None) -> torch.Tensor:
    if rho is None:
        return out
    flat = out.reshape(-1, out.shape[-1])
    return paillier.randomize_batch(flat, rho.reshape(flat.shape[0], -1).contiguous()).reshape(out.shape)


def _cipher_array(x_enc, min_dim: int, name: str) -> torch.Tensor:
    if not isinstance(x_enc, torch.Tensor) or x_enc.dim() < min_dim:
        raise ValueError(f"{name}: expected an array of at least {min_dim} axes, [...][words]")
    return x_enc.contiguous()


def sum_planes_batch(x_enc: torch.Tensor, paillier: Paillier, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_j x[j][b]]] for x_enc [k][B][2nw] -> [B][2nw]: the sum over the planes, geometry (outer, K, inner) = (1, k, B).
    rho [B][nw] (optional) re-randomizes the result."""
    x = _cipher_array(x_enc, 3, "x_enc")
    if x.dim() != 3 or x.shape[0] < 1:
        raise ValueError("x_enc: expected [k][B][words] with k >= 1")
    k, B, _ = x.shape
    return _rerandomize(paillier.engine.paillier_sum_axis(paillier.key, x, 1, k, B), paillier, rho)


def check_segment(B: int, segment: int | None) -> int:
    """The segment length of sum_rows_batch over B rows: B itself by default; ValueError unless 1 <= segment and segment divides B."""
    if segment is None:
        segment = B
    segment = int(segment)
    if segment < 1 or B % segment != 0:
        raise ValueError(f"segment = {segment}: expected a divisor of the {B} rows")
    return segment


def sum_rows_batch(x_enc: torch.Tensor, paillier: Paillier, segment: int | None = None, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_b x[..][b]]] over the rows of every plane of x_enc [..., B][2nw] -> [...][2nw]; with `segment` one total per run of `segment`
    consecutive rows -> [..., B / segment][2nw] (segment must divide B: ValueError).  Geometry (planes * B / segment, segment, 1).
    rho (one [nw] row per result, optional) re-randomizes the results."""
    x = _cipher_array(x_enc, 2, "x_enc")
    B, w = x.shape[-2], x.shape[-1]
    if B < 1:
        raise ValueError("x_enc: expected at least one row")
    seg = check_segment(B, segment)
    planes = x.numel() // (B * w)
    out = paillier.engine.paillier_sum_axis(paillier.key, x, planes * (B // seg), seg, 1)
    shape = tuple(x.shape[:-2]) + (() if segment is None else (B // seg,)) + (w,)
    return _rerandomize(out.reshape(shape), paillier, rho)


# ---- histogram, majority, group-by ------------------------------------------------------------------------------------------------
def secure_histogram_batch(index_enc: torch.Tensor, k: int, alice_paillier: Paillier, bob_paillier: Paillier, index_bits: int | None = None,
                           kappa: int = 40, draws: OnehotDraws | None = None, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[#{q : i_q mod k == t}]], t < k, for B rows of m encrypted indices each: index_enc [m][B][2nw] -> [k][B][2nw].  The one-hot encoding
    of the m indices (one round trip), then the sum over q.  0 <= i_q < 2^index_bits; an index at or above k counts at i_q mod k, as in
    secure_onehot_batch."""
    planes, _ = _as_planes(index_enc)
    layout = _onehot_layout(planes, k, index_bits, kappa, alice_paillier)                 # the fit rule, before any launch
    m, B = planes.shape[0], planes.shape[1]
    draws = draws if draws is not None else draw_onehot(B, layout, alice_paillier)
    onehot = onehot_batch(layout, planes, alice_paillier, bob_paillier, draws)            # [m][k][B][2nw]
    out = alice_paillier.engine.paillier_sum_axis(alice_paillier.key, onehot, 1, m, layout.k * B).reshape(layout.k, B, -1)
    return _rerandomize(out, alice_paillier, rho)


def count_bits(m: int) -> int:
    """Width of a count of at most m: bits(m)."""
    return max(1, int(m).bit_length())


def secure_majority_batch(label_enc: torch.Tensor, k: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                          index_bits: int | None = None, kappa: int = 40, draws: OnehotDraws | None = None):
    """([[the most frequent label]], [[its count]]) for B rows of m encrypted labels below k: label_enc [m][B][2nw] -> ([B][2nw], [B][2nw]).
    The histogram, then secure_argmax_batch over the k counts with l = bits(m).  Ties follow the argmax's rule: the lowest label wins."""
    from .selection import secure_argmax_batch

    planes, _ = _as_planes(label_enc)
    hist = secure_histogram_batch(planes, k, alice_paillier, bob_paillier, index_bits, kappa, draws)
    counts = hist.permute(1, 0, 2).contiguous()                                           # [B][k][2nw]
    top, label = secure_argmax_batch(counts, count_bits(planes.shape[0]), alice_paillier, alice_dgk, bob_paillier, bob_dgk, kappa)
    return label, top


def secure_groupby_count_batch(index_enc: torch.Tensor, k: int, alice_paillier: Paillier, bob_paillier: Paillier, index_bits: int | None = None,
                               kappa: int = 40, draws: OnehotDraws | None = None, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[#{b : i_b mod k == t}]], t < k, over the B rows of index_enc [B][2nw] -> [k][2nw]: the one-hot encoding with m = 1, then the sum
    over the rows of every plane."""
    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() != 2:
        raise ValueError("index_enc: expected [B][words]")
    planes = index_enc.unsqueeze(0)
    layout = _onehot_layout(planes, k, index_bits, kappa, alice_paillier)
    draws = draws if draws is not None else draw_onehot(planes.shape[1], layout, alice_paillier)
    onehot = onehot_batch(layout, planes, alice_paillier, bob_paillier, draws)[0]         # [k][B][2nw]
    return sum_rows_batch(onehot, alice_paillier, rho=rho)


def groupby_sum_layout(bits: int, B: int, signed: bool, kappa: int, paillier: Paillier) -> MulLayout:
    """The fit rule of secure_groupby_sum_batch and the layout of its multiplication: a group's sum of B values of `bits` bits takes
    bits + bits(B) bits (+ 1 when signed) and must stay below bits(N) - 1 (ValueError), so that it cannot wrap modulo N.  The one-hot
    operand is one bit wide, two when signed (the signed range of two bits holds 0 and 1)."""
    bits, B = int(bits), int(B)
    if bits < 1 or B < 1:
        raise ValueError("bits, B: expected positive")
    nbits = paillier.public_key.n.bit_length()
    need = bits + B.bit_length() + (1 if signed else 0)
    if need >= nbits - 1:
        raise ValueError(f"a sum of {B} values of {bits} bits ({need} bits) does not fit below a {nbits}-bit N")
    return MulLayout(kappa, bits, (2 if signed else 1,), signed, nbits)


def secure_groupby_sum_batch(value_enc: torch.Tensor, index_enc: torch.Tensor, k: int, bits: int, alice_paillier: Paillier,
                             bob_paillier: Paillier, signed: bool = False, index_bits: int | None = None, kappa: int = 40,
                             draws: OnehotDraws | None = None, mul_draws: MulDraws | None = None,
                             rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_{b : i_b mod k == t} v_b]], t < k, over B rows of encrypted values and indices: value_enc, index_enc [B][2nw] -> [k][2nw].
    Values: 0 <= v < 2^bits, or -2^(bits - 1) <= v < 2^(bits - 1) as residues modulo N when signed.  The one-hot encoding, one
    multiplication batch over the k B rows (v_b, onehot[t][b]), then the sum over the rows of every plane: two round trips.  ValueError,
    before any message is sent, when bits + bits(B) (+ 1 if signed) does not stay below bits(N) - 1."""
    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() != 2:
        raise ValueError("index_enc: expected [B][words]")
    if not isinstance(value_enc, torch.Tensor) or value_enc.shape != index_enc.shape:
        raise ValueError(f"value_enc: expected {tuple(index_enc.shape)} beside index_enc")
    B, w = index_enc.shape
    mul = groupby_sum_layout(bits, B, signed, kappa, alice_paillier)                      # both fit rules, before any launch
    planes = index_enc.unsqueeze(0)
    layout = _onehot_layout(planes, k, index_bits, kappa, alice_paillier)
    k = layout.k
    draws = draws if draws is not None else draw_onehot(B, layout, alice_paillier)
    onehot = onehot_batch(layout, planes, alice_paillier, bob_paillier, draws)[0]         # [k][B][2nw]
    x = value_enc.unsqueeze(0).expand(k, B, w).reshape(k * B, w).contiguous()
    y = onehot.reshape(k * B, w)
    mul_draws = mul_draws if mul_draws is not None else draw_mul(k * B, mul, alice_paillier)
    products = mul_batch(mul, x, y, alice_paillier, bob_paillier, mul_draws)[0]           # [k B][2nw]
    return sum_rows_batch(products.reshape(k, B, w), alice_paillier, rho=rho)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{histogram,majority,groupby_sum}_batch) ------------------
# Sequences of the existing sessions -- one-hot, multiplication, the argmax's rounds -- with Alice's local sums in between: no message
# id of their own and none changed.
async def alice_histogram(ini, index_enc, k, index_bits, kappa, draws, source, engine, generator, chunks):
    from .lookup import alice_onehot

    planes, _ = _as_planes(index_enc)
    onehot = await alice_onehot(ini, planes, k, index_bits, kappa, draws, source, engine, generator, chunks)     # [m][k][B][2nw]
    pai = ini.scheme_paillier
    m, kk, B, w = onehot.shape
    return pai.engine.paillier_sum_axis(pai.key, onehot.contiguous(), 1, m, kk * B).reshape(kk, B, w)


async def bob_histogram(kh, k, m, index_bits, kappa, draws, source, generator, count=None):
    from .lookup import bob_onehot

    return await bob_onehot(kh, k, m, index_bits, kappa, draws, source, generator, count)


async def alice_majority(ini, label_enc, k, index_bits, kappa, source, engine, generator, chunks):
    from .selection import alice_argext

    planes, _ = _as_planes(label_enc)
    if ini.l_maximum_bit_length < count_bits(planes.shape[0]):
        raise ValueError(f"l = {ini.l_maximum_bit_length}: counts of up to {planes.shape[0]} need {count_bits(planes.shape[0])} bits")
    hist = await alice_histogram(ini, planes, k, index_bits, kappa, None, source, engine, generator, chunks)
    top, label = await alice_argext(ini, hist.permute(1, 0, 2).contiguous(), kappa, source, engine, generator, chunks, want_max=True)
    return label, top


async def bob_majority(kh, k, m, index_bits, kappa, source, generator, count=None):
    from .selection import bob_rounds, index_bits as arg_index_bits, tournament_rounds

    if kh.l_maximum_bit_length < count_bits(m):
        raise ValueError(f"l = {kh.l_maximum_bit_length}: counts of up to {m} need {count_bits(m)} bits")
    await bob_histogram(kh, k, m, index_bits, kappa, None, source, generator, count)
    await bob_rounds(kh, tournament_rounds(int(k)), None, None, kappa, source, generator, (arg_index_bits(int(k)),))


async def alice_groupby_sum(ini, value_enc, index_enc, k, bits, signed, index_bits, kappa, source, engine, generator, chunks):
    from .lookup import alice_onehot
    from .multiplication import alice_multiply

    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() != 2:
        raise ValueError("index_enc: expected [B][words]")
    if not isinstance(value_enc, torch.Tensor) or value_enc.shape != index_enc.shape:
        raise ValueError(f"value_enc: expected {tuple(index_enc.shape)} beside index_enc")
    B, w = index_enc.shape
    if ini._scheme_paillier is not None:                   # the fit rule before any message where the key is known already
        groupby_sum_layout(bits, B, signed, kappa, ini._scheme_paillier)
    onehot = await alice_onehot(ini, index_enc, k, index_bits, kappa, None, source, engine, generator, chunks)  # [k][B][2nw]
    pai = ini.scheme_paillier
    mul = groupby_sum_layout(bits, B, signed, kappa, pai)
    kk = onehot.shape[0]
    x = value_enc.unsqueeze(0).expand(kk, B, w).reshape(kk * B, w).contiguous()
    products = await alice_multiply(ini, x, onehot.reshape(kk * B, w).contiguous(), bits, mul.wy[0], signed, kappa, None, source, engine,
                                    generator, chunks)
    return sum_rows_batch(products.reshape(kk, B, w), pai)


async def bob_groupby_sum(kh, k, bits, signed, index_bits, kappa, source, generator, count=None):
    from .lookup import bob_onehot
    from .multiplication import bob_multiply

    count = await bob_onehot(kh, k, 1, index_bits, kappa, None, source, generator, count)
    mul = groupby_sum_layout(bits, count, signed, kappa, kh.scheme_paillier)
    await bob_multiply(kh, bits, mul.wy[0], signed, kappa, None, source, generator, int(k) * count)

"""Sums and running sums of encrypted arrays along an axis, and the histogram, majority vote, group-by, cumulative distribution and
quantile that follow from them.

The sum of Paillier ciphertexts is their product modulo N^2.  sum_planes_batch / sum_rows_batch run it along one axis of an array with the
dedicated kernel k_prod_axis (sc_paillier_sum_axis, include/sc_amd.h): a tree of chains of at most 32 members, one Montgomery product per
member, one launch per level, no interaction and no randomness -- the result is a deterministic function of the inputs, so a caller who
hands it on passes `rho` to re-randomize it.

The two-party operations add no protocol of their own.  secure_histogram_batch is the one-hot encoding (lookup.py) summed over the indices
of a row, secure_majority_batch the argmax (selection.py) of that histogram, secure_groupby_count_batch / secure_groupby_sum_batch the
one-hot encoding (times the value: multiplication.py) summed over the rows.  Their draws are the one-hot's, the multiplication's and the
comparison's, in that order.

cumsum_planes_batch / cumsum_rows_batch are the running sums along the same two axes with the kernel k_scan_axis
(sc_paillier_cumsum_axis): two products per member, one launch when the array is wide enough across the axis, reduce-then-scan otherwise.
secure_cdf_batch is the histogram followed by the running sum over its bins, secure_quantile_batch counts the bins whose cumulative count
does not exceed the wanted rank with one comparison batch: the one-hot's draws, then the comparison's.
"""
from __future__ import annotations

import torch

from .lookup import OnehotDraws, _as_planes, _layout as _onehot_layout, draw_onehot, onehot_batch
from .multiplication import MulDraws, MulLayout, draw_mul, mul_batch
from .schemes import DGK, Paillier

MIN_CHUNK, MAX_CHUNK = 4, 32        # automatic chunk lengths of a level (axis_chunk in csrc/sc_axis_plan.h)


def _axis_chunk(total: int, resident_groups: int, forced: int) -> int:
    """The chunk length of a level of `total` members, as axis_chunk in csrc/sc_axis_plan.h: the shortest of 4 .. 32 members whose chains
    still fill `resident_groups` group slots (num_cu * 8 * 64 / G), or `forced` (2 .. 32, Engine.set_reduce_chunk) at every level."""
    return forced if forced else min(MAX_CHUNK, max(MIN_CHUNK, -(-total // resident_groups)))


def _plan_args(name: str, outer: int, K: int, inner: int, resident_groups: int, forced: int) -> tuple[int, int, int, int]:
    outer, K, inner, forced = int(outer), int(K), int(inner), int(forced)
    if K < 1 or outer < 1 or inner < 1 or resident_groups < 1:
        raise ValueError(f"{name}: expected positive sizes")
    if forced != 0 and not 2 <= forced <= MAX_CHUNK:
        raise ValueError(f"forced chunk {forced}: expected 0 or 2 .. {MAX_CHUNK}")
    return outer, K, inner, forced


def reduce_plan(outer: int, K: int, inner: int, resident_groups: int, forced: int = 0) -> list[tuple[int, int, int]]:
    """The levels (K, chunk, chains per output) of sc_modprod_axis' tree, as reduce_plan in csrc/sc_axis_plan.h computes them: a level
    cuts the K members of an output into ceil(K / chunk) chains and hands that many partials to the next level, until one is left.
    chunk: axis_chunk's, never more than K."""
    outer, K, inner, forced = _plan_args("reduce_plan", outer, K, inner, resident_groups, forced)
    levels = []
    while True:
        c = min(_axis_chunk(outer * K * inner, resident_groups, forced), K)
        nch = -(-K // c)
        levels.append((K, c, nch))
        if nch == 1:
            return levels
        K = nch


def scan_plan(outer: int, K: int, inner: int, resident_groups: int, forced: int = 0) -> list[tuple[str, int, int, int]]:
    """The launches (kind, K, chunk, chains) of sc_modscan_axis in order, as scan_plan in csrc/sc_axis_plan.h decides them.  Direct --
    one "scan" launch, one chain per (outer, inner) running the whole K -- when outer * inner chains fill `resident_groups` group slots
    (num_cu * 8 * 64 / G) by themselves or K is no longer than one chunk of axis_chunk's rule; otherwise blocked: a "totals" launch
    (k_prod_axis) over the ceil(K / chunk) - 1 full chunks that are followed by another, the launches of the scan of those totals by the
    same rule, and one seeded "scan" launch with a chain per chunk.  `forced` (2 .. 32, Engine.set_reduce_chunk) is the chunk length
    of every level and blocks every level longer than itself."""
    outer, K, inner, forced = _plan_args("scan_plan", outer, K, inner, resident_groups, forced)
    down, up = [], []
    while True:
        c = _axis_chunk(outer * K * inner, resident_groups, forced)
        if (not forced and outer * inner >= resident_groups) or K <= c:
            return down + [("scan", K, K, outer * inner)] + up[::-1]
        nch = -(-K // c)
        down.append(("totals", K, c, outer * (nch - 1) * inner))
        up.append(("scan", K, c, outer * nch * inner))
        K = nch - 1


def _rerandomize(out: torch.Tensor, paillier: Paillier, rho: torch.Tensor | None) -> torch.Tensor:
    if rho is None:
        return out
    flat = out.reshape(-1, out.shape[-1])
    return paillier.randomize_batch(flat, rho.reshape(flat.shape[0], -1).contiguous()).reshape(out.shape)


def _cipher_array(x_enc, min_dim: int, name: str) -> torch.Tensor:
    if not isinstance(x_enc, torch.Tensor) or x_enc.dim() < min_dim:
        raise ValueError(f"{name}: expected an array of at least {min_dim} axes, [...][words]")
    return x_enc.contiguous()


def _planes_geometry(x_enc) -> tuple[torch.Tensor, tuple[int, int, int]]:
    """x_enc [k][B][words], k >= 1, contiguous, and its geometry (outer, K, inner) = (1, k, B) along the planes."""
    x = _cipher_array(x_enc, 3, "x_enc")
    if x.dim() != 3 or x.shape[0] < 1:
        raise ValueError("x_enc: expected [k][B][words] with k >= 1")
    return x, (1, x.shape[0], x.shape[1])


def check_segment(B: int, segment: int | None) -> int:
    """The segment length of sum_rows_batch over B rows: B itself by default; ValueError unless 1 <= segment and segment divides B."""
    if segment is None:
        segment = B
    segment = int(segment)
    if segment < 1 or B % segment != 0:
        raise ValueError(f"segment = {segment}: expected a divisor of the {B} rows")
    return segment


def _rows_geometry(x_enc, segment: int | None) -> tuple[torch.Tensor, tuple[int, int, int]]:
    """x_enc [..., B][words], B >= 1, contiguous, and its geometry (planes * B / segment, segment, 1) along the rows."""
    x = _cipher_array(x_enc, 2, "x_enc")
    B, w = x.shape[-2], x.shape[-1]
    if B < 1:
        raise ValueError("x_enc: expected at least one row")
    seg = check_segment(B, segment)
    return x, (x.numel() // (seg * w), seg, 1)


def sum_planes_batch(x_enc: torch.Tensor, paillier: Paillier, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_j x[j][b]]] for x_enc [k][B][2nw] -> [B][2nw]: the sum over the planes, geometry (outer, K, inner) = (1, k, B).
    rho [B][nw] (optional) re-randomizes the result."""
    x, geometry = _planes_geometry(x_enc)
    return _rerandomize(paillier.engine.paillier_sum_axis(paillier.key, x, *geometry), paillier, rho)


def sum_rows_batch(x_enc: torch.Tensor, paillier: Paillier, segment: int | None = None, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_b x[..][b]]] over the rows of every plane of x_enc [..., B][2nw] -> [...][2nw]; with `segment` one total per run of `segment`
    consecutive rows -> [..., B / segment][2nw] (segment must divide B: ValueError).  Geometry (planes * B / segment, segment, 1).
    rho (one [nw] row per result, optional) re-randomizes the results."""
    x, geometry = _rows_geometry(x_enc, segment)
    out = paillier.engine.paillier_sum_axis(paillier.key, x, *geometry)
    shape = tuple(x.shape[:-2]) + (() if segment is None else (x.shape[-2] // geometry[1],)) + (x.shape[-1],)
    return _rerandomize(out.reshape(shape), paillier, rho)


def _cumsum(x: torch.Tensor, geometry: tuple[int, int, int], paillier: Paillier, exclusive: bool, rho: torch.Tensor | None) -> torch.Tensor:
    """The running sum of x along the middle axis of `geometry`, in the shape of x.  The exclusive one is the inclusive one a position
    later along the axis, the residue 1 (the unrandomized [[0]]) first."""
    out = paillier.engine.paillier_cumsum_axis(paillier.key, x, *geometry)
    if exclusive:
        v = out.reshape(*geometry, out.shape[-1])
        out = torch.empty_like(v)
        out[:, 1:] = v[:, :-1]
        out[:, 0] = 0
        out[:, 0, :, 0] = 1
    return _rerandomize(out.reshape(x.shape), paillier, rho)


def cumsum_planes_batch(x_enc: torch.Tensor, paillier: Paillier, exclusive: bool = False, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_{j' <= j} x[j'][b]]] for x_enc [k][B][2nw] -> [k][B][2nw]: the running sum over the planes, geometry (outer, K, inner) =
    (1, k, B).  exclusive: [[sum_{j' < j}]] instead, plane 0 the residue 1 (the unrandomized [[0]]).  The result is a deterministic
    function of the inputs: pass rho [k][B][nw] before handing it on; it re-randomizes every output."""
    return _cumsum(*_planes_geometry(x_enc), paillier, exclusive, rho)


def cumsum_rows_batch(x_enc: torch.Tensor, paillier: Paillier, segment: int | None = None, exclusive: bool = False,
                      rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[sum_{b' <= b} x[..][b']]] over the rows of every plane of x_enc [..., B][2nw] -> the same shape; with `segment` the running sum
    starts again every `segment` rows (segment must divide B: ValueError).  Geometry (planes * B / segment, segment, 1).  exclusive:
    [[sum_{b' < b}]] instead, the first row of every scan the residue 1 (the unrandomized [[0]]) -- the offsets of a group-by.  The
    result is a deterministic function of the inputs: pass rho (one [nw] row per output) before handing it on; it re-randomizes every
    output."""
    return _cumsum(*_rows_geometry(x_enc, segment), paillier, exclusive, rho)


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


# ---- cumulative distribution, quantile ---------------------------------------------------------------------------------------------
def secure_cdf_batch(index_enc: torch.Tensor, k: int, alice_paillier: Paillier, bob_paillier: Paillier, index_bits: int | None = None,
                     kappa: int = 40, draws: OnehotDraws | None = None, rho: torch.Tensor | None = None) -> torch.Tensor:
    """[[#{q : i_q mod k <= t}]], t < k, for B rows of m encrypted indices each: index_enc [m][B][2nw] -> [k][B][2nw].  The histogram
    (one round trip), then the running sum over its k bins; the last plane is [[m]].  rho [k][B][nw] re-randomizes every output."""
    hist = secure_histogram_batch(index_enc, k, alice_paillier, bob_paillier, index_bits, kappa, draws)
    return cumsum_planes_batch(hist, alice_paillier, rho=rho)


def check_rank(kth, m: int, B: int, words: int):
    """The rank argument of secure_quantile_batch over m values per row: a public integer 0 <= kth < m, or [B][words] encrypted ranks
    (returned as they are); ValueError otherwise, and when a count of up to m does not fit the comparison's 255 bits."""
    if count_bits(m) > 255:
        raise ValueError(f"m = {m}: counts of {count_bits(m)} bits exceed the comparison's 255")
    if isinstance(kth, torch.Tensor):
        if kth.dim() != 2 or tuple(kth.shape) != (B, words):
            raise ValueError(f"kth: expected an integer or [{B}][{words}] encrypted ranks")
        return kth.contiguous()
    if isinstance(kth, bool) or not isinstance(kth, int):
        raise ValueError(f"kth = {kth!r}: expected an integer or encrypted ranks")
    if not 0 <= kth < m:
        raise ValueError(f"kth = {kth}: expected 0 .. {m - 1}")
    return kth


def _rank_rows(kth, planes: int, B: int, paillier: Paillier) -> torch.Tensor:
    """[[kth]] for `planes` x B comparison rows, [planes * B][2nw]: the public rank unrandomized, the encrypted one repeated per plane."""
    engine, nw = paillier.engine, paillier.mod_n.nwords
    if isinstance(kth, torch.Tensor):
        return kth.unsqueeze(0).expand(planes, B, kth.shape[-1]).reshape(planes * B, -1).contiguous()
    return paillier.encrypt_raw_batch(engine.upload([kth] * (planes * B), nw))


def _zero_rows(B: int, paillier: Paillier) -> torch.Tensor:
    return paillier.encrypt_raw_batch(paillier.engine.upload([0] * B, paillier.mod_n.nwords))


def secure_quantile_batch(index_enc: torch.Tensor, k: int, kth, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                          index_bits: int | None = None, kappa: int = 40, draws: OnehotDraws | None = None, comparison_draws=None) -> torch.Tensor:
    """[[the bin of rank kth]] among the m binned values i_q mod k of every row (0 = the smallest, 0 <= kth < m, as secure_kth_batch counts):
    index_enc [m][B][2nw] -> [B][2nw].  kth: a public integer, or [B][2nw] encrypted ranks, one per row.  The cumulative distribution
    (secure_cdf_batch), then the answer #{t < k - 1 : cdf_t <= kth}: one comparison batch over (k - 1) B rows with l = bits(m) and the sum
    of its bits over the planes; the last plane of the distribution is m and is never compared, and k = 1 runs no comparison and returns
    [[0]].  ValueError, before any launch, for a public kth outside 0 .. m - 1, a kth that is neither an integer nor [B][2nw], and
    bits(m) > 255.  Draws: the one-hot's (`draws`), then the comparison's (`comparison_draws`, a batch.BatchDraws over (k - 1) B rows)."""
    from .batch import secure_comparison_batch
    from .selection import _comparison_draws

    planes, _ = _as_planes(index_enc)
    m, B, w = planes.shape
    kth = check_rank(kth, m, B, w)
    layout = _onehot_layout(planes, k, index_bits, kappa, alice_paillier)                 # the fit rule, before any launch
    cdf = secure_cdf_batch(planes, k, alice_paillier, bob_paillier, index_bits, kappa, draws)
    kk = layout.k
    if kk == 1:
        return _zero_rows(B, alice_paillier)
    l, rows = count_bits(m), (kk - 1) * B
    x = cdf[:kk - 1].reshape(rows, w).contiguous()
    y = _rank_rows(kth, kk - 1, B, alice_paillier)
    cd = comparison_draws if comparison_draws is not None else _comparison_draws(rows, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk)
    bits = secure_comparison_batch(x, y, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, cd)
    return sum_planes_batch(bits.reshape(kk - 1, B, w), alice_paillier)


def secure_histogram_median_batch(index_enc: torch.Tensor, k: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier,
                                  bob_dgk: DGK, index_bits: int | None = None, kappa: int = 40, draws: OnehotDraws | None = None,
                                  comparison_draws=None) -> torch.Tensor:
    """The lower median bin of every row: secure_quantile_batch with kth = (m - 1) // 2, as secure_median_batch chooses it."""
    planes, _ = _as_planes(index_enc)
    return secure_quantile_batch(planes, k, (planes.shape[0] - 1) // 2, alice_paillier, alice_dgk, bob_paillier, bob_dgk, index_bits, kappa,
                                 draws, comparison_draws)


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


def secure_groupby_mean_batch(value_enc: torch.Tensor, index_enc: torch.Tensor, k: int, bits: int, group_counts, alice_paillier: Paillier,
                              bob_paillier: Paillier, alice_dgk, bob_dgk, signed: bool = False, index_bits: int | None = None,
                              kappa: int = 40, draws: OnehotDraws | None = None, mul_draws: MulDraws | None = None,
                              div_draws=None) -> torch.Tensor:
    """[[floor(sum_{b : i_b mod k == t} v_b / n_t)]], t < k -> [k][2nw]: secure_groupby_sum_batch, then one division batch of k rows
    (division.py) by the PUBLIC group sizes n_t = group_counts[t] >= 1 (a list or CPU int64 tensor of [k]).  The counts are an input: a
    division by the ENCRYPTED counts of secure_groupby_count_batch is out of scope.  The division is told x_bits = bits + bits(B): an
    unsigned sum is below 2^x_bits, and a signed one lies in [-2^(x_bits - 1), 2^(x_bits - 1)), inside the division's signed range
    [-2^x_bits, 2^x_bits), so no further bit is added.  draws / mul_draws / div_draws (division.DivDraws for k rows) inject the three
    steps' randomness."""
    from .division import secure_divide_batch

    sums = secure_groupby_sum_batch(value_enc, index_enc, k, bits, alice_paillier, bob_paillier, signed, index_bits, kappa, draws, mul_draws)
    width = int(bits) + int(index_enc.shape[0]).bit_length()
    return secure_divide_batch(sums, group_counts, width, alice_paillier, bob_paillier, alice_dgk, bob_dgk, signed, kappa, div_draws)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{histogram,majority,groupby_sum,cdf,quantile}_batch) -----
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


async def alice_cdf(ini, index_enc, k, index_bits, kappa, draws, source, engine, generator, chunks):
    hist = await alice_histogram(ini, index_enc, k, index_bits, kappa, draws, source, engine, generator, chunks)
    return cumsum_planes_batch(hist, ini.scheme_paillier)


async def bob_cdf(kh, k, m, index_bits, kappa, draws, source, generator, count=None):
    return await bob_histogram(kh, k, m, index_bits, kappa, draws, source, generator, count)


async def alice_quantile(ini, index_enc, k, kth, index_bits, kappa, source, engine, generator, chunks):
    planes, _ = _as_planes(index_enc)
    m, B, w = planes.shape
    kth = check_rank(kth, m, B, w)
    if ini.l_maximum_bit_length < count_bits(m):
        raise ValueError(f"l = {ini.l_maximum_bit_length}: counts of up to {m} need {count_bits(m)} bits")
    cdf = await alice_cdf(ini, planes, k, index_bits, kappa, None, source, engine, generator, chunks)
    pai, kk = ini.scheme_paillier, cdf.shape[0]
    if kk == 1:
        return _zero_rows(B, pai)
    x = cdf[:kk - 1].reshape((kk - 1) * B, w).contiguous()
    bits = await ini.perform_secure_comparison_batch(x, _rank_rows(kth, kk - 1, B, pai), None, source, engine, generator)
    return sum_planes_batch(bits.reshape(kk - 1, B, w), pai)


async def bob_quantile(kh, k, m, index_bits, kappa, source, generator, count=None):
    if count_bits(m) > 255:
        raise ValueError(f"m = {m}: counts of {count_bits(m)} bits exceed the comparison's 255")
    if kh.l_maximum_bit_length < count_bits(m):
        raise ValueError(f"l = {kh.l_maximum_bit_length}: counts of up to {m} need {count_bits(m)} bits")
    await bob_histogram(kh, k, m, index_bits, kappa, None, source, generator, count)
    if int(k) > 1:
        await kh.perform_secure_comparison_batch(None, source, generator)

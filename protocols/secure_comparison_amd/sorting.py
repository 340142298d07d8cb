"""Batched secure sort and argsort over k encrypted values per row: an oblivious sorting network of compare-exchanges.

The network is Batcher's odd-even merge sort; its comparators do not depend on the data, so neither player learns more than k, B
and the column widths.  A compare-exchange of the operands F (compared first) and G is one comparison,
[[delta]] = [[F <= G]], and one selection (selection.py) with sigma = delta, base F_j and d_j = G_j - F_j + 2^w_j.  With T_j and
Bob's [[ab_j]] of that selection, [[S_j]] = [[delta (G_j - F_j)]] = [[ab_j]] T_j^-1, and with U_j = T_j [[ab_j]]:

    [[hi_j]] = [[F_j + S_j]] = [[F_j]] [[ab_j]]^2 U_j^-1        [[lo_j]] = [[G_j - S_j]] = [[G_j]] T_j^2 U_j^-1

so both outputs share one inversion (sc_select_finish_cx).  lo lands at F's position and hi at G's.  Ascending: F = the value at
i, G = the value at j of a comparator (i, j), i < j; descending: F = the value at j, G = the value at i.  Equal keys give delta = 1,
lo = F and hi = G: a comparator never exchanges equal keys, in either direction.  The sort is deterministic but not stable.

The m smallest (or largest) of k, one order statistic and the median run the same compare-exchange over a truncated network,
topk_network(k, m, only_last): the comparators the wanted outputs depend on, with a flag per output that says whether anything
reads it again; a dead output is handed the row past the buffer's end and is not written.  The sort is that path
with m = k, where topk_network returns batcher_network(k) with every flag true: schedule, steps, runner and player halves are one.
"""
from __future__ import annotations

import torch

from . import wire
from .batch import BatchDraws
from .exchange import no_chunks
from .flags import check_l
from .schemes import DGK, Paillier
from .selection import (MAX_FIELDS, SelectDraws, SelectLayout, _alice_compare, _alice_exchange, _bob_select, _compare, draw_select,
                        index_bits, select_mult, select_pack)

MAX_K = 1024        # values per row


# ---- the network and the schedule (pure Python: both players derive the same one) -----------------------------------------------
def batcher_network(k: int) -> list[list[tuple[int, int]]]:
    """Layers of Batcher's odd-even merge sort for k inputs, 1 <= k <= MAX_K: lists of disjoint comparators (i, j), i < j, that sort
    every row ascending when each puts the smaller value at i.  The power-of-two network for n = 2^ceil(log2 k), without the
    comparators that touch an index >= k (a padded position would hold +inf, so such a comparator leaves i as it is) and without
    the layers that end up empty."""
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k}: expected 1 <= k <= {MAX_K}")
    n = 1 << (k - 1).bit_length()
    layers = []
    p = 1
    while p < n:
        q = p
        while q >= 1:
            layer = [(i + j, i + j + q) for j in range(q % p, n - q, 2 * q) for i in range(min(q, n - j - q))
                     if (i + j) // (2 * p) == (i + j + q) // (2 * p) and i + j + q < k]
            if layer:
                layers.append(layer)
            q //= 2
        p *= 2
    return layers


# ---- the truncated network: the m smallest of k, or the m-th smallest alone ----------------------------------------
def _truncated_merges(k: int, m: int) -> list[tuple[int, int]] | None:
    """Candidate (A) in sequential order, or None when one block would span the whole padded row: Batcher-sort every block of
    m' = 2^ceil(log2 m) positions, then for stride = m', 2m', .. merge the blocks at a and b = a + stride into a -- the half-cleaner
    (a + i, b + m' - 1 - i) leaves the m' smallest of both in block a as a bitonic sequence, the bitonic merger sorts it.  A padded
    position (index >= k) holds +inf and every comparator puts the minimum at its lower index, so a comparator that touches one
    changes nothing and is left out, and so is the whole merge of a block b that starts at or past k."""
    mp = 1 << (m - 1).bit_length()
    n = 1 << (k - 1).bit_length()
    if mp >= n:
        return None
    block = [c for layer in batcher_network(mp) for c in layer] if mp > 1 else []
    seq = [(a + i, a + j) for a in range(0, k, mp) for i, j in block]
    stride = mp
    while stride < k:
        for a in range(0, k - stride, 2 * stride):                    # b >= k: block b is all +inf and block a stays as it is
            b = a + stride
            seq += [(a + i, b + mp - 1 - i) for i in range(mp)]
            q = mp // 2
            while q >= 1:
                seq += [(a + i, a + i + q) for i in range(mp) if (i // q) % 2 == 0]
                q //= 2
        stride *= 2
    return [(i, j) for i, j in seq if j < k]


def _prune(seq: list[tuple[int, int]], live: set[int]) -> list[tuple[int, int, bool, bool]]:
    """Backwards from the live outputs: a comparator with no live output goes, one with a live output makes both of its inputs live;
    the flags say which of its outputs is read again."""
    live = set(live)
    out = []
    for i, j in reversed(seq):
        ki, kj = i in live, j in live
        if ki or kj:
            out.append((i, j, ki, kj))
            live.add(i)
            live.add(j)
    out.reverse()
    return out


def _relayer(seq: list[tuple[int, int, bool, bool]], k: int) -> list[list[tuple[int, int, bool, bool]]]:
    """Every comparator into the earliest layer after the previous comparators of both of its positions, in sequential order."""
    depth = [0] * k
    layers: list[list[tuple[int, int, bool, bool]]] = []
    for c in seq:
        t = max(depth[c[0]], depth[c[1]])
        if t == len(layers):
            layers.append([])
        layers[t].append(c)
        depth[c[0]] = depth[c[1]] = t + 1
    return layers


def topk_network(k: int, m: int, only_last: bool = False) -> list[list[tuple[int, int, bool, bool]]]:
    """Layers of disjoint comparators (i, j, keep_i, keep_j), i < j, for 1 <= m <= k <= MAX_K: each puts the smaller value at i, and
    after the last layer the positions 0 .. m-1 hold the m smallest values in ascending order (only_last: position m-1 alone is
    guaranteed, the m-th smallest).  keep_i / keep_j say whether that output is read again, by a later comparator or as a result: a
    dead output need not be written.  A pure function of (k, m, only_last): the smaller of (A) the truncated merges and (B)
    batcher_network(k), each pruned backwards from the live outputs and packed into the earliest layers; (B) on a tie.  m = k without
    only_last prunes nothing: the layers are batcher_network(k)'s own, every flag true."""
    net = batcher_network(k)
    if not 1 <= int(m) <= k:
        raise ValueError(f"m = {m}: expected 1 <= m <= k = {k}")
    m = int(m)
    if m == k and not only_last:
        return [[(i, j, True, True) for i, j in layer] for layer in net]
    live = {m - 1} if only_last else set(range(m))
    best = _prune([c for layer in net for c in layer], live)
    merges = _truncated_merges(k, m)
    if merges is not None:
        cand = _prune(merges, live)
        if len(cand) < len(best):
            best = cand
    return _relayer(best, k)


# ---- the schedule (pure Python: both players derive the same one) -------------------------------------------------------------------
def _cut(layers: list, B: int, max_rows: int) -> list:
    """The schedule both players follow: per layer, (the layer, its sub-batches).  A layer's B * len(layer) comparisons are numbered
    t = c * B + b (comparator c, row b) and cut into [start, stop) ranges of at most max_rows; each range is one comparison and one
    compare-exchange selection, and live and dead outputs share it.  The one place that checks max_rows >= 1."""
    if int(max_rows) < 1:
        raise ValueError(f"max_rows = {max_rows}: expected >= 1")
    return [(layer, [(a, min(a + max_rows, B * len(layer))) for a in range(0, B * len(layer), max_rows)]) for layer in layers]


def _counts(layers: list, B: int, max_rows: int) -> list[int]:
    """The comparisons of every sub-batch, in order (what the key holder needs of the schedule)."""
    return [b - a for _, cuts in _cut(layers, B, max_rows) for a, b in cuts]


def sort_schedule(k: int, B: int, max_rows: int) -> list[tuple[list[tuple[int, int]], list[tuple[int, int]]]]:
    """The schedule of the sort: per layer of batcher_network(k), (its comparators (i, j), its sub-batches)."""
    return _cut(batcher_network(k), B, max_rows)


def schedule_counts(k: int, B: int, max_rows: int) -> list[int]:
    """topk_counts of the sort, m = k."""
    return topk_counts(k, k, False, B, max_rows)


def topk_schedule(k: int, m: int, only_last: bool, B: int, max_rows: int):
    """The schedule of topk_network(k, m, only_last): per layer, (its comparators (i, j, keep_i, keep_j), its sub-batches)."""
    return _cut(topk_network(k, m, only_last), B, max_rows)


def topk_counts(k: int, m: int, only_last: bool, B: int, max_rows: int) -> list[int]:
    """The comparisons of every sub-batch of topk_schedule, in order."""
    return _counts(topk_network(k, m, only_last), B, max_rows)


def _topk_steps(buf: torch.Tensor, B: int, k: int, m: int, only_last: bool, max_rows: int, largest: bool):
    """Yields (F [nf][count][2nw], G, lo rows, hi rows) per sub-batch of topk_schedule(k, m, only_last, B, max_rows); a sort passes
    m = k.  The rows are int64 [nf][count] flat rows of buf [nf][B k][2nw] seen as [nf B k][2nw].  F and G are gathered copies and
    a layer's comparators are disjoint, so the outputs of one sub-batch go straight into buf: no later sub-batch of the layer reads
    a row it writes.  A dead output's row is nf * B * k, the number of rows of buf: sc_select_finish_cx writes no row at or past
    out_rows, so the dead position keeps a ciphertext nothing reads again.  largest (the sort: descending): F is the value at j and
    G the one at i, so the larger value goes to i and keep_i belongs to hi."""
    nf, rows, _ = buf.shape
    dev = buf.device
    dead = nf * rows
    col = (torch.arange(nf, dtype=torch.int64, device=dev) * rows).unsqueeze(1)
    base = torch.arange(B, dtype=torch.int64, device=dev) * k
    for layer, cuts in topk_schedule(k, m, only_last, B, max_rows):
        c = torch.tensor(layer, dtype=torch.int64, device=dev)
        ri, rj = (c[:, 0:1] + base).reshape(-1), (c[:, 1:2] + base).reshape(-1)
        ki, kj = (c[:, 2:3].bool().expand(-1, B).reshape(-1), c[:, 3:4].bool().expand(-1, B).reshape(-1))
        (fr, fk), (gr, gk) = ((rj, kj), (ri, ki)) if largest else ((ri, ki), (rj, kj))
        for a, b in cuts:
            f_rows, g_rows = fr[a:b], gr[a:b]
            lo = torch.where(fk[a:b], col + f_rows, dead).contiguous()
            hi = torch.where(gk[a:b], col + g_rows, dead).contiguous()
            yield buf.index_select(1, f_rows), buf.index_select(1, g_rows), lo, hi


# ---- the compare-exchange ----------------------------------------------------------------------------------------------------------
def cx_differences(paillier: Paillier, layout: SelectLayout, f_enc: torch.Tensor, g_enc: torch.Tensor, d_key: torch.Tensor) -> torch.Tensor:
    """[[d_j]] = [[G_j - F_j + 2^w_j]] [nf][count][2nw]: the key column's is the comparison's own [[d]]; the other columns' are
    [[G_j]] [[F_j]]^-1 (1 + 2^w_j N), their inverses from one batched inversion and the products from one launch
    (sc_initiator_cx_differences)."""
    return paillier.engine.initiator_cx_differences(paillier.key, layout.kappa, layout.widths, f_enc.contiguous(), g_enc.contiguous(),
                                                    d_key.contiguous())


def cx_finish(layout: SelectLayout, delta_enc: torch.Tensor, d_enc: torch.Tensor, f_enc: torch.Tensor, g_enc: torch.Tensor,
              products: torch.Tensor, plain, draws: SelectDraws, paillier: Paillier, out: torch.Tensor | None = None,
              lo_index: torch.Tensor | None = None, hi_index: torch.Tensor | None = None) -> torch.Tensor:
    """Alice's end of a compare-exchange (sc_initiator_cx_finish): T_j as in select_finish, U_j = T_j [[ab_j]] (one product), one
    inversion of U, then sc_select_finish_cx's launch.  Without index rows the result is [2][nf][count][2nw] = (lo, hi); with them, lo /
    hi of column j, item i go to row lo_index[j][i] / hi_index[j][i] of `out` seen as rows of 2nw words."""
    et, rab = plain
    return paillier.engine.initiator_cx_finish(paillier.key, layout.kappa, layout.widths, delta_enc, d_enc.contiguous(), f_enc.contiguous(),
                                               g_enc.contiguous(), products.contiguous(), draws.r_a, et, rab, lo_index, hi_index, out)


def _cx_batch(layout, l, f, g, ap, ad, bp, bd, draws=None, select_draws=None, out=None, lo_index=None, hi_index=None):
    """Both players' halves of one compare-exchange batch in one process."""
    delta, d_key = _compare(f[0], g[0], l, ap, ad, bp, bd, draws)
    d = cx_differences(ap, layout, f, g, d_key)
    sd = select_draws if select_draws is not None else draw_select(f.shape[1], layout, ap)
    P, plain = select_pack(layout, delta, d, sd, ap)
    products = select_mult(layout, P, bp, sd.rho_products)
    return cx_finish(layout, delta, d, f, g, products, plain, sd, ap, out, lo_index, hi_index)


def secure_compare_exchange_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK,
                                  bob_paillier: Paillier, bob_dgk: DGK, draws: BatchDraws | None = None,
                                  select_draws: SelectDraws | None = None, kappa: int = 40):
    """([[min(x, y)]], [[max(x, y)]]) for B pairs [B][2nw]: one comparison and one selection for both (on ties min = x, max = y)."""
    check_l(l)
    layout = SelectLayout(l, kappa, (), alice_paillier.public_key.n.bit_length())
    out = _cx_batch(layout, l, x_enc.unsqueeze(0), y_enc.unsqueeze(0), alice_paillier, alice_dgk, bob_paillier, bob_dgk, draws,
                    select_draws)
    return out[0, 0], out[1, 0]


# ---- the sort, top-m and the k-th order statistic in one process: one path, the sort is m = k ---------------------------------------
def _sort_layout(l, k, payload_bits, return_indices, kappa, paillier) -> SelectLayout:
    """The layout of the key column, the payload columns and -- return_indices -- the index column of k values per row."""
    widths = tuple(int(b) for b in payload_bits) + ((index_bits(k),) if return_indices else ())
    if 1 + len(widths) > MAX_FIELDS:
        raise ValueError(f"{1 + len(widths)} columns (key, payload, index): at most {MAX_FIELDS}")
    return SelectLayout(l, kappa, widths, paillier.public_key.n.bit_length())


def _start(v_enc, m, l, ap, payload, payload_bits, return_indices, kappa, max_rows):
    """Every check that comes before an upload or a launch; returns (layout, B, k, m).  m None is the sort: m = k."""
    check_l(l)
    _cut((), 0, max_rows)                                                # max_rows >= 1
    if not isinstance(v_enc, torch.Tensor) or v_enc.dim() != 3:
        raise ValueError("v_enc: expected [B][k][2nw]")
    B, k, words = v_enc.shape
    nw2 = ap.mod_n2.nwords
    if words != nw2:
        raise ValueError(f"v_enc: {words} words per ciphertext, expected {nw2}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k}: expected 1 <= k <= {MAX_K}")
    payload_bits = tuple(int(b) for b in payload_bits)
    if payload is None:
        if payload_bits:
            raise ValueError("payload_bits given without payload columns")
    elif not isinstance(payload, torch.Tensor) or payload.dim() != 4 or tuple(payload.shape[1:]) != (B, k, nw2):
        raise ValueError(f"payload: expected [np][{B}][{k}][{nw2}]")
    elif payload.shape[0] != len(payload_bits):
        raise ValueError(f"payload: {payload.shape[0]} columns, {len(payload_bits)} widths in payload_bits")
    layout = _sort_layout(l, k, payload_bits, return_indices, kappa, ap)
    if m is None:
        m = k
    elif isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= k:
        raise ValueError(f"m = {m}: expected an integer, 1 <= m <= k = {k}")
    return layout, B, k, int(m)


def _sort_buffer(v_enc, payload, return_indices, ap, B, k):
    """The columns [nf][B k][2nw]: key, payload, and the index column as trivial encryptions 1 + iN of each row's positions."""
    nw2 = ap.mod_n2.nwords
    cols = [v_enc.reshape(B * k, nw2)]
    if payload is not None:
        cols += [payload[c].reshape(B * k, nw2) for c in range(payload.shape[0])]
    if return_indices:
        pos = (torch.arange(B * k, dtype=torch.int64, device=ap.engine.device) % k).to(torch.int32).unsqueeze(1).contiguous()
        cols.append(ap.encrypt_raw_batch(pos))
    return torch.stack(cols).contiguous()


def _result(buf, payload, return_indices, B, k, m, only_last):
    """The first m positions of every row of the columns of buf, or -- only_last -- position m - 1 alone.  With m = k these are
    buf's own rows, anything less is a copy."""
    nw2 = buf.shape[-1]
    cut = (lambda t: t[..., m - 1, :].contiguous()) if only_last else (lambda t: t[..., :m, :].contiguous())
    pay = None if payload is None else cut(buf[1:1 + payload.shape[0]].reshape(payload.shape[0], B, k, nw2))
    idx = cut(buf[-1].reshape(B, k, nw2)) if return_indices else None
    return cut(buf[0].reshape(B, k, nw2)), pay, idx


def _topk_buffer(v_enc, m, only_last, l, ap, ad, bp, bd, payload, payload_bits, largest, return_indices, kappa, max_rows):
    """The checks and the network over the columns [nf][B k][2nw] in place; returns that buffer: the results sit in the first m
    positions of every row, every other position holds whatever its last live output -- or the input -- left there."""
    layout, B, k, m = _start(v_enc, m, l, ap, payload, payload_bits, return_indices, kappa, max_rows)
    buf = _sort_buffer(v_enc, payload, return_indices, ap, B, k)
    out = buf.reshape(-1, buf.shape[-1])
    for f, g, lo, hi in _topk_steps(buf, B, k, m, only_last, int(max_rows), largest):
        _cx_batch(layout, l, f, g, ap, ad, bp, bd, out=out, lo_index=lo, hi_index=hi)
    return buf


def _topk_run(v_enc, m, only_last, l, ap, ad, bp, bd, payload, payload_bits, largest, return_indices, kappa, max_rows):
    buf = _topk_buffer(v_enc, m, only_last, l, ap, ad, bp, bd, payload, payload_bits, largest, return_indices, kappa, max_rows)
    B, k = v_enc.shape[:2]
    return _result(buf, payload, return_indices, B, k, k if m is None else int(m), only_last)


def secure_sort_batch(v_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                      payload: torch.Tensor | None = None, payload_bits=(), descending: bool = False, return_indices: bool = False,
                      kappa: int = 40, max_rows: int = 65536):
    """Sort k values per row, v_enc [B][k][2nw] (0 <= v < 2^l): (sorted [B][k][2nw], payload [np][B][k][2nw] or None, indices
    [B][k][2nw] or None).  Payload columns (payload_bits[c] bits wide) and the original positions (return_indices) travel with
    their key.  Every layer of the network is cut into sub-batches of at most max_rows comparisons, each one comparison and one
    compare-exchange selection.  Equal keys are never exchanged; the sort is not stable.  The path is secure_topk_batch's with
    m = k: topk_network(k, k) is batcher_network(k) with every output live."""
    return _topk_run(v_enc, None, False, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, payload, payload_bits, descending,
                     return_indices, kappa, max_rows)


def secure_topk_batch(v_enc: torch.Tensor, m: int, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                      payload: torch.Tensor | None = None, payload_bits=(), largest: bool = False, return_indices: bool = False,
                      kappa: int = 40, max_rows: int = 65536):
    """The m smallest of k values per row in ascending order, v_enc [B][k][2nw] (0 <= v < 2^l), 1 <= m <= k: (values [B][m][2nw],
    payload [np][B][m][2nw] or None, indices [B][m][2nw] or None); largest: the m largest, largest first.  Payload columns and the
    original positions travel with their key as in secure_sort_batch.  The network is topk_network(k, m): only the comparators the
    m outputs depend on, and an output nothing reads again is not written.  Equal keys are never exchanged, so which of several
    equal keys lands among the m -- and with it whose payload and index -- is fixed by the network, not by position: every key
    returned is right, the choice among equals is deterministic but not the lowest index.  Not stable."""
    return _topk_run(v_enc, m, False, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, payload, payload_bits, largest, return_indices,
                     kappa, max_rows)


def secure_kth_batch(v_enc: torch.Tensor, kth: int, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier,
                     bob_dgk: DGK, payload: torch.Tensor | None = None, payload_bits=(), largest: bool = False,
                     return_indices: bool = False, kappa: int = 40, max_rows: int = 65536):
    """The value of rank kth (0 = the smallest; largest: 0 = the largest) of every row, 0 <= kth < k: (value [B][2nw], payload
    [np][B][2nw] or None, index [B][2nw] or None) from topk_network(k, kth + 1, only_last=True).  Ties as in secure_topk_batch."""
    if isinstance(kth, bool) or int(kth) != kth:
        raise ValueError(f"kth = {kth}: expected an integer")
    return _topk_run(v_enc, int(kth) + 1, True, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, payload, payload_bits, largest,
                     return_indices, kappa, max_rows)


def secure_median_batch(v_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                        payload: torch.Tensor | None = None, payload_bits=(), return_indices: bool = False, kappa: int = 40,
                        max_rows: int = 65536):
    """The lower median of every row: secure_kth_batch with kth = (k - 1) // 2."""
    k = v_enc.shape[1] if isinstance(v_enc, torch.Tensor) and v_enc.dim() == 3 else 1     # a bad v_enc is refused by the checks below
    return secure_kth_batch(v_enc, max(k - 1, 0) // 2, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, payload, payload_bits, False,
                            return_indices, kappa, max_rows)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{sort,topk}_batch) -----------------------------------
# An opening message tells the key holder what he cannot derive, B; he refuses a header that differs from his own arguments in anything
# else and derives the schedule from it.  Sub-batch i is then the unchanged comparison session and one selection exchange under the tag
# `session_{sid}_{word}_{i}`, word = `sort` or `topk`: the key holder's work does not depend on which outputs are live.
# The header `{word}_0_session_{sid}` is int32: the word's own fields -- k for `sort`; k, m, only_last for `topk` -- then B, max_rows,
# kappa and the column widths.  The callers below pass in the word and what differs.
async def _alice_half(ini, word, v_enc, m, only_last, payload, payload_bits, flip, return_indices, kappa, source, engine, generator,
                      chunks, max_rows):
    """The initiator's half of `word`, in place in the columns' buffer.  m None: the sort, m = k, whose header has k alone."""
    no_chunks(chunks)
    if not isinstance(v_enc, torch.Tensor) or v_enc.dim() != 3:
        raise ValueError("v_enc: expected [B][k][2nw]")
    if not 1 <= int(max_rows) < 1 << 31:
        raise ValueError(f"max_rows = {max_rows}: expected 1 <= max_rows < 2^31")
    sid = await ini._open_batch_session(v_enc[:, 0], v_enc[:, 0], engine)
    pai, sort = ini.scheme_paillier, m is None
    layout, B, k, m = _start(v_enc, m, ini.l_maximum_bit_length, pai, payload, payload_bits, return_indices, kappa, max_rows)
    fields = [k] if sort else [k, m, int(only_last)]
    head = torch.tensor([*fields, B, int(max_rows), *layout.header], dtype=torch.int32, device=v_enc.device)
    await ini.communicator.send(ini.other_party, wire.outgoing(ini.communicator, head), msg_id=f"{word}_0_session_{sid}")
    buf = _sort_buffer(v_enc, payload, return_indices, pai, B, k)
    out = buf.reshape(-1, buf.shape[-1])
    for i, (f, g, lo, hi) in enumerate(_topk_steps(buf, B, k, m, only_last, int(max_rows), flip)):
        tag = f"session_{sid}_{word}_{i}"
        delta, d_key = await _alice_compare(ini, tag, f[0], g[0], None, source, generator)
        d = cx_differences(pai, layout, f, g, d_key)
        products, plain, sd = await _alice_exchange(ini, tag, layout, delta, d, None, source, generator)
        cx_finish(layout, delta, d, f, g, products, plain, sd, pai, out, lo, hi)
    return _result(buf, payload, return_indices, B, k, m, only_last)


async def _bob_half(kh, sid, word, fields, layers, payload_bits, return_indices, kappa, source, generator, max_rows):
    """The key holder's half of `word` over the network `layers`, after he opened session sid.  fields: his own header fields by name,
    k first.  He refuses, in this order, a malformed header, one that announces something else than his arguments and a negative B,
    and then every sub-batch of another size than the schedule's."""
    pai, n = kh.scheme_paillier, len(fields)
    layout = _sort_layout(kh.l_maximum_bit_length, fields["k"], payload_bits, return_indices, kappa, pai)
    (head,) = wire.incoming(await kh.communicator.recv(kh.other_party, msg_id=f"{word}_0_session_{sid}"), pai.engine.device, expect=1)
    if not isinstance(head, torch.Tensor) or head.dim() != 1 or not n + 4 <= head.shape[0] <= n + 3 + MAX_FIELDS:
        raise ValueError(f"{word}: malformed header")
    theirs = [int(v) for v in head.cpu().tolist()]
    B = theirs.pop(n)
    mine = [*fields.values(), int(max_rows), *layout.header]
    if theirs != mine:
        raise ValueError(f"{word}: the initiator announces {', '.join(fields)}, max_rows, kappa and widths {theirs}, "
                         f"this key holder expects {mine}")
    if B < 0:
        raise ValueError(f"{word}: the initiator announces B = {B}")
    for i, count in enumerate(_counts(layers, B, int(max_rows))):
        tag = f"session_{sid}_{word}_{i}"
        got = await kh._batch_session(tag, None, None, source, generator)
        if got != count:
            raise ValueError(f"{word}: sub-batch {i} carries {got} comparisons, the schedule has {count}")
        await _bob_select(kh, tag, layout, count, None, source, generator)


async def alice_sort(ini, v_enc, payload, payload_bits, descending, return_indices, kappa, source, engine, generator, chunks, max_rows):
    return await _alice_half(ini, "sort", v_enc, None, False, payload, payload_bits, descending, return_indices, kappa, source, engine,
                             generator, chunks, max_rows)


async def bob_sort(kh, k, payload_bits, return_indices, kappa, source, generator, max_rows):
    sid = await kh._open_batch_session()
    await _bob_half(kh, sid, "sort", {"k": k}, topk_network(k, k), payload_bits, return_indices, kappa, source, generator, max_rows)


async def alice_topk(ini, v_enc, m, payload, payload_bits, largest, return_indices, kappa, source, engine, generator, chunks, max_rows,
                     only_last):
    return await _alice_half(ini, "topk", v_enc, m, bool(only_last), payload, payload_bits, largest, return_indices, kappa, source, engine,
                             generator, chunks, max_rows)


async def bob_topk(kh, k, m, payload_bits, return_indices, kappa, only_last, source, generator, max_rows):
    sid = await kh._open_batch_session()
    layers = topk_network(k, m, bool(only_last))                         # k and m in range
    await _bob_half(kh, sid, "topk", {"k": k, "m": int(m), "only_last": int(bool(only_last))}, layers, payload_bits, return_indices, kappa,
                    source, generator, max_rows)

"""Batched secure sort and argsort over k encrypted values per row: an oblivious sorting network of compare-exchanges.

The network is Batcher's odd-even merge sort; its comparators do not depend on the data, so neither player learns more than k, B
and the column widths.  A compare-exchange of the operands F (compared first) and G is one comparison,
[[delta]] = [[F <= G]], and one selection (selection.py) with sigma = delta, base F_j and d_j = G_j - F_j + 2^w_j.  With T_j and
Bob's [[ab_j]] of that selection, [[S_j]] = [[delta (G_j - F_j)]] = [[ab_j]] T_j^-1, and with U_j = T_j [[ab_j]]:

    [[hi_j]] = [[F_j + S_j]] = [[F_j]] [[ab_j]]^2 U_j^-1        [[lo_j]] = [[G_j - S_j]] = [[G_j]] T_j^2 U_j^-1

so both outputs share one inversion (sc_select_finish_cx).  lo lands at F's position and hi at G's.  Ascending: F = the value at
i, G = the value at j of a comparator (i, j), i < j; descending: F = the value at j, G = the value at i.  Equal keys give delta = 1,
lo = F and hi = G: a comparator never exchanges equal keys, in either direction.  The sort is deterministic but not stable.
"""
from __future__ import annotations

import torch

from .batch import BatchDraws
from .flags import check_l
from .schemes import DGK, Paillier
from .selection import (MAX_FIELDS, SelectDraws, SelectLayout, _alice_compare, _alice_exchange, _bob_select, _compare, _no_chunks,
                        draw_select, index_bits, select_mult, select_pack)

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


def sort_schedule(k: int, B: int, max_rows: int) -> list[tuple[list[tuple[int, int]], list[tuple[int, int]]]]:
    """The schedule both players follow: per layer, (its comparators, its sub-batches).  A layer's B * len(layer) comparisons are
    numbered t = c * B + b (comparator c, row b) and cut into [start, stop) ranges of at most max_rows; each range is one comparison
    and one compare-exchange selection."""
    if int(max_rows) < 1:
        raise ValueError(f"max_rows = {max_rows}: expected >= 1")
    out = []
    for layer in batcher_network(k):
        total = B * len(layer)
        out.append((layer, [(a, min(a + max_rows, total)) for a in range(0, total, max_rows)]))
    return out


def schedule_counts(k: int, B: int, max_rows: int) -> list[int]:
    """The comparisons of every sub-batch, in order (what the key holder needs of the schedule)."""
    return [b - a for _, cuts in sort_schedule(k, B, max_rows) for a, b in cuts]


def _sort_steps(buf: torch.Tensor, B: int, k: int, max_rows: int, descending: bool):
    """Yields (F [nf][count][2nw], G, lo rows, hi rows) per sub-batch of the schedule; the rows are int64 [nf][count] flat rows of
    buf [nf][B k][2nw] seen as [nf B k][2nw].  F and G are gathered copies and a layer's comparators are disjoint, so the outputs of
    one sub-batch go straight into buf: no later sub-batch of the layer reads a row it writes."""
    nf, rows, _ = buf.shape
    dev = buf.device
    col = (torch.arange(nf, dtype=torch.int64, device=dev) * rows).unsqueeze(1)
    base = torch.arange(B, dtype=torch.int64, device=dev) * k
    for layer, cuts in sort_schedule(k, B, max_rows):
        ij = torch.tensor(layer, dtype=torch.int64, device=dev)
        ri, rj = (ij[:, 0:1] + base).reshape(-1), (ij[:, 1:2] + base).reshape(-1)
        fr, gr = (rj, ri) if descending else (ri, rj)
        for a, b in cuts:
            f_rows, g_rows = fr[a:b], gr[a:b]
            yield (buf.index_select(1, f_rows), buf.index_select(1, g_rows), (col + f_rows).contiguous(), (col + g_rows).contiguous())


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


# ---- the sort in one process -------------------------------------------------------------------------------------------------------
def _sort_start(v_enc, l, ap, payload, payload_bits, return_indices, kappa, max_rows):
    """Every check that comes before an upload or a launch; returns (layout, B, k)."""
    check_l(l)
    if int(max_rows) < 1:
        raise ValueError(f"max_rows = {max_rows}: expected >= 1")
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
    widths = payload_bits + ((index_bits(k),) if return_indices else ())
    if 1 + len(widths) > MAX_FIELDS:
        raise ValueError(f"{1 + len(widths)} columns (key, payload, index): at most {MAX_FIELDS}")
    return SelectLayout(l, kappa, widths, ap.public_key.n.bit_length()), B, k


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


def _sort_result(buf, payload, return_indices, B, k):
    nw2 = buf.shape[-1]
    pay = None if payload is None else buf[1:1 + payload.shape[0]].reshape(payload.shape[0], B, k, nw2)
    idx = buf[-1].reshape(B, k, nw2) if return_indices else None
    return buf[0].reshape(B, k, nw2), pay, idx


def secure_sort_batch(v_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                      payload: torch.Tensor | None = None, payload_bits=(), descending: bool = False, return_indices: bool = False,
                      kappa: int = 40, max_rows: int = 65536):
    """Sort k values per row, v_enc [B][k][2nw] (0 <= v < 2^l): (sorted [B][k][2nw], payload [np][B][k][2nw] or None, indices
    [B][k][2nw] or None).  Payload columns (payload_bits[c] bits wide) and the original positions (return_indices) travel with
    their key.  Every layer of the network is cut into sub-batches of at most max_rows comparisons, each one comparison and one
    compare-exchange selection.  Equal keys are never exchanged; the sort is not stable."""
    ap = alice_paillier
    layout, B, k = _sort_start(v_enc, l, ap, payload, payload_bits, return_indices, kappa, max_rows)
    buf = _sort_buffer(v_enc, payload, return_indices, ap, B, k)
    out = buf.reshape(-1, buf.shape[-1])
    for f, g, lo, hi in _sort_steps(buf, B, k, int(max_rows), descending):
        _cx_batch(layout, l, f, g, ap, alice_dgk, bob_paillier, bob_dgk, out=out, lo_index=lo, hi_index=hi)
    return _sort_result(buf, payload, return_indices, B, k)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_sort_batch) -----------------------------------------
# `sort_0_session_{sid}` (int32: k, B, max_rows, kappa, the column widths) opens the sort; the key holder refuses a header that
# differs from his own arguments and derives the schedule from it.  Sub-batch i is the unchanged comparison session and one selection
# exchange under the tag `session_{sid}_sort_{i}`.
async def alice_sort(ini, v_enc, payload, payload_bits, descending, return_indices, kappa, source, engine, generator, chunks, max_rows):
    from . import wire

    _no_chunks(chunks)
    if not isinstance(v_enc, torch.Tensor) or v_enc.dim() != 3:
        raise ValueError("v_enc: expected [B][k][2nw]")
    if not 1 <= int(max_rows) < 1 << 31:
        raise ValueError(f"max_rows = {max_rows}: expected 1 <= max_rows < 2^31")
    sid = await ini._open_batch_session(v_enc[:, 0], v_enc[:, 0], engine)
    pai, l = ini.scheme_paillier, ini.l_maximum_bit_length
    layout, B, k = _sort_start(v_enc, l, pai, payload, payload_bits, return_indices, kappa, max_rows)
    head = torch.tensor([k, B, int(max_rows), layout.kappa, *layout.widths], dtype=torch.int32, device=v_enc.device)
    await ini.communicator.send(ini.other_party, wire.outgoing(ini.communicator, head), msg_id=f"sort_0_session_{sid}")
    buf = _sort_buffer(v_enc, payload, return_indices, pai, B, k)
    out = buf.reshape(-1, buf.shape[-1])
    for i, (f, g, lo, hi) in enumerate(_sort_steps(buf, B, k, int(max_rows), descending)):
        tag = f"session_{sid}_sort_{i}"
        delta, d_key = await _alice_compare(ini, tag, f[0], g[0], None, source, generator)
        d = cx_differences(pai, layout, f, g, d_key)
        products, plain, sd = await _alice_exchange(ini, tag, layout, delta, d, None, source, generator)
        cx_finish(layout, delta, d, f, g, products, plain, sd, pai, out, lo, hi)
    return _sort_result(buf, payload, return_indices, B, k)


async def bob_sort(kh, k, payload_bits, return_indices, kappa, source, generator, max_rows):
    from . import wire

    sid = await kh._open_batch_session()
    comm, pai, l = kh.communicator, kh.scheme_paillier, kh.l_maximum_bit_length
    batcher_network(k)                                                   # k in range
    widths = tuple(int(b) for b in payload_bits) + ((index_bits(k),) if return_indices else ())
    if 1 + len(widths) > MAX_FIELDS:
        raise ValueError(f"{1 + len(widths)} columns (key, payload, index): at most {MAX_FIELDS}")
    layout = SelectLayout(l, kappa, widths, pai.public_key.n.bit_length())
    (head,) = wire.incoming(await comm.recv(kh.other_party, msg_id=f"sort_0_session_{sid}"), pai.engine.device, expect=1)
    if not isinstance(head, torch.Tensor) or head.dim() != 1 or not 5 <= head.shape[0] <= 4 + MAX_FIELDS:
        raise ValueError("sort: malformed header")
    hk, B, mr, *rest = [int(v) for v in head.cpu().tolist()]
    mine = [k, int(max_rows), layout.kappa, *layout.widths]
    if [hk, mr, *rest] != mine:
        raise ValueError(f"sort: the initiator announces k, max_rows, kappa and widths {[hk, mr, *rest]}, this key holder expects {mine}")
    if B < 0:
        raise ValueError(f"sort: the initiator announces B = {B}")
    for i, count in enumerate(schedule_counts(k, B, mr)):
        tag = f"session_{sid}_sort_{i}"
        got = await kh._batch_session(tag, None, None, source, generator)
        if got != count:
            raise ValueError(f"sort: sub-batch {i} carries {got} comparisons, the schedule has {count}")
        await _bob_select(kh, tag, layout, count, None, source, generator)

"""The families chained as the examples and the README chain them, on the GPU: one family's output is the next one's
input -- unrandomized deterministic residues, plaintexts a previous stage produced, permuted and reshaped arrays, and the widths every
stage must declare for what the stage before it can produce.  The reference is tests/_pipeline_model.py on plain integers; it follows
the networks through the existing models, so rows with equal keys at a cut are checked like every other row.

Every chain decrypts every intermediate on all rows and names the stage and the first wrong row when one differs, checks the documented
shape of every intermediate, compares every array it handed to the library with a clone taken before the call, and runs once with the
outputs handed on as they are ("handed-on": no rho, no randomize_batch) and once re-randomized between the stages ("rerandomized").
Keys: the golden 1024-bit Paillier key and the 1024-bit DGK key for l = 16."""
import asyncio
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_model as PM  # noqa: E402
import test_gpu_aggregate as A  # noqa: E402
from test_gpu_aggregate import world  # noqa: E402,F401  (fixture)
from test_gpu_select import _two_players  # noqa: E402

pytestmark = pytest.mark.gpu

B = PM.B
MODES = ("handed-on", "rerandomized")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _stage(chain, stage, got, want):
    at = PM.first_diff(got, want)
    if at is not None:
        pair = f"got {got[at]}, expected {want[at]}" if at < min(len(got), len(want)) else f"{len(got)} values, expected {len(want)}"
        raise AssertionError(f"{chain}: stage '{stage}': first wrong row {at} of {len(want)}: {pair}")


def _shape(chain, stage, t, *dims):
    assert tuple(t.shape[:-1]) == dims, f"{chain}: stage '{stage}': shape {tuple(t.shape)}, documented [{']['.join(map(str, dims))}][2nw]"


def _flat(rows):
    return [v for r in rows for v in r]


class _Inputs:
    """Every array handed to the library, with the clone taken before the call."""

    def __init__(self, chain):
        self.chain, self.items = chain, []

    def __call__(self, name, t):
        self.items.append((name, t, t.clone()))
        return t

    def unchanged(self):
        for name, t, clone in self.items:
            assert torch.equal(t, clone), f"{self.chain}: the input '{name}' was modified"


def _rho(w, rng, *shape):
    engine, sk, ap = w[0], w[1], w[2]
    count = 1
    for s in shape:
        count *= s
    return engine.upload([rng.randrange(1, sk.n) for _ in range(count)], ap.mod_n.nwords).reshape(*shape, -1)


def _hand(w, rng, mode):
    """What passes an output on to the next stage: itself, or a fresh randomization of every ciphertext in it."""
    if mode == "handed-on":
        return lambda t: t
    ap = w[2]

    def fresh(t):
        flat = t.reshape(-1, t.shape[-1]).contiguous()
        return ap.randomize_batch(flat, _rho(w, rng, flat.shape[0])).reshape(t.shape)

    return fresh


def _offset(ap, c, shift):
    """[[v + shift]] for every ciphertext of c: the public offset as the unrandomized [[shift]]."""
    flat = c.reshape(-1, c.shape[-1]).contiguous()
    plus = ap.encrypt_raw_batch(ap.engine.upload([shift] * flat.shape[0], ap.mod_n.nwords))
    return ap.add_batch(flat, plus).reshape(c.shape)


def _knn_inputs(w, rng, K, keep):
    rows = B * K.k
    x = keep("x", A._enc(w, rng, _flat(K.x_planes())).reshape(K.dims, rows, -1).contiguous())
    y = keep("y", A._enc(w, rng, _flat(K.y_planes())).reshape(K.dims, rows, -1).contiguous())
    return x, y


def _layers(K):
    from protocols.secure_comparison_amd.sorting import topk_network

    return topk_network(K.k, K.m)


# ---- chain 1: squared distance -> top-m with the labels as payload -> [m][B] votes -> majority (examples/knn_classify.py) ------------------
@pytest.mark.parametrize("mode", MODES)
def test_knn_classify(world, mode):  # noqa: F811
    from protocols.secure_comparison_amd import secure_majority_batch, secure_squared_distance_batch, secure_topk_batch

    chain, K = f"kNN classify ({mode})", PM.Knn()
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"knn:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    x, y = _knn_inputs(world, rng, K, keep)
    labels = keep("labels", A._enc(world, rng, K.label_rows()).reshape(1, B, K.k, -1).contiguous())
    layers = _layers(K)

    dist = secure_squared_distance_batch(x, y, K.bits, ap, bp)
    _shape(chain, "squared distance", dist, B * K.k)
    _stage(chain, "squared distance", A._dec(world, dist), _flat(K.distances()))

    rows = keep("distances [B][k]", hand(dist).reshape(B, K.k, -1).contiguous())
    values, near, index = secure_topk_batch(rows, K.m, K.l, ap, ad, bp, bd, payload=labels, payload_bits=(K.label_bits,))
    assert index is None
    _shape(chain, "top-m distances", values, B, K.m)
    _shape(chain, "top-m labels", near, 1, B, K.m)
    want = K.nearest(layers)
    _stage(chain, "top-m distances", A._dec(world, values), [t[0] for r in want for t in r])
    _stage(chain, "top-m labels", A._dec(world, near), [t[1] for r in want for t in r])

    votes = keep("votes [m][B]", hand(near)[0].permute(1, 0, 2).contiguous())
    _shape(chain, "votes", votes, K.m, B)
    _stage(chain, "votes", A._dec(world, votes), _flat(K.votes(layers)))
    cls, cnt = secure_majority_batch(votes, K.classes, ap, ad, bp, bd, index_bits=K.label_bits)
    _shape(chain, "majority class", cls, B)
    _shape(chain, "majority count", cnt, B)
    want_cls, want_cnt = K.majority(layers)
    _stage(chain, "majority count", A._dec(world, cnt), want_cnt)
    _stage(chain, "majority class", A._dec(world, cls), want_cls)
    keep.unchanged()


# ---- chain 2: squared distance -> argmin -> lookup by the encrypted index; gather by (argmin, argmax) (examples/label_lookup.py) -----------
@pytest.mark.parametrize("mode", MODES)
def test_nearest_label(world, mode):  # noqa: F811
    from protocols.secure_comparison_amd import (secure_argmax_batch, secure_argmin_batch, secure_gather_batch, secure_lookup_batch,
                                                 secure_squared_distance_batch)

    chain, K = f"nearest label ({mode})", PM.Knn()
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"label:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    x, y = _knn_inputs(world, rng, K, keep)
    table = keep("table", A._enc(world, rng, _flat(K.table())).reshape(K.k, B, -1).contiguous())

    dist = secure_squared_distance_batch(x, y, K.bits, ap, bp)
    _stage(chain, "squared distance", A._dec(world, dist), _flat(K.distances()))
    rows = keep("distances [B][k]", hand(dist).reshape(B, K.k, -1).contiguous())

    low, idx = secure_argmin_batch(rows, K.l, ap, ad, bp, bd)
    _shape(chain, "argmin value", low, B)
    _shape(chain, "argmin index", idx, B)
    _stage(chain, "argmin value", A._dec(world, low), [v for v, _ in K.argmin()])
    _stage(chain, "argmin index", A._dec(world, idx), [i for _, i in K.argmin()])

    idx = keep("argmin index", hand(idx).contiguous())
    lab = secure_lookup_batch(table, idx, K.label_bits, ap, bp)
    _shape(chain, "lookup", lab, B)
    _stage(chain, "lookup", A._dec(world, lab), K.looked_up())

    high, imax = secure_argmax_batch(rows, K.l, ap, ad, bp, bd)
    _stage(chain, "argmax value", A._dec(world, high), [v for v, _ in K.argmax()])
    _stage(chain, "argmax index", A._dec(world, imax), [i for _, i in K.argmax()])
    both = keep("argmin and argmax [2][B]", torch.stack([idx, hand(imax)]).contiguous())
    got = secure_gather_batch(table, both, K.label_bits, ap, bp)
    _shape(chain, "gather", got, 2, B)
    _stage(chain, "gather", A._dec(world, got), _flat(K.gathered()))
    keep.unchanged()


# ---- chain 3: linear map with signed weights and a bias -> offset -> argmax (examples/linear_score.py) ------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_linear_score(world, mode):  # noqa: F811
    from protocols.secure_comparison_amd import linear_planes_batch, secure_argmax_batch

    chain, L = f"linear score ({mode})", PM.Linear()
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"linear:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    x = keep("x", A._enc(world, rng, _flat(L.planes())).reshape(L.K, B, -1).contiguous())
    x_bits = L.x_bits(sk.n.bit_length())
    before = engine.launch_counts()
    with pytest.raises(ValueError, match="row 3"):                       # one bit more and the fit rule refuses the row of +-(2^64 - 1)
        linear_planes_batch(x, L.W, ap, bias=L.bias, x_bits=x_bits + 1)
    assert engine.launch_counts() == before

    rho = None if mode == "handed-on" else _rho(world, rng, L.J, B)
    scores = linear_planes_batch(x, L.W, ap, bias=L.bias, x_bits=x_bits, rho=rho)
    _shape(chain, "scores", scores, L.J, B)
    _stage(chain, "scores", A._dec(world, scores, signed=True), _flat(L.scores()))
    if rho is None:                                                       # the zero row is the bare 1 + b N, b = N - 10
        _stage(chain, "scores: the zero row's residue", A._ints(engine, scores[0]), [(1 + (L.bias[0] % sk.n) * sk.n) % sk.n2] * B)

    shifted = _offset(ap, keep("scores", scores), L.reach())
    _stage(chain, "offset scores", A._dec(world, shifted), _flat(L.shifted()))
    rows = keep("scores [B][J]", hand(shifted).permute(1, 0, 2).contiguous())
    _shape(chain, "scores [B][J]", rows, B, L.J)
    top, label = secure_argmax_batch(rows, L.l(), ap, ad, bp, bd)
    _shape(chain, "best score", top, B)
    _shape(chain, "label", label, B)
    _stage(chain, "best score", A._dec(world, top), [v for v, _ in L.best()])
    _stage(chain, "label", A._dec(world, label), [j for _, j in L.best()])
    keep.unchanged()


# ---- chain 4: histogram -> running sum -> quantile; the one-call forms and the sorting network beside it (examples/histogram_median.py) ---
@pytest.mark.parametrize("k", (4, 1))
@pytest.mark.parametrize("mode", MODES)
def test_histogram_median(world, mode, k):  # noqa: F811
    from protocols.secure_comparison_amd import (secure_cdf_batch, secure_histogram_batch, secure_histogram_median_batch, secure_kth_batch,
                                                 secure_quantile_batch)
    from protocols.secure_comparison_amd import aggregate as AG
    from protocols.secure_comparison_amd.batch import secure_comparison_batch
    from protocols.secure_comparison_amd.selection import _comparison_draws

    chain, H = f"histogram median (k = {k}, {mode})", PM.Histogram(k)
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"median:{k}:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    m, w = H.m, ap.mod_n2.nwords
    enc = keep("indices", A._enc(world, rng, _flat(H.idx)).reshape(m, B, -1).contiguous())
    ranks = keep("ranks", A._enc(world, rng, H.ranks))
    fresh = mode == "rerandomized"

    hist = secure_histogram_batch(enc, k, ap, bp, index_bits=H.ib, rho=_rho(world, rng, k, B) if fresh else None)
    _shape(chain, "histogram", hist, k, B)
    _stage(chain, "histogram", A._dec(world, hist), _flat(H.hist()))
    cdf = AG.cumsum_planes_batch(keep("histogram", hist), ap, rho=_rho(world, rng, k, B) if fresh else None)
    _shape(chain, "running sum", cdf, k, B)
    _stage(chain, "running sum", A._dec(world, cdf), _flat(H.cdf()))
    direct = secure_cdf_batch(enc, k, ap, bp, index_bits=H.ib)
    _stage(chain, "secure_cdf_batch", A._dec(world, direct), _flat(H.cdf()))

    kths = (0, m - 1, H.ranks)
    keep("running sum", cdf)
    for kth in kths:
        name = "encrypted ranks" if isinstance(kth, list) else f"kth = {kth}"
        if k > 1:                                                        # the quantile's own steps over the chained distribution
            rows = (k - 1) * B
            xs = keep("running sum without its last plane", cdf[:k - 1].reshape(rows, w).contiguous())
            ys = ranks.unsqueeze(0).expand(k - 1, B, w).reshape(rows, w).contiguous() if isinstance(kth, list) else \
                ap.encrypt_raw_batch(engine.upload([kth] * rows, ap.mod_n.nwords))
            bits = secure_comparison_batch(xs, keep("[[kth]]", ys), H.l, ap, ad, bp, bd, _comparison_draws(rows, H.l, ap, ad, bp, bd))
            _shape(chain, f"comparison bits, {name}", bits, rows)
            _stage(chain, f"comparison bits, {name}", A._dec(world, bits), _flat(H.bits_below(kth)))
            chained = AG.sum_planes_batch(keep("comparison bits", hand(bits).reshape(k - 1, B, w).contiguous()), ap)
            _shape(chain, f"chained quantile, {name}", chained, B)
            _stage(chain, f"chained quantile, {name}", A._dec(world, chained), H.quantile(kth))
        got = secure_quantile_batch(enc, k, ranks if isinstance(kth, list) else kth, ap, ad, bp, bd, index_bits=H.ib)
        _shape(chain, f"secure_quantile_batch, {name}", got, B)
        _stage(chain, f"secure_quantile_batch, {name}", A._dec(world, got), H.quantile(kth))
    got = secure_histogram_median_batch(enc, k, ap, ad, bp, bd, index_bits=H.ib)
    _stage(chain, "secure_histogram_median_batch", A._dec(world, got), H.quantile((m - 1) // 2))

    per_row = keep("indices [B][m]", enc.permute(1, 0, 2).contiguous())                   # the sorting-network route over the same indices
    below = H.below_k()
    assert below
    for kth in (0, (m - 1) // 2, m - 1):
        got = A._dec(world, secure_kth_batch(per_row, kth, H.ib, ap, ad, bp, bd)[0])
        _stage(chain, f"secure_kth_batch, kth = {kth}", got, H.kth_of_indices(kth))
        _stage(chain, f"quantile against the sorting network, kth = {kth}", [got[b] for b in below], [H.quantile(kth)[b] for b in below])
    keep.unchanged()


# ---- chain 5: group-by sum -> sort with the permutation -> gather of a label table by the permutation's first index -----------------------
@pytest.mark.parametrize("mode", MODES)
def test_groupby_then_rank(world, mode):  # noqa: F811
    from protocols.secure_comparison_amd import secure_gather_batch, secure_groupby_sum_batch, secure_sort_batch

    chain, Gb = f"group-by then rank ({mode})", PM.Groupby()
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"groupby:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    sums = []
    for g in range(Gb.G):
        v, i = keep(f"values {g}", A._enc(world, rng, Gb.vals[g])), keep(f"groups {g}", A._enc(world, rng, Gb.idx[g]))
        out = secure_groupby_sum_batch(v, i, Gb.k, Gb.bits, ap, bp, index_bits=Gb.ib,
                                       rho=_rho(world, rng, Gb.k) if mode == "rerandomized" else None)
        _shape(chain, f"group-by sum of set {g}", out, Gb.k)
        _stage(chain, f"group-by sum of set {g}", A._dec(world, out), Gb.sums()[g])
        sums.append(out)
    rows = keep("sums [G][k]", torch.stack(sums).contiguous())
    ordered, none, perm = secure_sort_batch(rows, Gb.l, ap, ad, bp, bd, descending=True, return_indices=True)
    assert none is None
    _shape(chain, "sorted sums", ordered, Gb.G, Gb.k)
    _shape(chain, "permutation", perm, Gb.G, Gb.k)
    want_sorted, want_perm = Gb.ranked()
    _stage(chain, "sorted sums", A._dec(world, ordered), _flat(want_sorted))
    _stage(chain, "permutation", A._dec(world, perm), _flat(want_perm))

    table = keep("table", A._enc(world, rng, _flat(Gb.table)).reshape(Gb.k, Gb.G, -1).contiguous())
    first = keep("first index [1][G]", hand(perm[:, 0]).unsqueeze(0).contiguous())
    lab = secure_gather_batch(table, first, Gb.table_bits, ap, bp)
    _shape(chain, "gathered label", lab, 1, Gb.G)
    _stage(chain, "gathered label", A._dec(world, lab), Gb.first_label())
    keep.unchanged()


# ---- chain 6: signed products -> segment sums without rho -> offset -> interval and equality against encrypted constants -------------------
@pytest.mark.parametrize("mode", MODES)
def test_arithmetic_chain(world, mode):  # noqa: F811
    from protocols.secure_comparison_amd import secure_equal_batch, secure_in_range_batch, secure_multiply_batch
    from protocols.secure_comparison_amd import aggregate as AG

    chain, Ar = f"arithmetic chain ({mode})", PM.Arithmetic()
    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"arithmetic:{mode}")
    keep, hand = _Inputs(chain), _hand(world, rng, mode)
    x, y = keep("x", A._enc(world, rng, Ar.x)), keep("y", A._enc(world, rng, Ar.y))
    prod = secure_multiply_batch(x, y, Ar.xb, Ar.xb, ap, bp, signed=True)
    _shape(chain, "products", prod, Ar.seg * B)
    _stage(chain, "products", A._dec(world, prod, signed=True), Ar.products())

    sums = AG.sum_rows_batch(keep("products", hand(prod)), ap, segment=Ar.seg, rho=_rho(world, rng, B) if mode == "rerandomized" else None)
    _shape(chain, "segment sums", sums, B)
    _stage(chain, "segment sums", A._dec(world, sums, signed=True), Ar.sums())
    shifted = keep("offset sums", hand(_offset(ap, keep("segment sums", sums), Ar.offset)).contiguous())
    _stage(chain, "offset sums", A._dec(world, shifted), Ar.shifted())

    lo = keep("lower end", A._enc(world, rng, [Ar.range_lo + Ar.offset] * B))
    hi = keep("upper end", A._enc(world, rng, [Ar.range_hi + Ar.offset] * B))
    inside = secure_in_range_batch(shifted, lo, hi, Ar.l, ap, ad, bp, bd)
    _shape(chain, "in range", inside, B)
    _stage(chain, "in range", A._dec(world, inside), Ar.in_range())
    c = keep("constant", A._enc(world, rng, [Ar.equal_to + Ar.offset] * B))
    eq, le, ge = secure_equal_batch(shifted, c, Ar.l, ap, ad, bp, bd)
    want_eq, want_le, want_ge = Ar.equal()
    for name, t, want in (("x <= c", le, want_le), ("c <= x", ge, want_ge), ("equal", eq, want_eq)):
        _shape(chain, name, t, B)
        _stage(chain, name, A._dec(world, t), want)
    keep.unchanged()


# ---- chain 7: chain 1 between two players, device tensors handed from one call to the next ------------------------------------------------
def test_players_knn_classify(engine, keys):
    from protocols.secure_comparison_amd.dotproduct import _differences

    chain, K = "two players", PM.Knn()
    sk, ap, bp, alice, bob = _two_players(engine, keys, K.l)
    w = (engine, sk, ap, None, bp, None)
    rng = random.Random("players:knn")
    keep = _Inputs(chain)
    x, y = _knn_inputs(w, rng, K, keep)
    labels = keep("labels", A._enc(w, rng, K.label_rows()).reshape(1, B, K.k, -1).contiguous())
    layers, lb = _layers(K), K.label_bits

    async def run():
        d = keep("differences", _differences(x, y, ap))
        dist, _ = await asyncio.gather(alice.perform_secure_dot_batch(d, None, K.bits + 1, signed=True, square=True, engine=engine),
                                       bob.perform_secure_dot_batch(K.dims, K.bits + 1, signed=True, square=True))
        _shape(chain, "squared distance", dist, B * K.k)
        _stage(chain, "squared distance", A._dec(w, dist), _flat(K.distances()))
        rows = keep("distances [B][k]", dist.reshape(B, K.k, -1).contiguous())
        (values, near, _), _ = await asyncio.gather(
            alice.perform_secure_topk_batch(rows, K.m, payload=labels, payload_bits=(lb,), engine=engine),
            bob.perform_secure_topk_batch(K.k, K.m, payload_bits=(lb,)))
        _shape(chain, "top-m distances", values, B, K.m)
        _shape(chain, "top-m labels", near, 1, B, K.m)
        want = K.nearest(layers)
        _stage(chain, "top-m distances", A._dec(w, values), [t[0] for r in want for t in r])
        _stage(chain, "top-m labels", A._dec(w, near), [t[1] for r in want for t in r])
        votes = keep("votes [m][B]", near[0].permute(1, 0, 2).contiguous())
        (cls, cnt), _ = await asyncio.gather(alice.perform_secure_majority_batch(votes, K.classes, index_bits=lb, engine=engine),
                                             bob.perform_secure_majority_batch(K.classes, K.m, index_bits=lb))
        return cls, cnt

    cls, cnt = asyncio.run(run())
    _shape(chain, "majority class", cls, B)
    want_cls, want_cnt = K.majority(layers)
    _stage(chain, "majority count", A._dec(w, cnt), want_cnt)
    _stage(chain, "majority class", A._dec(w, cls), want_cls)
    keep.unchanged()

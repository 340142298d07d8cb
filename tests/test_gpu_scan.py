"""The running product along an axis (sc_modscan_axis / k_scan_axis) and what is built on it, on the GPU.  Every residue
is compared bit for bit with plain Python (tests/_scan_model.py): every compiled instance at the ends of its configuration's range and
every geometry, the last position against sc_modprod_axis, every recursion depth a forced chunk length reaches with the launch counters
held to the plan, the grid-stride loop, the refusals with nothing launched, the running sums of the Python layer on both axes, and the
cumulative distribution and the quantile decrypted on every row, under injected draws, under the library's own draws and between two
players.  Outputs sit between guard rows and inputs are compared with their clones afterwards."""
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _instance_matrix as M  # noqa: E402
import _reduce_model as R  # noqa: E402
import _scan_model as S  # noqa: E402
import test_gpu_aggregate as A  # noqa: E402
from test_gpu_aggregate import n2world, seeded_world, world  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = A.GUARD
KAPPA = A.KAPPA


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _counts(eng, g, l):
    c = eng.launch_counts()
    return c.get(("scan", g, l, 29, False, False, False), 0), c.get(("reduce", g, l, 29, False, False, False), 0)


def _plan(eng, g, outer, K, inner, forced=0):
    from protocols.secure_comparison_amd.aggregate import scan_plan

    return scan_plan(outer, K, inner, A._num_cu(eng) * 8 * (64 // g), forced)


def _run(eng, mod, cfg, x, outer, K, inner, label, forced=0):
    """sc_modscan_axis into a guarded output: guards and input intact, the launches under bit 29 and bit 28 those of the plan; the
    result as Python ints."""
    g, l = cfg
    rows = outer * K * inner
    buf = torch.full((rows + 2, mod.nwords), GUARD, dtype=torch.int32, device=eng.device)
    out = buf[1:rows + 1]
    clone = x.clone()
    scans, totals = _counts(eng, g, l)
    eng.modscan_axis(mod, x, outer, K, inner, out=out)
    torch.cuda.synchronize()
    plan = _plan(eng, g, outer, K, inner, forced)
    scans2, totals2 = _counts(eng, g, l)
    assert (scans2 - scans, totals2 - totals) == (S.count(plan, "scan"), S.count(plan, "totals")), (label, "launches of the plan")
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), (label, "a guard row was written")
    assert torch.equal(x, clone), (label, "the input was modified")
    return eng.download(out)


def _last(got, outer, K, inner):
    return [got[(o * K + K - 1) * inner + i] for o in range(outer) for i in range(inner)]


# ---- every compiled instance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", S.INSTANCES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_instance(engine, cfg):
    """Smallest and largest whole-word modulus of the configuration with low limb -1, 1 and random, and a square; operands include
    0, 1, n - 1 and all-ones limbs below n.  Every position against the model (a 0 blanks the rest of its own scan and no other), the
    last position against sc_modprod_axis word for word."""
    g, l = cfg
    inst = ("vm", g, l, 29, False, False, False)
    lo, hi = M.size_range(cfg)
    cases = [(f"{bits}-{shape}", M.make_modulus(bits, shape)) for bits in (lo, hi) for shape in ("neg1", "one", "rand")] + \
            [(f"{hi}-square", M.make_modulus(hi, "square"))]
    assert all(M.first_fit(n.bit_length()) == cfg for _, n in cases)
    zeros_seen = 0
    for ci, (case_label, n) in enumerate(cases):
        mod = engine.modulus(n)
        for gi, (outer, K, inner) in enumerate(A._geometries(64 // g)):
            ops = M.operands(n, inst, outer * K * inner, ci + gi)
            if gi % 2:                                  # zeros blank the rest of their scans: keep them to every other geometry
                ops = [v if v else n - 2 for v in ops]
            random.Random(f"{n & 0xffff}:{gi}").shuffle(ops)
            label = f"{g}x{l}/{case_label}/{(outer, K, inner)}"
            x = engine.upload(ops, mod.nwords)
            got = _run(engine, mod, cfg, x, outer, K, inner, label)
            A._assert_rows(label, got, S.scan_axis(n, ops, outer, K, inner))
            for at, v in enumerate(ops):                # the zero rule, spelt out
                if v == 0:
                    o, j, i = at // (K * inner), at // inner % K, at % inner
                    assert all(got[(o * K + jj) * inner + i] == 0 for jj in range(j, K)), label
                    zeros_seen += 1
            assert _last(got, outer, K, inner) == engine.download(engine.modprod_axis(mod, x, outer, K, inner)), (label, "against the reduction")
    assert zeros_seen > 0


def test_instance_without_a_kernel_is_refused(engine):
    """A one-lane (1,18) modulus has no k_scan_axis instance: ValueError (SC_ERR_ARG) that names the configuration."""
    n = M.make_modulus(256, "rand")
    assert M.first_fit(256) == (1, 18)
    mod = engine.modulus(n)
    x = engine.upload([3, 5], mod.nwords)
    with pytest.raises(ValueError, match=r"k_scan_axis.*G=1, L=18, W=29"):
        engine.modscan_axis(mod, x, 1, 2, 1)


# ---- the 1024-bit key's N^2: recursion, short last chunks, seeds across chunk and level boundaries ------------------------------------
DEPTH = [(c, K, 2, 3) for c in (2, 3) for K in (2, 3, 4, 5, 7, 8, 9, 27, 28)] + [(32, K, outer, 1) for K in (33, 1025) for outer in (1, 3)]


@pytest.mark.parametrize("chunk,K,outer,inner", DEPTH)
def test_forced_chunks(n2world, chunk, K, outer, inner):
    """A forced chunk length equals the automatic plan and the model, whatever the depth and however short the last chunk; the launch
    counters under bit 29 and bit 28 are the plan's (in _run)."""
    eng, sk, mod, cfg = n2world
    n = sk.n2
    rng = random.Random(f"scan-depth:{chunk}:{K}:{outer}")
    ops = [rng.randrange(1, n) for _ in range(outer * K * inner)]
    ops[0], ops[-1], ops[len(ops) // 2] = 1, n - 1, (1 << (29 * 72)) % n
    x = eng.upload(ops, mod.nwords)
    expect = S.scan_axis(n, ops, outer, K, inner)
    auto = _run(eng, mod, cfg, x, outer, K, inner, f"auto/{K}")
    try:
        eng.set_reduce_chunk(chunk)
        plan = _plan(eng, cfg[0], outer, K, inner, chunk)
        assert K <= chunk or S.count(plan, "totals") >= 1
        forced = _run(eng, mod, cfg, x, outer, K, inner, f"chunk {chunk}/{K}", forced=chunk)
    finally:
        eng.set_reduce_chunk(0)
    A._assert_rows(f"auto/{K}", auto, expect)
    A._assert_rows(f"chunk {chunk}/{K}", forced, expect)


def test_grid_stride(n2world):
    """More chains than every resident wave of a full chip holds, K = 2, 257 distinct operands tiled, every row compared."""
    eng, sk, mod, cfg = n2world
    n, ng = sk.n2, 64 // cfg[0]
    chains = A._num_cu(eng) * 16 * ng + ng + 1
    rng = random.Random("scan-grid-stride")
    ops = [rng.randrange(n) for _ in range(M.TILE)]
    rows = eng.upload(ops, mod.nwords)
    index = torch.arange(2 * chains, device=eng.device) % M.TILE
    x = rows[index].contiguous()
    # member j of scan i is operand (j * chains + i) mod 257: position (0, i) is the operand, (1, i) its product with the next member
    prods = eng.upload([ops[t] * ops[(chains + t) % M.TILE] % n for t in range(M.TILE)], mod.nwords)
    expect = torch.cat([rows[index[:chains]], prods[index[:chains]]])
    buf = torch.full((2 * chains + 2, mod.nwords), GUARD, dtype=torch.int32, device=eng.device)
    clone = x.clone()
    assert _plan(eng, cfg[0], 1, 2, chains) == [("scan", 2, 2, chains)]
    eng.modscan_axis(mod, x, 1, 2, chains, out=buf[1:2 * chains + 1])
    torch.cuda.synchronize()
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()) and torch.equal(x, clone)
    differ = (buf[1:2 * chains + 1] != expect).any(dim=1)
    assert not bool(differ.any()), f"{int(differ.sum())} of {2 * chains} rows differ, first at row {int(differ.nonzero()[0])}"


def test_argument_checks_launch_nothing(n2world):
    eng, sk, mod, cfg = n2world
    w = mod.nwords
    buf = eng.upload([3] * 16, w)
    lib, ctx, p = eng.lib, eng.ctx, eng._ptr
    off = lambda rows: torch.Tensor.data_ptr(buf) + rows * w * 4  # noqa: E731
    before, stats = eng.launch_counts(), eng.stats()
    eng._sync_stream()
    assert lib.sc_modscan_axis(ctx, mod.id, None, 1, 2, 1, p(buf)) == -1                      # null pointers
    assert lib.sc_modscan_axis(ctx, mod.id, p(buf), 1, 2, 1, None) == -1
    assert "sc_modscan_axis: bad argument" in lib.sc_last_error(ctx).decode()
    assert lib.sc_modscan_axis(ctx, 10 ** 6, p(buf), 1, 2, 1, off(8)) == -1                   # no such modulus
    assert lib.sc_modscan_axis(ctx, mod.id, p(buf), 1, 0, 1, off(8)) == -1                    # K = 0
    assert "sc_modscan_axis: K must be at least 1" in lib.sc_last_error(ctx).decode()
    for outer, K, inner in ((1 << 39, 4, 1), (1 << 62, 4, 1), (3, 1 << 63, 5), (1 << 20, 1 << 20, 1 << 20)):
        assert lib.sc_modscan_axis(ctx, mod.id, p(buf), outer, K, inner, off(8)) == -1        # past 2^40 words, or wrapping 2^64
        assert "sc_modscan_axis: outer * K * inner * nwords exceeds 2^40 words" in lib.sc_last_error(ctx).decode()
    for x_at, out_at in ((0, 0), (0, 3), (0, 7), (2, 0), (7, 0)):                            # x and out: 8 rows each (2 x 2 x 2)
        assert lib.sc_modscan_axis(ctx, mod.id, off(x_at), 2, 2, 2, off(out_at)) == -1, (x_at, out_at)
        assert "sc_modscan_axis: out overlaps x" in lib.sc_last_error(ctx).decode()
    assert lib.sc_modscan_axis(ctx, mod.id, p(buf), 0, 2, 1, off(8)) == 0                     # empty: SC_OK, nothing launched
    assert lib.sc_modscan_axis(ctx, mod.id, p(buf), 3, 2, 0, off(8)) == 0
    assert lib.sc_paillier_cumsum_axis(ctx, 10 ** 6, p(buf), 1, 2, 1, off(8)) == -1           # no such key
    assert "sc_paillier_cumsum_axis: bad key" in lib.sc_last_error(ctx).decode()
    torch.cuda.synchronize()
    assert eng.launch_counts() == before and eng.stats() == stats
    assert eng.download(buf) == [3] * 16
    assert lib.sc_modscan_axis(ctx, mod.id, p(buf), 2, 2, 2, off(8)) == 0                     # adjacent, not overlapping: accepted
    torch.cuda.synchronize()
    assert eng.download(buf) == [3] * 8 + [3, 3, 9, 9] * 2


def test_constant_table_turns_over_inside_one_scan(keys):
    """The context keeps 64 constants R^e.  On a fresh context, sums over K = 10 .. 71 leave 62 of them; a scan at a forced chunk of 2
    over K = 28 then needs the four exponents 2, 3, 5, 9 in one call, which the table cannot take beside the 62: it is emptied during that
    call's fetch.  Every result before, in and after that call is the model's, and the launches are the plan's (in _run)."""
    from protocols.secure_comparison_amd.engine import Engine

    sk = oracle_paillier(keys, 1024)
    eng = Engine()
    try:
        mod, n, cfg = eng.modulus(sk.n2), sk.n2, M.first_fit(sk.n2.bit_length())
        assert cfg == (4, 18)
        rng = random.Random("scan-constants")
        ops = [rng.randrange(1, n) for _ in range(71 * 2)]
        rows = eng.upload(ops, mod.nwords)
        sum_of = lambda K, forced=0: A._run(eng, mod, cfg, rows[:2 * K], 1, K, 2, f"sum/{K}", forced=forced)  # noqa: E731
        for K in range(10, 72):                                   # 62 distinct exponents
            A._assert_rows(f"sum/{K}", sum_of(K), R.prod_axis(n, ops[:2 * K], 1, K, 2))
        K = 28
        expect = S.scan_axis(n, ops[:2 * K], 1, K, 2)
        try:
            eng.set_reduce_chunk(2)
            plan = _plan(eng, cfg[0], 1, K, 2, 2)
            assert S.count(plan, "scan") == 4 and S.count(plan, "totals") == 3            # members 1, 2, 4, 8 behind a level's member
            A._assert_rows("scan/turnover", _run(eng, mod, cfg, rows[:2 * K], 1, K, 2, "scan/turnover", forced=2), expect)
            A._assert_rows("sum/10 again", sum_of(10, 2), R.prod_axis(n, ops[:20], 1, 10, 2))
            A._assert_rows("scan/again", _run(eng, mod, cfg, rows[:2 * K], 1, K, 2, "scan/again", forced=2), expect)
        finally:
            eng.set_reduce_chunk(0)
    finally:
        eng.close()


def test_mac_counter_counts_two_products_per_member(n2world):
    eng, sk, mod, cfg = n2world
    s2 = (cfg[0] * cfg[1]) ** 2 * 2.0
    x = eng.upload([5] * (2 * 9 * 3), mod.nwords)
    try:
        for forced in (0, 2):
            eng.set_reduce_chunk(forced)
            eng.mac_counter(reset=True)
            eng.modscan_axis(mod, x, 2, 9, 3)
            assert eng.mac_counter() == s2 * S.products(_plan(eng, cfg[0], 2, 9, 3, forced)), forced
    finally:
        eng.set_reduce_chunk(0)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_running_sums_on_both_axes_of_a_non_square_array(world):
    """cumsum_planes_batch and cumsum_rows_batch on one [3][10] array: segments 1, 2, 5, 10, inclusive and exclusive, with and without
    rho; decrypted against integer running sums, and without rho bit for bit the products of the inputs."""
    from protocols.secure_comparison_amd.aggregate import cumsum_planes_batch, cumsum_rows_batch

    engine, sk, ap = world[0], world[1], world[2]
    rng = random.Random("scan-axes")
    k, B, n2 = 3, 10, sk.n2
    plain = [[rng.randrange(1000) for _ in range(B)] for _ in range(k)]
    x = A._enc(world, rng, [v for row in plain for v in row]).reshape(k, B, -1).contiguous()
    flat, clone = A._ints(engine, x), x.clone()
    rho = engine.upload([rng.randrange(1, sk.n) for _ in range(k * B)], ap.mod_n.nwords).reshape(k, B, -1)
    fresh = lambda cs: [c * pow(r, sk.n, n2) % n2 for c, r in zip(cs, A._ints(engine, rho))]  # noqa: E731

    want = S.scan_axis(n2, flat, 1, k, B)
    sums = [sum(plain[jj][b] for jj in range(j + 1)) for j in range(k) for b in range(B)]
    for exclusive in (False, True):
        bits = [1] * B + want[:-B] if exclusive else want
        ints = [0] * B + sums[:-B] if exclusive else sums
        got = cumsum_planes_batch(x, ap, exclusive=exclusive)
        assert tuple(got.shape) == tuple(x.shape) and A._ints(engine, got) == bits and A._dec(world, got) == ints
        got = cumsum_planes_batch(x, ap, exclusive=exclusive, rho=rho)
        assert A._ints(engine, got) == fresh(bits) and A._dec(world, got) == ints
    for seg in (1, 2, 5, 10):
        want = S.scan_axis(n2, flat, k * (B // seg), seg, 1)
        for exclusive in (False, True):
            bits = [1 if t % seg == 0 else want[t - 1] for t in range(k * B)] if exclusive else want
            ints = [sum(plain[t // B][(t % B) // seg * seg:t % B + (0 if exclusive else 1)]) for t in range(k * B)]
            got = cumsum_rows_batch(x, ap, segment=seg, exclusive=exclusive)
            assert tuple(got.shape) == tuple(x.shape) and A._ints(engine, got) == bits and A._dec(world, got) == ints, (seg, exclusive)
            got = cumsum_rows_batch(x, ap, segment=seg, exclusive=exclusive, rho=rho)
            assert A._ints(engine, got) == fresh(bits) and A._dec(world, got) == ints
    assert A._ints(engine, cumsum_rows_batch(x, ap)) == S.scan_axis(n2, flat, k, B, 1)
    with pytest.raises(ValueError, match="divisor"):
        cumsum_rows_batch(x, ap, segment=3)
    assert torch.equal(x, clone)


# ---- cumulative distribution and quantile ---------------------------------------------------------------------------------------------
COUNT = 20


def _planted(rng, k, m, ib, count):
    """Indices [m][count]: row 0 all in one bin, row 1 all in the first, row 2 all in the last, row 3 only the two end bins (every bin
    between them empty), row 4 an index at or above k that counts at i mod k; the rest random below 2^ib."""
    idx = [[rng.getrandbits(ib) for _ in range(count)] for _ in range(m)]
    for q in range(m):
        idx[q][0], idx[q][1], idx[q][2] = k // 2, 0, k - 1
        idx[q][3] = 0 if q % 2 else k - 1
        idx[q][4] = k + (q % k)
    assert all(v < (1 << ib) for row in idx for v in row)
    return idx


def _sorted_bins(idx, k, b):
    return sorted(row[b] % k for row in idx)


@pytest.mark.parametrize("k", (1, 2, 3, 7))
@pytest.mark.parametrize("m", (1, 3, 5, 8))
def test_cdf_and_quantile(world, m, k):
    """Every row decrypted: the cumulative counts, the bin of every public rank, and encrypted per-row ranks that run through all of them."""
    from protocols.secure_comparison_amd import secure_cdf_batch, secure_histogram_median_batch, secure_quantile_batch
    from protocols.secure_comparison_amd.lookup import default_index_bits

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"quantile:{k}:{m}")
    ib = default_index_bits(k) + 1                                    # room for an index at or above k
    idx = _planted(rng, k, m, ib, COUNT)
    enc = A._enc(world, rng, [v for row in idx for v in row]).reshape(m, COUNT, -1).contiguous()
    clone = enc.clone()
    cdf = secure_cdf_batch(enc, k, ap, bp, index_bits=ib)
    assert tuple(cdf.shape) == (k, COUNT, enc.shape[-1])
    assert A._dec(world, cdf) == [sum(1 for q in range(m) if idx[q][b] % k <= t) for t in range(k) for b in range(COUNT)]
    for kth in range(m):
        got = secure_quantile_batch(enc, k, kth, ap, ad, bp, bd, index_bits=ib)
        assert tuple(got.shape) == (COUNT, enc.shape[-1])
        assert A._dec(world, got) == [_sorted_bins(idx, k, b)[kth] for b in range(COUNT)], kth
    ranks = [b % m for b in range(COUNT)]
    got = secure_quantile_batch(enc, k, A._enc(world, rng, ranks), ap, ad, bp, bd, index_bits=ib)
    assert A._dec(world, got) == [_sorted_bins(idx, k, b)[ranks[b]] for b in range(COUNT)]
    got = secure_histogram_median_batch(enc, k, ap, ad, bp, bd, index_bits=ib)
    assert A._dec(world, got) == [_sorted_bins(idx, k, b)[(m - 1) // 2] for b in range(COUNT)]
    assert torch.equal(enc, clone)


def test_quantile_against_the_sorting_network(world):
    """m = 8 values below k = 7 per row: the bin of every other rank is secure_kth_batch's decrypted value on the same data."""
    from protocols.secure_comparison_amd import secure_kth_batch, secure_quantile_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random("quantile-vs-kth")
    k, m = 7, 8
    idx = [[rng.randrange(k) for _ in range(COUNT)] for _ in range(m)]
    enc = A._enc(world, rng, [v for row in idx for v in row]).reshape(m, COUNT, -1).contiguous()
    rows = enc.permute(1, 0, 2).contiguous()                          # [B][m][2nw]
    for kth in (0, 3, 7):
        ours = A._dec(world, secure_quantile_batch(enc, k, kth, ap, ad, bp, bd))
        theirs = A._dec(world, secure_kth_batch(rows, kth, 3, ap, ad, bp, bd)[0])
        assert ours == theirs == [_sorted_bins(idx, k, b)[kth] for b in range(COUNT)]


def test_quantile_refuses_before_any_launch(world):
    from protocols.secure_comparison_amd import secure_quantile_batch

    engine, sk, ap, ad, bp, bd = world
    enc = A._enc(world, random.Random("scan-refuse"), [1, 2, 3, 0, 1, 2]).reshape(3, 2, -1).contiguous()
    before = engine.launch_counts()
    for bad in (-1, 3, 2.0, "0", None):
        with pytest.raises(ValueError):
            secure_quantile_batch(enc, 4, bad, ap, ad, bp, bd)
    with pytest.raises(ValueError, match="encrypted ranks"):
        secure_quantile_batch(enc, 4, enc[0][:1].contiguous(), ap, ad, bp, bd)
    assert engine.launch_counts() == before


# ---- injected draws: every intermediate against the models ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(3, 5), (7, 3), (2, 1)])
def test_cdf_and_quantile_under_injected_draws(world, keys, k, m):
    """draws= and comparison_draws= handed in: P, E and the rotated one-hot against the model, the comparison's bits against the oracle's,
    and the outputs bit for bit the scan and the sum of those intermediates."""
    from oracle import sc_oracle as o
    import test_gpu_parity as P
    from protocols.secure_comparison_amd import secure_cdf_batch, secure_quantile_batch
    from protocols.secure_comparison_amd.aggregate import count_bits
    from protocols.secure_comparison_amd.lookup import default_index_bits

    engine, sk, ap, ad, bp, bd = world
    od = oracle_dgk(keys, "dgk_1024_l16")
    rng = random.Random(f"inj:quantile:{k}:{m}")
    ib, count, n2, kth = default_index_bits(k), 6, sk.n2, (m - 1) // 2
    idx = [[rng.getrandbits(ib) for _ in range(count)] for _ in range(m)]
    for q in range(m):
        idx[q][0], idx[q][1], idx[q][2] = 0, (k - 1), (1 << ib) - 1
    i_t = A._enc(world, rng, [v for row in idx for v in row]).reshape(m, count, -1).contiguous()
    flat = A._ints(engine, i_t)
    i_c = [flat[q * count:(q + 1) * count] for q in range(m)]
    lay, draws, md = A._onehot_draws(world, rng, ib, k, m, count)
    hot = A._check_onehot_steps(world, lay, i_c, i_t, draws, md, idx)
    hist = [A._prod(n2, [hot[(q * k + t) * count + b] for q in range(m)]) for t in range(k) for b in range(count)]
    want_cdf = S.scan_axis(n2, hist, 1, k, count)
    cdf = secure_cdf_batch(i_t, k, ap, bp, index_bits=ib, draws=md)
    assert A._ints(engine, cdf) == want_cdf
    assert A._dec(world, cdf) == [sum(1 for q in range(m) if idx[q][b] % k <= t) for t in range(k) for b in range(count)]

    l, rows = count_bits(m), (k - 1) * count
    drs = [o.draw(rng, l, sk, od, 400, shuffle=True) for _ in range(rows)]
    cd = P._draw_tensors(engine, drs, l, ap.mod_n.nwords, (od.u.bit_length() + 31) // 32, (400 + 31) // 32, engine.device)
    y = (1 + kth * sk.n) % n2                                          # the unrandomized [[kth]]
    bits = [o.compare(want_cdf[r], y, l, sk, od, drs[r], True) for r in range(rows)]
    got = secure_quantile_batch(i_t, k, kth, ap, ad, bp, bd, index_bits=ib, draws=md, comparison_draws=cd)
    assert A._ints(engine, got) == [A._prod(n2, [bits[t * count + b] for t in range(k - 1)]) for b in range(count)]
    assert A._dec(world, got) == [_sorted_bins(idx, k, b)[kth] for b in range(count)]


# ---- the library's own draws against the replay: the one-hot's, then the comparison's ---------------------------
def replay_quantile(sk, dgk, key, idx, k, ib, B, kth):
    """The expected cumulative distribution and quantile ciphertexts of every row under the generator `key`, from _draw_replay's
    functions in call order -- the one-hot's three calls, then one comparison batch over (k - 1) B rows at l = bits(m) -- and the
    driver that made them."""
    import _draw_replay as dr
    from protocols.secure_comparison_amd.aggregate import count_bits

    m, n2 = len(idx), sk.n2
    d = dr.Driver(sk, dgk, count_bits(m), 400, key)
    hot = A._model_onehot(sk, d.a, idx, k, ib, B)
    hist = [A._prod(n2, [hot[q][t][b] for q in range(m)]) for t in range(k) for b in range(B)]
    cdf = S.scan_axis(n2, hist, 1, k, B)
    rows = (k - 1) * B
    bits = d.compare(cdf[:rows], [(1 + kth * sk.n) % n2] * rows, range(rows), rows)[0]
    return cdf, [A._prod(n2, [bits[t * B + b] for t in range(k - 1)]) for b in range(B)], d


def test_own_draws_cdf_and_quantile(seeded_world, keys):
    """Seeded generator, no draws argument: the distribution and the quantile are the replay's ciphertexts bit for bit, and the generator
    ends on call 3 and on call 11."""
    from oracle import chacha_rng as cr
    from protocols.secure_comparison_amd import secure_cdf_batch, secure_quantile_batch

    engine, sk, ap, ad, bp, bd = seeded_world
    rng = random.Random("own:quantile")
    k, m, ib, B, kth = 4, 3, 2, 5, 1
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    idx[0][0] = idx[1][0] = idx[2][0] = 3
    i_t = A._enc(seeded_world, rng, [v for row in idx for v in row]).reshape(m, B, -1).contiguous()
    want_cdf, want_q, d = replay_quantile(sk, oracle_dgk(keys, "dgk_1024_l16"), A.KEY, idx, k, ib, B, kth)
    engine.rng_seed(A.KEY)
    assert A._ints(engine, secure_cdf_batch(i_t, k, ap, bp, index_bits=ib)) == want_cdf
    assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(A.KEY, 3, 64, 4)
    engine.rng_seed(A.KEY)
    got = secure_quantile_batch(i_t, k, kth, ap, ad, bp, bd, index_bits=ib)
    assert A._ints(engine, got) == want_q
    assert A._dec(seeded_world, got) == [_sorted_bins(idx, k, b)[kth] for b in range(B)]
    assert d.calls[0] == 11 and engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(A.KEY, 11, 64, 4)


# ---- two players over a communicator; scans between the other families -----------------------------------------------------------------
def test_players_cdf_and_quantile(engine, keys):
    import asyncio

    from protocols.secure_comparison_amd import DGK, InMemoryCommunicator, Initiator, KeyHolder, Paillier
    from protocols.secure_comparison_amd.engine import Engine

    sk, dk = oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16")
    if not A._HIS:
        A._HIS.append(Engine())
    his = A._HIS[0]
    bp = Paillier(sk.n, sk.p, sk.q, engine=his)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=his, randomizer_bits=400)
    ap = Paillier(sk.n, engine=engine)
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=600.0)
    alice = Initiator(16, communicator=comm, other_party="keyholder")
    bob = KeyHolder(16, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    w = (engine, sk, ap, None, bp, bd)
    rng = random.Random("scan-players")
    k, m, B = 5, 4, 20
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    ranks = [b % m for b in range(B)]
    i_t = A._enc(w, rng, [v for row in idx for v in row]).reshape(m, B, -1).contiguous()
    r_t = A._enc(w, rng, ranks)

    async def run():
        cdf, _ = await asyncio.gather(alice.perform_secure_cdf_batch(i_t, k, engine=engine), bob.perform_secure_cdf_batch(k, m))
        q1, _ = await asyncio.gather(alice.perform_secure_quantile_batch(i_t, k, 2, engine=engine), bob.perform_secure_quantile_batch(k, m))
        q2, _ = await asyncio.gather(alice.perform_secure_quantile_batch(i_t, k, r_t, engine=engine), bob.perform_secure_quantile_batch(k, m))
        q3, _ = await asyncio.gather(alice.perform_secure_quantile_batch(i_t, 1, 0, engine=engine), bob.perform_secure_quantile_batch(1, m))
        return cdf, q1, q2, q3

    cdf, q1, q2, q3 = asyncio.run(run())
    dec = lambda t: his.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).to(his.device).contiguous()))  # noqa: E731
    assert dec(cdf) == [sum(1 for q in range(m) if idx[q][b] <= t) for t in range(k) for b in range(B)]
    assert dec(q1) == [_sorted_bins(idx, k, b)[2] for b in range(B)]
    assert dec(q2) == [_sorted_bins(idx, k, b)[ranks[b]] for b in range(B)]
    assert dec(q3) == [0] * B
    with pytest.raises(ValueError, match="expected 0 .. 3"):
        asyncio.run(alice.perform_secure_quantile_batch(i_t, k, m, engine=engine))


def test_interleaved_with_the_other_families(world):
    """Scans between calls of the reduction, multiplication, one-hot and comparison families on one context, at a forced chunk of 2 (five
    levels of totals and prefixes in the temporary): every scan is compared with the model, every other result decrypted."""
    from protocols.secure_comparison_amd import secure_multiply_batch, secure_onehot_batch
    from protocols.secure_comparison_amd.aggregate import cumsum_planes_batch, cumsum_rows_batch, sum_planes_batch
    from protocols.secure_comparison_amd.selection import secure_minimum_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random("scan-interleave")
    k, B, n2 = 37, 40, sk.n2
    plain = [[rng.randrange(1 << 12) for _ in range(B)] for _ in range(k)]
    x = A._enc(world, rng, [v for row in plain for v in row]).reshape(k, B, -1).contiguous()
    flat = A._ints(engine, x)
    want_planes, want_rows = S.scan_axis(n2, flat, 1, k, B), S.scan_axis(n2, flat, k, B, 1)
    try:
        engine.set_reduce_chunk(2)
        assert A._ints(engine, cumsum_planes_batch(x, ap)) == want_planes
        assert A._ints(engine, sum_planes_batch(x, ap)) == want_planes[-B:]
        prod = secure_multiply_batch(x[0], x[1], 12, 12, ap, bp)
        assert A._ints(engine, cumsum_rows_batch(x, ap)) == want_rows
        assert A._dec(world, prod) == [a * b for a, b in zip(plain[0], plain[1])]
        hot = secure_onehot_batch(x[2], 5, ap, bp, index_bits=12)
        assert A._ints(engine, cumsum_planes_batch(x, ap)) == want_planes
        assert A._dec(world, hot) == [int(v % 5 == t) for t in range(5) for v in plain[2]]
        low, _ = secure_minimum_batch(x[3], x[4], 16, ap, ad, bp, bd)
        assert A._ints(engine, cumsum_rows_batch(x, ap)) == want_rows
        assert A._dec(world, low) == [min(a, b) for a, b in zip(plain[3], plain[4])]
    finally:
        engine.set_reduce_chunk(0)

"""The product along an axis (sc_modprod_axis / k_prod_axis) and what is built on it, on the GPU.  Every residue is
compared bit for bit with plain Python (tests/_reduce_model.py): every compiled instance at the ends of its configuration's range, every
tree depth a forced chunk length reaches, the grid-stride loop, both axes of a non-square array, the refusals with nothing launched, and
the compositions -- histogram, majority, group-by count and sum -- decrypted and compared with plain Python on every row.  Outputs sit
between guard rows and inputs are compared with their clones afterwards."""
import os
import random
import sys

import pytest
import torch

from conftest import oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _instance_matrix as M  # noqa: E402
import _reduce_model as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
COUNT = 100


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _num_cu(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _key(g, l):
    return ("reduce", g, l, 29, False, False, False)


def _launches(eng, g, l):
    return eng.launch_counts().get(_key(g, l), 0)


def _plan(eng, g, outer, K, inner, forced=0):
    from protocols.secure_comparison_amd.aggregate import reduce_plan

    return reduce_plan(outer, K, inner, _num_cu(eng) * 8 * (64 // g), forced)


def _run(eng, mod, cfg, x, outer, K, inner, label, forced=0):
    """sc_modprod_axis into a guarded output: guards and input intact, one launch per level of the plan; the result as Python ints."""
    g, l = cfg
    rows = outer * inner
    buf = torch.full((rows + 2, mod.nwords), GUARD, dtype=torch.int32, device=eng.device)
    out = buf[1:rows + 1]
    clone = x.clone()
    before = _launches(eng, g, l)
    eng.modprod_axis(mod, x, outer, K, inner, out=out)
    torch.cuda.synchronize()
    assert _launches(eng, g, l) - before == len(_plan(eng, g, outer, K, inner, forced)), (label, "launches per level")
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), (label, "a guard row was written")
    assert torch.equal(x, clone), (label, "the input was modified")
    return eng.download(out)


def _assert_rows(label, got, expect):
    if got != expect:
        bad = [i for i, (a, b) in enumerate(zip(got, expect)) if a != b]
        raise AssertionError(f"{label}: {len(bad)} of {len(expect)} rows differ, first at row {bad[0]}")


def _geometries(ng):
    return [(1, 1, 1), (1, 2, 1), (1, 3, 5), (3, 7, 1), (2, 5, ng - 1), (1, 4, ng), (1, 4, ng + 1), (1, 33, 2 * ng + 3)]


# ---- every compiled instance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", R.INSTANCES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_instance(engine, cfg):
    """Smallest and largest whole-word modulus of the configuration with low limb -1, 1 and random, and a square; operands include
    0, 1, n - 1 and all-ones limbs below n."""
    g, l = cfg
    inst = ("vm", g, l, 29, False, False, False)
    lo, hi = M.size_range(cfg)
    cases = [(f"{bits}-{shape}", M.make_modulus(bits, shape)) for bits in (lo, hi) for shape in ("neg1", "one", "rand")] + \
            [(f"{hi}-square", M.make_modulus(hi, "square"))]
    assert all(M.first_fit(n.bit_length()) == cfg for _, n in cases)
    for ci, (case_label, n) in enumerate(cases):
        mod = engine.modulus(n)
        for gi, (outer, K, inner) in enumerate(_geometries(64 // g)):
            ops = M.operands(n, inst, outer * K * inner, ci + gi)
            if gi % 2:                                  # zeros would blank half of the products: keep them to every other geometry
                ops = [v if v else n - 2 for v in ops]
            random.Random(f"{n & 0xffff}:{gi}").shuffle(ops)
            label = f"{g}x{l}/{case_label}/{(outer, K, inner)}"
            _assert_rows(label, _run(engine, mod, cfg, engine.upload(ops, mod.nwords), outer, K, inner, label),
                         R.prod_axis(n, ops, outer, K, inner))


def test_instance_without_a_kernel_is_refused(engine):
    """A one-lane (1,18) modulus has no k_prod_axis instance: ValueError (SC_ERR_ARG) that names the configuration."""
    n = M.make_modulus(256, "rand")
    assert M.first_fit(256) == (1, 18)
    mod = engine.modulus(n)
    x = engine.upload([3, 5], mod.nwords)
    with pytest.raises(ValueError, match=r"G=1, L=18, W=29"):
        engine.modprod_axis(mod, x, 1, 2, 1)


# ---- the 1024-bit key's N^2 -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n2world(engine, keys):
    sk = oracle_paillier(keys, 1024)
    mod = engine.modulus(sk.n2)
    cfg = M.first_fit(sk.n2.bit_length())
    assert cfg == (4, 18)
    return engine, sk, mod, cfg


DEPTH = [(c, K) for c in (2, 3) for K in (2, 3, 4, 7, 8, 9, 27, 28)] + [(32, 33), (32, 1025)]


@pytest.mark.parametrize("chunk,K", DEPTH)
def test_tree_depth(n2world, chunk, K):
    """A forced chunk length equals the automatic tree and the model, whatever the depth and however short the last chunk."""
    eng, sk, mod, cfg = n2world
    n, outer, inner = sk.n2, 2, 3
    rng = random.Random(f"depth:{chunk}:{K}")
    ops = [rng.randrange(1, n) for _ in range(outer * K * inner)]
    ops[0], ops[-1], ops[len(ops) // 2] = 1, n - 1, (1 << (29 * 72)) % n
    x = eng.upload(ops, mod.nwords)
    expect = R.prod_axis(n, ops, outer, K, inner)
    auto = _run(eng, mod, cfg, x, outer, K, inner, f"auto/{K}")
    try:
        eng.set_reduce_chunk(chunk)
        forced = _run(eng, mod, cfg, x, outer, K, inner, f"chunk {chunk}/{K}", forced=chunk)
    finally:
        eng.set_reduce_chunk(0)
    _assert_rows(f"auto/{K}", auto, expect)
    _assert_rows(f"chunk {chunk}/{K}", forced, expect)


def test_reduce_chunk_range(n2world):
    eng = n2world[0]
    for bad in (1, 33, -1):
        assert eng.lib.sc_ctx_set_reduce_chunk(eng.ctx, bad) == -1
    assert eng.lib.sc_ctx_set_reduce_chunk(eng.ctx, 0) == 0


def test_grid_stride(n2world):
    """More outputs than every resident wave of a full chip holds, K = 2, 257 distinct operands tiled, every row compared."""
    eng, sk, mod, cfg = n2world
    n, ng = sk.n2, 64 // cfg[0]
    outputs = _num_cu(eng) * 16 * ng + ng + 1
    rng = random.Random("grid-stride")
    ops = [rng.randrange(n) for _ in range(M.TILE)]
    rows = eng.upload(ops, mod.nwords)
    x = rows[torch.arange(2 * outputs, device=eng.device) % M.TILE].contiguous()
    # member j of output i is operand (j * outputs + i) mod 257
    prods = eng.upload([ops[t] * ops[(outputs + t) % M.TILE] % n for t in range(M.TILE)], mod.nwords)
    expect = prods[torch.arange(outputs, device=eng.device) % M.TILE]
    buf = torch.full((outputs + 2, mod.nwords), GUARD, dtype=torch.int32, device=eng.device)
    clone = x.clone()
    eng.modprod_axis(mod, x, 1, 2, outputs, out=buf[1:outputs + 1])
    torch.cuda.synchronize()
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()) and torch.equal(x, clone)
    differ = (buf[1:outputs + 1] != expect).any(dim=1)
    assert not bool(differ.any()), f"{int(differ.sum())} of {outputs} rows differ, first at row {int(differ.nonzero()[0])}"


def test_argument_checks_launch_nothing(n2world):
    eng, sk, mod, cfg = n2world
    w = mod.nwords
    buf = eng.upload([3] * 12, w)
    lib, ctx, p = eng.lib, eng.ctx, eng._ptr
    off = lambda rows: torch.Tensor.data_ptr(buf) + rows * w * 4  # noqa: E731
    before, stats = eng.launch_counts(), eng.stats()
    eng._sync_stream()
    assert lib.sc_modprod_axis(ctx, mod.id, None, 1, 2, 1, p(buf)) == -1                      # null pointers
    assert lib.sc_modprod_axis(ctx, mod.id, p(buf), 1, 2, 1, None) == -1
    assert lib.sc_modprod_axis(ctx, 10 ** 6, p(buf), 1, 2, 1, off(8)) == -1                   # no such modulus
    assert lib.sc_modprod_axis(ctx, mod.id, p(buf), 1, 0, 1, off(8)) == -1                    # K = 0
    assert "K must be at least 1" in lib.sc_last_error(ctx).decode()
    for outer, K, inner in ((1 << 39, 4, 1), (1 << 62, 4, 1), (3, 1 << 63, 5), (1 << 20, 1 << 20, 1 << 20)):
        assert lib.sc_modprod_axis(ctx, mod.id, p(buf), outer, K, inner, off(8)) == -1        # past 2^40 words, or wrapping 2^64
        assert "2^40" in lib.sc_last_error(ctx).decode()
    for x_at, out_at in ((0, 0), (0, 3), (0, 7), (2, 0)):                                    # x: 8 rows (2 x 2 x 2), out: 4 rows
        assert lib.sc_modprod_axis(ctx, mod.id, off(x_at), 2, 2, 2, off(out_at)) == -1, (x_at, out_at)
        assert "overlaps" in lib.sc_last_error(ctx).decode()
    assert lib.sc_modprod_axis(ctx, mod.id, p(buf), 0, 2, 1, off(8)) == 0                     # empty: SC_OK, nothing launched
    assert lib.sc_modprod_axis(ctx, mod.id, p(buf), 3, 2, 0, off(8)) == 0
    assert lib.sc_paillier_sum_axis(ctx, 10 ** 6, p(buf), 1, 2, 1, off(8)) == -1              # no such key
    torch.cuda.synchronize()
    assert eng.launch_counts() == before and eng.stats() == stats
    assert eng.download(buf) == [3] * 12
    assert lib.sc_modprod_axis(ctx, mod.id, p(buf), 2, 2, 2, off(8)) == 0                     # adjacent, not overlapping: accepted
    torch.cuda.synchronize()
    assert eng.download(buf) == [3] * 8 + [9] * 4


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(engine, keys):
    from protocols.secure_comparison_amd import DGK, Paillier

    sk, dk = oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16")
    bp = Paillier(sk.n, sk.p, sk.q, engine=engine)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=engine, randomizer_bits=400)
    return engine, sk, bp.public_copy(), bd.public_copy(), bp, bd


def _enc(world, rng, values):
    """Randomized encryptions of `values` (residues modulo N), made on the device: [len][2nw]."""
    engine, sk, ap = world[0], world[1], world[2]
    nw = ap.mod_n.nwords
    return ap.randomize_batch(ap.encrypt_raw_batch(engine.upload([v % sk.n for v in values], nw)),
                              engine.upload([rng.randrange(1, sk.n) for _ in values], nw))


def _dec(world, c, signed=False):
    engine, sk, bp = world[0], world[1], world[4]
    flat = c.reshape(-1, c.shape[-1]).contiguous()
    vals = engine.download(bp.decrypt_raw_batch(flat))
    return [v - sk.n if signed and v > sk.n // 2 else v for v in vals]


def _ints(engine, t):
    return engine.download(t.reshape(-1, t.shape[-1]).contiguous())


def test_both_axes_of_a_non_square_array(world):
    """sum_planes_batch and sum_rows_batch on one [3][10] array against the model on both axes (swapped strides cannot pass), and
    segments of 1, 2 and B rows; re-randomizing keeps the plaintexts."""
    from protocols.secure_comparison_amd.aggregate import sum_planes_batch, sum_rows_batch

    engine, sk, ap = world[0], world[1], world[2]
    rng = random.Random("axes")
    k, B, n2 = 3, 10, sk.n2
    plain = [[rng.randrange(1000) for _ in range(B)] for _ in range(k)]
    x = _enc(world, rng, [v for row in plain for v in row]).reshape(k, B, -1).contiguous()
    flat, clone = _ints(engine, x), x.clone()
    planes = sum_planes_batch(x, ap)
    assert tuple(planes.shape) == (B, x.shape[-1])
    assert _ints(engine, planes) == R.prod_axis(n2, flat, 1, k, B)
    assert _dec(world, planes) == [sum(plain[j][b] for j in range(k)) for b in range(B)]
    rows = sum_rows_batch(x, ap)
    assert tuple(rows.shape) == (k, x.shape[-1])
    assert _ints(engine, rows) == R.prod_axis(n2, flat, k, B, 1)
    assert _dec(world, rows) == [sum(r) for r in plain]
    for seg in (1, 2, B):
        got = sum_rows_batch(x, ap, segment=seg)
        assert tuple(got.shape) == (k, B // seg, x.shape[-1])
        assert _ints(engine, got) == R.prod_axis(n2, flat, k * (B // seg), seg, 1)
        assert _dec(world, got) == [sum(r[s:s + seg]) for r in plain for s in range(0, B, seg)]
    with pytest.raises(ValueError, match="divisor"):
        sum_rows_batch(x, ap, segment=3)
    rho = engine.upload([rng.randrange(1, sk.n) for _ in range(k)], ap.mod_n.nwords)
    fresh = sum_rows_batch(x, ap, rho=rho)
    assert _ints(engine, fresh) == [c * pow(r, sk.n, n2) % n2 for c, r in zip(_ints(engine, rows), engine.download(rho))]
    assert torch.equal(x, clone)


def _hist(rows_of_indices, k):
    """[k][B] counts from indices [m][B]."""
    m, B = len(rows_of_indices), len(rows_of_indices[0])
    return [[sum(1 for q in range(m) if rows_of_indices[q][b] % k == t) for b in range(B)] for t in range(k)]


@pytest.mark.parametrize("k,m,count", [(1, 1, COUNT), (2, 3, COUNT), (3, 5, COUNT), (7, 1, COUNT), (7, 3, COUNT), (7, 5, COUNT), (1000, 3, 3)])
def test_histogram(world, k, m, count):
    from protocols.secure_comparison_amd import secure_histogram_batch
    from protocols.secure_comparison_amd.lookup import default_index_bits

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"hist:{k}:{m}")
    ib = default_index_bits(k)
    idx = [[rng.getrandbits(ib) for _ in range(count)] for _ in range(m)]         # at or above k where ib allows: counted at i mod k
    for q in range(m):
        idx[q][0], idx[q][1] = 0, (k - 1)
    enc = _enc(world, rng, [v for row in idx for v in row]).reshape(m, count, -1).contiguous()
    clone = enc.clone()
    out = secure_histogram_batch(enc, k, ap, bp)
    assert tuple(out.shape) == (k, count, enc.shape[-1]) and torch.equal(enc, clone)
    assert _dec(world, out) == [v for row in _hist(idx, k) for v in row]


@pytest.mark.parametrize("k,m", [(2, 3), (3, 3), (3, 5), (7, 5), (7, 1)])
def test_majority_with_planted_ties(world, k, m):
    """Ties go to the lowest label, as secure_argmax_batch's: rows 0 .. 2 are planted ties."""
    from protocols.secure_comparison_amd import secure_majority_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"vote:{k}:{m}")
    count = COUNT
    labels = [[rng.randrange(k) for _ in range(count)] for _ in range(m)]
    for q in range(m):
        labels[q][0] = (k - 1 - q) % k                     # every label once (or evenly): a tie between all of them
        labels[q][1] = k - 1                               # unanimous for the last label
        labels[q][2] = (k - 1) if q % 2 else (k - 2)       # the two highest labels tie when m is even, else k - 2 leads by one
    enc = _enc(world, rng, [v for row in labels for v in row]).reshape(m, count, -1).contiguous()
    label, top = secure_majority_batch(enc, k, ap, ad, bp, bd)
    hist = _hist(labels, k)
    cols = [[hist[t][b] for t in range(k)] for b in range(count)]
    assert _dec(world, top) == [max(c) for c in cols]
    assert _dec(world, label) == [c.index(max(c)) for c in cols]


@pytest.mark.parametrize("k,count", [(1, COUNT), (2, COUNT), (3, COUNT), (7, COUNT), (1000, 3)])
def test_groupby_count(world, k, count):
    from protocols.secure_comparison_amd import secure_groupby_count_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"gcount:{k}")
    idx = [rng.randrange(k) for _ in range(count)]
    out = secure_groupby_count_batch(_enc(world, rng, idx), k, ap, bp)
    assert tuple(out.shape)[0] == k
    assert _dec(world, out) == [idx.count(t) for t in range(k)]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("k,count", [(1, COUNT), (3, COUNT), (7, COUNT), (1000, 3)])
def test_groupby_sum(world, k, count, signed):
    from protocols.secure_comparison_amd import secure_groupby_sum_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"gsum:{k}:{signed}")
    bits = 20
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    vals = [rng.randint(lo, hi) for _ in range(count)]
    vals[0], vals[1], vals[2] = lo, hi, 0
    idx = [rng.randrange(k) for _ in range(count)]
    v_enc, i_enc = _enc(world, rng, vals), _enc(world, rng, idx)
    cv, ci = v_enc.clone(), i_enc.clone()
    out = secure_groupby_sum_batch(v_enc, i_enc, k, bits, ap, bp, signed=signed)
    assert torch.equal(v_enc, cv) and torch.equal(i_enc, ci)
    assert _dec(world, out, signed) == [sum(v for v, i in zip(vals, idx) if i == t) for t in range(k)]


def test_groupby_sum_refuses_before_any_launch(world):
    from protocols.secure_comparison_amd import secure_groupby_sum_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random("refuse")
    v = _enc(world, rng, [1, 2, 3])
    before = engine.launch_counts()
    with pytest.raises(ValueError, match="does not fit"):
        secure_groupby_sum_batch(v, v, 3, 1021, ap, bp)        # 1021 + bits(3) = 1023 = bits(N) - 1
    assert engine.launch_counts() == before


def test_interleaved_with_the_other_families(world):
    """Sums between calls of the comparison, multiplication, one-hot and inversion families on one context: the temporaries do not
    collide (every sum is compared with the model, every other result decrypted)."""
    from protocols.secure_comparison_amd import secure_multiply_batch, secure_onehot_batch
    from protocols.secure_comparison_amd.aggregate import sum_planes_batch, sum_rows_batch
    from protocols.secure_comparison_amd.selection import secure_minimum_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random("interleave")
    k, B, n2 = 37, 40, sk.n2
    plain = [[rng.randrange(1 << 12) for _ in range(B)] for _ in range(k)]
    x = _enc(world, rng, [v for row in plain for v in row]).reshape(k, B, -1).contiguous()
    flat = _ints(engine, x)
    want_planes, want_rows = R.prod_axis(n2, flat, 1, k, B), R.prod_axis(n2, flat, k, B, 1)
    try:
        engine.set_reduce_chunk(2)                              # six levels: both halves of the temporary in use
        assert _ints(engine, sum_planes_batch(x, ap)) == want_planes
        prod = secure_multiply_batch(x[0], x[1], 12, 12, ap, bp)
        assert _ints(engine, sum_rows_batch(x, ap)) == want_rows
        assert _dec(world, prod) == [a * b for a, b in zip(plain[0], plain[1])]
        hot = secure_onehot_batch(x[2], 5, ap, bp, index_bits=12)
        assert _ints(engine, sum_planes_batch(x, ap)) == want_planes
        assert _dec(world, hot) == [int(v % 5 == t) for t in range(5) for v in plain[2]]
        low, _ = secure_minimum_batch(x[3], x[4], 16, ap, ad, bp, bd)
        assert _ints(engine, sum_rows_batch(x, ap)) == want_rows
        assert _dec(world, low) == [min(a, b) for a, b in zip(plain[3], plain[4])]
        inv = ap.neg_batch(x[5])
        assert _ints(engine, sum_planes_batch(x, ap)) == want_planes
        assert _dec(world, inv, signed=True) == [-v for v in plain[5]]
    finally:
        engine.set_reduce_chunk(0)


# ---- the library's own draws against the replay: one-hot, then multiplication, then comparison -------------------
KEY = bytes((7 * i + 41) & 0xFF for i in range(32))
KAPPA = 40


def _model_onehot(sk, rp, idx, k, ib, B):
    """The rotated one-hot planes [m][k][B] as the model's ciphertexts under the replay's three calls (r, rho_p, Bob's rho_e)."""
    import _onehot_model as omodel

    m, n = len(idx), sk.n
    _, _, M, _ = omodel.layout(KAPPA, ib, k, m, n.bit_length())
    r = rp.bits(ib + KAPPA, m * B, range(m * B))
    rp.below(n, M * B, True, [0])
    rho_e = rp.below(n, m * k * B, True, range(m * k * B))
    out = []
    for q in range(m):
        planes = []
        for t in range(k):
            row = []
            for b in range(B):
                rq = r[q * B + b]
                s = (t + rq) % k
                row.append(omodel.enc(sk, 1 if s == (idx[q][b] + rq) % k else 0, rho_e[(q * k + s) * B + b]))
            planes.append(row)
        out.append(planes)
    return out


def _prod(n2, cs):
    v = 1
    for c in cs:
        v = v * c % n2
    return v


@pytest.fixture()
def seeded_world(world):
    try:
        yield world
    finally:
        world[0].rng_seed(None)


def test_own_draws_histogram_and_majority(seeded_world, keys):
    """Seeded generator, no draws argument.  The histogram is the product over q of the model's rotated one-hot ciphertexts, bit for bit
    (E, the rotation and the sum are pinned through it); the majority continues with the argmax's comparison and selection draws."""
    import _draw_replay as dr
    from oracle import chacha_rng as cr
    from protocols.secure_comparison_amd import secure_histogram_batch, secure_majority_batch
    from protocols.secure_comparison_amd.aggregate import count_bits

    engine, sk, ap, ad, bp, bd = seeded_world
    rng = random.Random("own:hist")
    k, m, ib, B = 4, 3, 2, 5
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    idx[0][0] = idx[1][0] = idx[2][0] = 3
    i_t = _enc(seeded_world, rng, [v for row in idx for v in row]).reshape(m, B, -1).contiguous()
    engine.rng_seed(KEY)
    got = _ints(engine, secure_histogram_batch(i_t, k, ap, bp, index_bits=ib))
    rp = dr.Replay(KEY)
    hot = _model_onehot(sk, rp, idx, k, ib, B)
    want = [[_prod(sk.n2, [hot[q][t][b] for q in range(m)]) for b in range(B)] for t in range(k)]
    assert got == [c for row in want for c in row]
    assert rp.call == 3 and engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(KEY, 3, 64, 4)

    engine.rng_seed(KEY)
    label, top = secure_majority_batch(i_t, k, ap, ad, bp, bd, index_bits=ib)
    d = dr.Driver(sk, oracle_dgk(keys, "dgk_1024_l16"), count_bits(m), 400, KEY)
    d.a.call = 3                                                     # after the one-hot's three calls
    want_top, want_label = d.argext([[want[t][b] for t in range(k)] for b in range(B)], B, range(B), True)
    assert _ints(engine, top) == want_top and _ints(engine, label) == want_label
    assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(KEY, d.calls[0], 64, 4)


@pytest.mark.parametrize("signed", [False, True])
def test_own_draws_groupby_count_and_sum(seeded_world, signed):
    """One-hot draws, then the multiplication's over k B rows; the products and the sums are the model's, bit for bit."""
    import _draw_replay as dr
    from oracle import chacha_rng as cr
    from protocols.secure_comparison_amd import secure_groupby_count_batch, secure_groupby_sum_batch

    engine, sk, ap, ad, bp, bd = seeded_world
    rng = random.Random(f"own:gsum:{signed}")
    k, ib, B, bits = 3, 2, 6, 12
    idx = [rng.randrange(k) for _ in range(B)]
    vals = [rng.randint(-(1 << 11), (1 << 11) - 1) if signed else rng.getrandbits(bits) for _ in range(B)]
    i_t, v_t = _enc(seeded_world, rng, idx), _enc(seeded_world, rng, vals)
    v_c = engine.download(v_t)

    engine.rng_seed(KEY)
    got = engine.download(secure_groupby_count_batch(i_t, k, ap, bp, index_bits=ib))
    rp = dr.Replay(KEY)
    hot = _model_onehot(sk, rp, [idx], k, ib, B)[0]
    assert got == [_prod(sk.n2, hot[t]) for t in range(k)] and rp.call == 3

    engine.rng_seed(KEY)
    got = engine.download(secure_groupby_sum_batch(v_t, i_t, k, bits, ap, bp, signed=signed, index_bits=ib))
    d = dr.Driver(sk, None, 0, 0, KEY)
    d.a.call = 3
    ys = [hot[t][b] for t in range(k) for b in range(B)]
    prods = d.multiply([v_c[b] for t in range(k) for b in range(B)], [ys], range(k * B), k * B, bits, (2 if signed else 1,), signed)[0]
    assert got == [_prod(sk.n2, prods[t * B:(t + 1) * B]) for t in range(k)]
    assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(KEY, d.calls[0], 64, 4)


# ---- two players over a communicator ---------------------------------------------------------------------------------------------------
_HIS = []


def test_players_histogram_majority_groupby_sum(engine, keys):
    import asyncio

    from protocols.secure_comparison_amd import DGK, InMemoryCommunicator, Initiator, KeyHolder, Paillier
    from protocols.secure_comparison_amd.engine import Engine

    sk, dk = oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16")
    if not _HIS:
        _HIS.append(Engine())
    his = _HIS[0]
    bp = Paillier(sk.n, sk.p, sk.q, engine=his)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=his, randomizer_bits=400)
    ap = Paillier(sk.n, engine=engine)
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=600.0)
    alice = Initiator(16, communicator=comm, other_party="keyholder")
    bob = KeyHolder(16, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    w = (engine, sk, ap, None, bp, bd)
    rng = random.Random("players")
    k, m, B, bits = 5, 3, 40, 16
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    vals = [rng.randint(-(1 << 15), (1 << 15) - 1) for _ in range(B)]
    i_t = _enc(w, rng, [v for row in idx for v in row]).reshape(m, B, -1).contiguous()
    v_t = _enc(w, rng, vals)

    async def run():
        hist, _ = await asyncio.gather(alice.perform_secure_histogram_batch(i_t, k, engine=engine), bob.perform_secure_histogram_batch(k, m))
        vote, _ = await asyncio.gather(alice.perform_secure_majority_batch(i_t, k, engine=engine), bob.perform_secure_majority_batch(k, m))
        gsum, _ = await asyncio.gather(alice.perform_secure_groupby_sum_batch(v_t, i_t[0].contiguous(), k, bits, signed=True, engine=engine),
                                       bob.perform_secure_groupby_sum_batch(k, bits, signed=True, count=B))
        return hist, vote, gsum

    hist, (label, top), gsum = asyncio.run(run())

    def dec(t, signed=False):
        out = his.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).to(his.device).contiguous()))
        return [v - sk.n if signed and v > sk.n // 2 else v for v in out]

    counts = _hist(idx, k)
    cols = [[counts[t][b] for t in range(k)] for b in range(B)]
    assert dec(hist) == [v for row in counts for v in row]
    assert dec(top) == [max(c) for c in cols] and dec(label) == [c.index(max(c)) for c in cols]
    assert dec(gsum, True) == [sum(v for v, i in zip(vals, idx[0]) if i == t) for t in range(k)]


# ---- compositions under injected draws: every intermediate against the models (tests/_onehot_model.py, tests/_mult_model.py) --------------
def _sample_rows(count):
    return sorted(set(range(min(3, count))) | set(range(max(0, count - 2), count)))


def _onehot_draws(world, rng, ib, k, m, count):
    """Per-row model draws (rs [m], rho_ps [M], rho_es [m][k]) and the same as OnehotDraws arrays."""
    import _onehot_model as omodel
    from protocols.secure_comparison_amd import OnehotDraws, OnehotLayout

    engine, sk, ap = world[0], world[1], world[2]
    n, nw = sk.n, ap.mod_n.nwords
    lay = OnehotLayout(KAPPA, ib, k, m, n.bit_length())
    top = (1 << (ib + KAPPA)) - 1
    draws = []
    for b in range(count):
        rs, rho_ps, rho_es = omodel.draw(rng, KAPPA, ib, k, m, n)
        if b < 2:
            rs = [0 if b == 0 else top] * m                # the ends of the mask range
        draws.append((rs, rho_ps, rho_es))
    plane = lambda vals, w: engine.upload(vals, w)  # noqa: E731
    md = OnehotDraws(r=torch.stack([plane([d[0][q] for d in draws], lay.rw) for q in range(m)]).contiguous(),
                     rho_p=torch.stack([plane([d[1][mm] for d in draws], nw) for mm in range(lay.M)]).contiguous(),
                     rho_e=torch.stack([torch.stack([plane([d[2][q][t] for d in draws], nw) for t in range(k)]) for q in range(m)]).contiguous())
    return lay, draws, md


def _check_onehot_steps(world, lay, i_c, i_t, draws, md, idx):
    """onehot_pack / onehot_answer / onehot_finish beside the composition, with the same draws: P, E and the rotated planes against
    the model on the sampled rows (the hot position, its neighbour, both ends, the index's own position; and what rotates onto them),
    E and the rotated planes decrypted on every row.  Returns the rotated planes as integers, [m][k][count] flat."""
    import _onehot_model as omodel
    from protocols.secure_comparison_amd.lookup import onehot_answer, onehot_finish, onehot_pack

    engine, sk, ap, bp = world[0], world[1], world[2], world[4]
    k, m, ib, count, nbits = lay.k, lay.m, lay.ib, i_t.shape[1], sk.n.bit_length()
    P, rot = onehot_pack(lay, i_t, md, ap)
    E = onehot_answer(lay, P, bp, md.rho_e)
    out = onehot_finish(lay, E, rot, ap)
    got_P, got_E, got_out = _ints(engine, P), _ints(engine, E), _ints(engine, out)
    hot = [[(idx[q][b] + draws[b][0][q]) % k for b in range(count)] for q in range(m)]
    assert _dec(world, E) == [1 if t == hot[q][b] else 0 for q in range(m) for t in range(k) for b in range(count)]
    assert _dec(world, out) == [1 if t == idx[q][b] % k else 0 for q in range(m) for t in range(k) for b in range(count)]
    for b in _sample_rows(count):
        rs, rho_ps, rho_es = draws[b]
        _, rots = omodel.plain(KAPPA, ib, k, m, nbits, rs)
        assert rot[:, b].cpu().tolist() == rots
        want_P = omodel.pack(sk, KAPPA, ib, k, [i_c[q][b] for q in range(m)], rs, rho_ps)
        assert [got_P[mm * count + b] for mm in range(lay.M)] == want_P, b
        ts = {q: sorted({0, k - 1, hot[q][b], (hot[q][b] + 1) % k, idx[q][b] % k}) for q in range(m)}
        only = sorted({(q, t) for q in range(m) for t in ts[q]} | {(q, (t + rots[q]) % k) for q in range(m) for t in ts[q]})
        mE, _, mj, bad = omodel.answer(sk, KAPPA, ib, k, m, want_P, rho_es, only)
        assert not bad and mj == [hot[q][b] for q in range(m)]
        assert all(got_E[(q * k + t) * count + b] == c for (q, t), c in mE.items()), b
        assert all(got_out[(q * k + t) * count + b] == mE[(q, (t + rots[q]) % k)] for q in range(m) for t in ts[q]), b
    return got_out


INJECTED = [(k, m, COUNT) for k in (1, 2, 3, 7) for m in (1, 3, 5)] + [(1000, 3, 3)]


@pytest.mark.parametrize("k,m,count", INJECTED)
def test_histogram_and_majority_under_injected_draws(world, k, m, count):
    """draws= handed in: P, E and the rotated one-hot against the model, the histogram bit for bit the product over q of the rotated
    planes and decrypted on every row; the majority on the same draws decrypted (its comparison draws are the library's)."""
    from protocols.secure_comparison_amd import secure_histogram_batch, secure_majority_batch
    from protocols.secure_comparison_amd.lookup import default_index_bits

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"inj:hist:{k}:{m}")
    ib = default_index_bits(k)
    idx = [[rng.getrandbits(ib) for _ in range(count)] for _ in range(m)]
    for q in range(m):
        idx[q][0], idx[q][1], idx[q][2] = 0, (k - 1), (1 << ib) - 1        # the last one at or above k where ib allows
    i_t = _enc(world, rng, [v for row in idx for v in row]).reshape(m, count, -1).contiguous()
    flat = _ints(engine, i_t)
    i_c = [flat[q * count:(q + 1) * count] for q in range(m)]
    lay, draws, md = _onehot_draws(world, rng, ib, k, m, count)
    hot = _check_onehot_steps(world, lay, i_c, i_t, draws, md, idx)
    clone = i_t.clone()
    out = secure_histogram_batch(i_t, k, ap, bp, index_bits=ib, draws=md)
    assert torch.equal(i_t, clone)
    assert _ints(engine, out) == [_prod(sk.n2, [hot[(q * k + t) * count + b] for q in range(m)]) for t in range(k) for b in range(count)]
    counts = _hist(idx, k)
    assert _dec(world, out) == [v for row in counts for v in row]
    if k <= 7:
        label, top = secure_majority_batch(i_t, k, ap, ad, bp, bd, index_bits=ib, draws=md)
        cols = [[counts[t][b] for t in range(k)] for b in range(count)]
        assert _dec(world, top) == [max(c) for c in cols] and _dec(world, label) == [c.index(max(c)) for c in cols]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("k,count", [(1, COUNT), (2, COUNT), (3, COUNT), (7, COUNT), (1000, 3)])
def test_groupby_under_injected_draws(world, k, count, signed):
    """draws= and mul_draws= handed in: the one-hot steps and mul_batch's products against the models beside the composition, the
    group-by count and sum bit for bit the products over the rows of those intermediates, every output decrypted."""
    import _mult_model as mmodel
    from protocols.secure_comparison_amd import secure_groupby_count_batch, secure_groupby_sum_batch
    from protocols.secure_comparison_amd.aggregate import groupby_sum_layout
    from protocols.secure_comparison_amd.lookup import default_index_bits
    from protocols.secure_comparison_amd.multiplication import MulDraws, mul_batch

    engine, sk, ap, ad, bp, bd = world
    rng = random.Random(f"inj:gsum:{k}:{signed}")
    n, n2, nw, bits, ib = sk.n, sk.n2, ap.mod_n.nwords, 20, default_index_bits(k)
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    vals = [rng.randint(lo, hi) for _ in range(count)]
    vals[0], vals[1], vals[2] = lo, hi, 0
    idx = [rng.getrandbits(ib) for _ in range(count)]
    idx[0], idx[1] = 0, k - 1
    v_t, i_t = _enc(world, rng, vals), _enc(world, rng, idx)
    v_c, i_c = engine.download(v_t), engine.download(i_t)
    lay, draws, md = _onehot_draws(world, rng, ib, k, 1, count)
    hot = _check_onehot_steps(world, lay, [i_c], i_t.unsqueeze(0).contiguous(), draws, md, [idx])          # [k][count] flat

    got = secure_groupby_count_batch(i_t, k, ap, bp, index_bits=ib, draws=md)
    assert engine.download(got) == [_prod(n2, hot[t * count:(t + 1) * count]) for t in range(k)]
    assert _dec(world, got) == [sum(1 for i in idx if i % k == t) for t in range(k)]

    mul = groupby_sum_layout(bits, count, signed, KAPPA, ap)
    wx, wy, rows = mul.wx, mul.wy, k * count
    mdraws = [mmodel.draw(rng, KAPPA, wx, wy, n) for _ in range(rows)]
    aw, bw = (wx + KAPPA + 31) // 32, (max(wy) + KAPPA + 31) // 32
    mm = MulDraws(r_a=engine.upload([d[0] for d in mdraws], aw), r_b=engine.upload([d[1][0] for d in mdraws], bw).unsqueeze(0).contiguous(),
                  rho_p=engine.upload([d[2] for d in mdraws], nw), rho_products=engine.upload([d[3][0] for d in mdraws], nw).unsqueeze(0).contiguous())
    x = v_t.unsqueeze(0).expand(k, count, v_t.shape[-1]).reshape(rows, -1).contiguous()
    y = engine.upload(hot, 2 * nw)
    products = engine.download(mul_batch(mul, x, y, ap, bp, mm)[0])
    sample = sorted({t * count + b for t in sorted({0, k - 1, idx[0] % k}) for b in _sample_rows(count)})
    for r in sample:
        assert products[r] == mmodel.multiply_enc(sk, KAPPA, wx, wy, signed, v_c[r % count], [hot[r]], mdraws[r])[0], r
    plain = [vals[r % count] * (1 if idx[r % count] % k == r // count else 0) for r in range(rows)]
    assert _dec(world, engine.upload(products, 2 * nw), signed) == plain

    cv, ci = v_t.clone(), i_t.clone()
    out = secure_groupby_sum_batch(v_t, i_t, k, bits, ap, bp, signed=signed, index_bits=ib, draws=md, mul_draws=mm)
    assert torch.equal(v_t, cv) and torch.equal(i_t, ci)
    assert engine.download(out) == [_prod(n2, products[t * count:(t + 1) * count]) for t in range(k)]
    assert _dec(world, out, signed) == [sum(v for v, i in zip(vals, idx) if i % k == t) for t in range(k)]

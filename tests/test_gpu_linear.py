"""Linear maps with public weights along an axis (sc_modlin_axis / k_lin_axis) and the Python layer on it, on the GPU.
Every residue is compared bit for bit with plain Python (tests/_linear_model.py): every compiled instance at the ends of its
configuration's range with padded last blocks on both axes, weight rows of every kind in one matrix, the grid-stride loop, the refusals
with nothing launched, and linear_planes_batch / linear_rows_batch decrypted on every row and compared with the route that existed.
Outputs sit between guard rows and inputs are compared with their clones afterwards."""
import ctypes
import os
import random
import sys

import pytest
import torch

from conftest import oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _instance_matrix as M  # noqa: E402
import _linear_model as LM  # noqa: E402
import _reduce_model as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
COUNT = 100
KS, JS = (1, 2, 3, 7, 33), (1, 2, 5)


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _num_cu(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _launches(eng, g, l):
    c = eng.launch_counts()
    return c.get(("lift", g, l, 29, False, False, False), 0), c.get(("lin", g, l, 29, False, False, False), 0)


def _run(eng, mod, cfg, x, outer, K, inner, W, label):
    """sc_modlin_axis into a guarded output: guards and input intact, one lift and one k_lin_axis launch; the result as Python ints."""
    g, l = cfg
    rows = outer * len(W) * inner
    buf = torch.full((rows + 2, mod.nwords), GUARD, dtype=torch.int32, device=eng.device)
    clone = x.clone()
    before = _launches(eng, g, l)
    eng.modlin_axis(mod, x, outer, K, inner, W, out=buf[1:rows + 1])
    torch.cuda.synchronize()
    after = _launches(eng, g, l)
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1), (label, "one lift launch and one k_lin_axis launch per call")
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), (label, "a guard row was written")
    assert torch.equal(x, clone), (label, "the input was modified")
    return eng.download(buf[1:rows + 1])


def _assert_rows(label, got, expect):
    if got != expect:
        bad = [i for i, (a, b) in enumerate(zip(got, expect)) if a != b]
        raise AssertionError(f"{label}: {len(bad)} of {len(expect)} rows differ, first at row {bad[0]}")


# ---- every compiled instance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("end", ("smallest", "largest"))
@pytest.mark.parametrize("cfg", R.INSTANCES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_instance(engine, cfg, end):
    """The smallest or the largest modulus of the configuration with low limb -1, 1 and random; outer * inner in {1, NG - 1, NG, NG + 1,
    2 NG + 3} split as (outer, 1) and as (1, inner), so that the last block of every row j is padded on either axis, three of the nine
    geometries per modulus; every K of KS and every J of JS (the fifteen pairs over the two ends), the J rows taken from one matrix of
    all five kinds; then, at every K, all five kinds in one launch (J = 5), so that rowbits differs between rows that share it.
    Operands include 0, 1, n - 1 and all-ones limbs below n."""
    g, l = cfg
    ng = 64 // g
    inst = ("vm", g, l, 29, False, False, False)
    bits = M.size_range(cfg)[end == "largest"]
    cases = [(f"{bits}-{shape}", M.make_modulus(bits, shape)) for shape in ("neg1", "one", "rand")]
    assert all(M.first_fit(n.bit_length()) == cfg for _, n in cases)
    shapes = [(t, 1) for t in (1, ng - 1, ng, ng + 1, 2 * ng + 3)] + [(1, t) for t in (ng - 1, ng, ng + 1, 2 * ng + 3)]
    runs = []
    for t, (outer, inner) in enumerate(shapes if end == "smallest" else shapes[::-1]):
        step = t + (6 if end == "largest" else 0)                                   # steps 0 .. 8 and 6 .. 14: the fifteen (K, J) pairs
        runs.append((cases[t // 3], outer, inner, KS[step % 5], JS[step % 3], step))
    runs += [(cases[2], *shapes[(2 * t + 4) % 9], K, 5, 20 + t) for t, K in enumerate(KS)]      # K = 33 on (NG + 1, 1): a padded block
    assert {r[3] for r in runs[:9]} == set(KS) and {r[4] for r in runs[:9]} == set(JS)
    for ri, ((case_label, n), outer, inner, K, J, step) in enumerate(runs):
        mod = engine.modulus(n)
        W = LM.matrix(K, J, salt=step)
        ops = M.operands(n, inst, outer * K * inner, step)
        if ri % 2:                                      # zeros would blank half of the outputs: keep them to every other run
            ops = [v if v else n - 2 for v in ops]
        random.Random(f"{n & 0xffff}:{ri}").shuffle(ops)
        label = f"{g}x{l}/{case_label}/{(outer, K, inner)}/J={J}"
        _assert_rows(label, _run(engine, mod, cfg, engine.upload(ops, mod.nwords), outer, K, inner, W, label),
                     LM.lin_axis(n, ops, outer, K, inner, W))


def test_single_one_returns_the_member_and_zero_row_one(engine):
    n = M.make_modulus(2048, "rand")
    cfg = M.first_fit(2048)
    mod = engine.modulus(n)
    ops = M.operands(n, ("vm",) + cfg + (29, False, False, False), 3 * 5, 1)
    got = _run(engine, mod, cfg, engine.upload(ops, mod.nwords), 1, 3, 5, [[0, 0, 0], [0, 1, 0], [0, 0, 1]], "identity")
    assert got == [1] * 5 + ops[5:10] + ops[10:15]


def test_instance_without_a_kernel_is_refused(engine):
    """A one-lane (1,18) modulus has no k_lin_axis instance: ValueError (SC_ERR_ARG) that names the configuration, nothing launched."""
    n = M.make_modulus(256, "rand")
    assert M.first_fit(256) == (1, 18)
    mod = engine.modulus(n)
    x = engine.upload([3, 5], mod.nwords)
    before = engine.launch_counts()
    with pytest.raises(ValueError, match=r"sc_modlin_axis.*k_lin_axis.*G=1, L=18, W=29"):
        engine.modlin_axis(mod, x, 1, 2, 1, [[1, 1]])
    assert engine.launch_counts() == before


# ---- the 1024-bit key's N^2 -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n2world(engine, keys):
    sk = oracle_paillier(keys, 1024)
    mod = engine.modulus(sk.n2)
    cfg = M.first_fit(sk.n2.bit_length())
    assert cfg == (4, 18)
    return engine, sk, mod, cfg


def test_grid_stride(engine):
    """A small modulus and more waves than every resident slot of a full chip holds: K = 2, J = 2, 257 distinct operands tiled, every
    row compared; the two rows differ in rowbits."""
    cfg = (2, 18)
    lo, _ = M.size_range(cfg)
    n = M.make_modulus(lo, "rand")
    mod = engine.modulus(n)
    ng = 64 // cfg[0]
    pairs = _num_cu(engine) * 16 * ng + ng + 1          # per row j; the launcher clamps the resident waves per CU to 16
    W = [[3, 0x10001], [1, 2]]
    rng = random.Random("grid-stride")
    ops = [rng.randrange(n) for _ in range(M.TILE)]
    rows = engine.upload(ops, mod.nwords)
    x = rows[torch.arange(2 * pairs, device=engine.device) % M.TILE].contiguous()
    # member k of pair i is operand (k * pairs + i) mod 257
    tiles = [engine.upload([pow(ops[t], w[0], n) * pow(ops[(pairs + t) % M.TILE], w[1], n) % n for t in range(M.TILE)], mod.nwords) for w in W]
    at = torch.arange(pairs, device=engine.device) % M.TILE
    expect = torch.cat([tiles[0][at], tiles[1][at]])
    buf = torch.full((2 * pairs + 2, mod.nwords), GUARD, dtype=torch.int32, device=engine.device)
    clone = x.clone()
    engine.modlin_axis(mod, x, 1, 2, pairs, W, out=buf[1:2 * pairs + 1])
    torch.cuda.synchronize()
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()) and torch.equal(x, clone)
    differ = (buf[1:2 * pairs + 1] != expect).any(dim=1)
    assert not bool(differ.any()), f"{int(differ.sum())} of {2 * pairs} rows differ, first at row {int(differ.nonzero()[0])}"


def test_argument_checks_launch_nothing(n2world):
    eng, sk, mod, cfg = n2world
    w = mod.nwords
    buf = eng.upload([3] * 16, w)
    lib, ctx, p = eng.lib, eng.ctx, eng._ptr
    off = lambda rows: torch.Tensor.data_ptr(buf) + rows * w * 4  # noqa: E731
    wt = (ctypes.c_uint64 * 4)(1, 1, 2, 0)
    big = (ctypes.c_uint64 * (1025 * 2))()
    err = lambda: lib.sc_last_error(ctx).decode()  # noqa: E731
    before, stats = eng.launch_counts(), eng.stats()
    eng._sync_stream()
    call = lib.sc_modlin_axis
    assert call(ctx, mod.id, None, 1, 2, 1, wt, 2, off(8)) == -1                             # null pointers
    assert call(ctx, mod.id, p(buf), 1, 2, 1, None, 2, off(8)) == -1
    assert call(ctx, mod.id, p(buf), 1, 2, 1, wt, 2, None) == -1
    assert call(ctx, 10 ** 6, p(buf), 1, 2, 1, wt, 2, off(8)) == -1                          # no such modulus
    for args, name in (((0, 2, 1, wt, 2), "outer"), ((1, 0, 1, wt, 2), "K"), ((1, 2, 0, wt, 2), "inner"), ((1, 2, 1, wt, 0), "J")):
        assert call(ctx, mod.id, p(buf), *args, off(8)) == -1 and name in err(), name         # a zero size
    assert call(ctx, mod.id, p(buf), 1, 1025, 1, big, 2, off(8)) == -1 and "K = 1025" in err()
    assert call(ctx, mod.id, p(buf), 1, 2, 1, big, 1025, off(8)) == -1 and "J = 1025" in err()
    for outer, K, inner, J in ((1 << 39, 4, 1, 1), (1 << 62, 1, 1, 4), (3, 1, 1 << 63, 5), (1 << 20, 1, 1 << 20, 1024)):
        assert call(ctx, mod.id, p(buf), outer, K, inner, big, J, off(8)) == -1 and "2^40" in err()   # past 2^40 words, or wrapping
    for x_at, out_at in ((0, 0), (0, 3), (0, 7), (4, 0), (7, 0)):                            # x: 8 rows (2 x 2 x 2), out: 8 rows (2 x 2 x 2)
        assert call(ctx, mod.id, off(x_at), 2, 2, 2, wt, 2, off(out_at)) == -1, (x_at, out_at)
        assert "overlaps" in err()
    assert lib.sc_paillier_linear_axis(ctx, 10 ** 6, p(buf), 1, 2, 1, wt, 2, off(8)) == -1    # no such key
    torch.cuda.synchronize()
    assert eng.launch_counts() == before and eng.stats() == stats
    assert eng.download(buf) == [3] * 16
    assert call(ctx, mod.id, p(buf), 2, 2, 2, wt, 2, off(8)) == 0                            # adjacent, not overlapping: accepted
    wt[0] = wt[1] = wt[2] = wt[3] = 0                                                        # the host array is free on return
    torch.cuda.synchronize()
    assert eng.download(buf) == [3] * 8 + [9, 9, 9, 9] * 2
    with pytest.raises(ValueError):
        eng.modlin_axis(mod, buf[:4], 1, 2, 2, [[1, 2, 3]])                                  # a ragged matrix never reaches the library
    with pytest.raises(ValueError):
        eng.modlin_axis(mod, buf[:4], 1, 2, 2, [[1, 1 << 64]])


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(engine, keys):
    from protocols.secure_comparison_amd import Paillier

    sk = oracle_paillier(keys, 1024)
    bp = Paillier(sk.n, sk.p, sk.q, engine=engine)
    return engine, sk, bp.public_copy(), bp


def _enc(world, rng, values):
    engine, sk, ap = world[0], world[1], world[2]
    nw = ap.mod_n.nwords
    return ap.randomize_batch(ap.encrypt_raw_batch(engine.upload([v % sk.n for v in values], nw)),
                              engine.upload([rng.randrange(1, sk.n) for _ in values], nw))


def _dec(world, c):
    engine, sk, bp = world[0], world[1], world[3]
    vals = engine.download(bp.decrypt_raw_batch(c.reshape(-1, c.shape[-1]).contiguous()))
    return [v - sk.n if v > sk.n // 2 else v for v in vals]


def _ints(engine, t):
    return engine.download(t.reshape(-1, t.shape[-1]).contiguous())


def _existing_route(world, x, W, bias):
    """scalar_mul_batch per (output, plane) on the plane or its inverse, sum_planes_batch per output, add_batch of the unrandomized bias."""
    from protocols.secure_comparison_amd.aggregate import sum_planes_batch

    engine, sk, ap = world[0], world[1], world[2]
    K, B, w = x.shape
    minus = ap.neg_batch(x.reshape(K * B, w)).reshape(K, B, w)
    out = []
    for j, row in enumerate(W):
        terms = [ap.scalar_mul_batch((x if wk >= 0 else minus)[k].contiguous(), engine.upload([abs(wk)] * B, 2), 64) for k, wk in enumerate(row)]
        total = sum_planes_batch(torch.stack(terms), ap)
        out.append(ap.add_batch(total, ap.encrypt_raw_batch(engine.upload([bias[j] % sk.n] * B, ap.mod_n.nwords))))
    return torch.stack(out)


def test_planes_signed_with_bias(world):
    """COUNT rows, signed weights and bias: the decryption equals W x + b on every row, the residues equal the existing route's bit
    for bit before re-randomization, rho changes every output and no plaintext."""
    from protocols.secure_comparison_amd import linear_planes_batch

    engine, sk, ap = world[0], world[1], world[2]
    rng, K = random.Random("planes"), 4
    plain = [[rng.randrange(-(1 << 20), 1 << 20) for _ in range(COUNT)] for _ in range(K)]
    W = [[3, -5, 0, 1], [0, 0, 0, 0], [-(1 << 64) + 1, (1 << 64) - 1, 1 << 63, -1], [0, 0, 1, 0], [rng.randrange(-(1 << 16), 1 << 16) for _ in range(K)]]
    bias = [7, -7, 1 << 80, -(1 << 80), 0]
    x = _enc(world, rng, [v for row in plain for v in row]).reshape(K, COUNT, -1).contiguous()
    clone = x.clone()
    out = linear_planes_batch(x, W, ap, bias=bias, x_bits=21)
    assert tuple(out.shape) == (len(W), COUNT, x.shape[-1]) and torch.equal(x, clone)
    assert _dec(world, out) == [v for row in LM.signed_map(W, bias, plain) for v in row]
    assert torch.equal(out, _existing_route(world, x, W, bias))
    rho = engine.upload([rng.randrange(1, sk.n) for _ in range(len(W) * COUNT)], ap.mod_n.nwords).reshape(len(W), COUNT, -1)
    fresh = linear_planes_batch(x, W, ap, bias=bias, rho=rho)
    assert bool((fresh != out).any(dim=-1).all()) and _dec(world, fresh) == _dec(world, out)
    assert _ints(engine, fresh) == [c * pow(r, sk.n, sk.n2) % sk.n2 for c, r in zip(_ints(engine, out), _ints(engine, rho))]
    with pytest.raises(ValueError, match=r"row 2\b"):
        linear_planes_batch(x, W, ap, x_bits=sk.n.bit_length() - 68)                     # row 2 sums to 66 bits: one bit too many
    assert torch.equal(x, clone)


def test_rows_with_and_without_segment(world):
    from protocols.secure_comparison_amd import linear_rows_batch

    engine, sk, ap = world[0], world[1], world[2]
    rng, P, B = random.Random("rows"), 3, 12
    plain = [[rng.randrange(-1000, 1000) for _ in range(B)] for _ in range(P)]
    x = _enc(world, rng, [v for row in plain for v in row]).reshape(P, B, -1).contiguous()
    clone = x.clone()
    for seg in (None, 1, 3, 4, 12):
        s = B if seg is None else seg
        W = [[rng.randrange(-(1 << 30), 1 << 30) for _ in range(s)], [0] * s, [1] * s]
        bias = [-4, 9, 0]
        out = linear_rows_batch(x, W, ap, segment=seg, bias=bias)
        assert tuple(out.shape) == (P,) + (() if seg is None else (B // s,)) + (3, x.shape[-1])
        assert _dec(world, out) == [sum(w * v for w, v in zip(row, plain[p][t:t + s])) + b for p in range(P) for t in range(0, B, s)
                                    for row, b in zip(W, bias)]
    with pytest.raises(ValueError, match="divisor"):
        linear_rows_batch(x, [[1] * 5], ap, segment=5)
    assert torch.equal(x, clone)


def test_2048_bit_key(engine, keys):
    from protocols.secure_comparison_amd import Paillier, linear_planes_batch

    sk = oracle_paillier(keys, 2048)
    bp = Paillier(sk.n, sk.p, sk.q, engine=engine)
    w2048 = (engine, sk, bp.public_copy(), bp)
    rng, K, J, B = random.Random("2048"), 5, 3, 9
    plain = [[rng.randrange(-(1 << 30), 1 << 30) for _ in range(B)] for _ in range(K)]
    W = [[rng.randrange(-(1 << 64) + 1, 1 << 64) for _ in range(K)] for _ in range(J)]
    bias = [rng.randrange(-(1 << 90), 1 << 90) for _ in range(J)]
    x = _enc(w2048, rng, [v for row in plain for v in row]).reshape(K, B, -1).contiguous()
    out = linear_planes_batch(x, W, w2048[2], bias=bias, x_bits=31)
    assert _dec(w2048, out) == [v for row in LM.signed_map(W, bias, plain) for v in row]
    members, Wp = LM.split_signed(W)
    flat = _ints(engine, x)
    ops = [flat[k * B + b] if not neg else pow(flat[k * B + b], -1, sk.n2) for k, neg in members for b in range(B)]
    want = [c * (1 + (bj % sk.n) * sk.n) % sk.n2 for c, bj in zip(LM.lin_axis(sk.n2, ops, 1, len(members), B, Wp), [bj for bj in bias for _ in range(B)])]
    assert _ints(engine, out) == want

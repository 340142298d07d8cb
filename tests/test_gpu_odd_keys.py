"""The families on Paillier keys that do not fill their words (tests/golden/keys_odd.json; conditions, instances and widths from
tests/_odd_keys.py), on the GPU: N with a partial top word, N^2 with a zero top word that the whole-words rule moves to another
configuration, N on an L = 27 configuration reached through its L = 14 pair twin, primes of unequal length and unequal words.

Every residue is compared with Python integers or with the existing pure-Python models, on every row (batches of at most 24 rows,
1 and NG + 1 of the instance N^2 runs on); outputs sit between guard rows where a call takes `out=`, inputs are compared with clones,
and the launch counters must show the instances tests/_odd_keys.py predicts -- no others."""
import asyncio
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _draw_replay as dr  # noqa: E402
import _linear_model as LM  # noqa: E402
import _odd_keys as K  # noqa: E402
import _reduce_model as R  # noqa: E402
import _scan_model as S  # noqa: E402
import _select_model as smodel  # noqa: E402
import test_gpu_aggregate as tagg  # noqa: E402
import test_gpu_dot as tdot  # noqa: E402
import test_gpu_instance_matrix as tim  # noqa: E402
import test_gpu_lookup as tlook  # noqa: E402
import test_gpu_mult as tmul  # noqa: E402
import test_gpu_pipelines as tpipe  # noqa: E402
import test_gpu_scan as tscan  # noqa: E402
import test_gpu_select as tsel  # noqa: E402
import test_gpu_topk as ttopk  # noqa: E402
from oracle import chacha_rng as cr  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = K.load()
SIZES = sorted(KEYS)
COMPARED = (1025, 1100)           # the keys of the comparison-based families (DGK: dgk_1024_l16, l = 16)
L = 16


def _schemes(engine, bits, **kw):
    from protocols.secure_comparison_amd import Paillier

    k = KEYS[bits]
    bob = Paillier(k.n, k.p, k.q, engine=engine, **kw)
    return k.oracle(), bob.public_copy(), bob


def _with_odd(keys, bits):
    """The golden keys and this odd key under the name the existing helpers look up (conftest.oracle_paillier)."""
    k = KEYS[bits]
    return {**keys, f"paillier_{bits}": {"p": hex(k.p), "q": hex(k.q)}}


class _PoliciesOff:
    """Small-batch and one-lane policies off, so that the instance of a call follows from the modulus alone."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_latency_mode(0)
        self.eng.set_onelane_mode(0)

    def __exit__(self, *exc):
        self.eng.set_onelane_mode(1)
        self.eng.set_fork_mode(1)


def _interpreter_launches(eng, before):
    return {k for k in tim._grew(eng, before) if k[0] in ("vm", "pvm")}


def _assert_launched(eng, before, ins, call, label):
    """The interpreter instances that grew are exactly the predicted ones of this call."""
    grew = _interpreter_launches(eng, before)
    assert grew == ins[call], (label, call, "not run", sorted(ins[call] - grew), "not predicted", sorted(grew - ins[call]))


# ---- Paillier --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", SIZES)
def test_paillier_primitives_and_their_instances(engine, bits):
    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    n, n2, nw = key.n, key.n2, key.nw
    ins = K.instances(key)
    assert (ap.mod_n.nwords, ap.mod_n2.nwords) == (nw, 2 * nw)
    rng = random.Random(bits)
    up = engine.upload
    bobs = {(crt, pairs): _schemes(engine, bits, use_crt=crt, use_pairs=pairs)[2] for crt in (True, False) for pairs in (True, False)}
    with _PoliciesOff(engine):
        for ci, count in enumerate(K.batch_sizes(key)):
            tag = f"{bits}[{count}]"
            ms = ([0, 1, n - 1, n - 2, (1 << (bits - 1)) - 1][ci:] + [rng.randrange(n) for _ in range(count)])[:count]
            rhos = ([1, n - 1, 2][ci:] + [rng.randrange(1, n) for _ in range(count)])[:count]
            tm_, tr = up(ms, nw), up(rhos, nw)
            want_c = [sk.enc_raw(m) for m in ms]
            tim._check(engine, f"{tag} encrypt_raw", want_c, lambda o: engine.paillier_encrypt(ap.key, tm_, out=o), count, 2 * nw, m=tm_)
            tim._check(engine, f"{tag} encrypt_raw_neg", [pow(c, -1, n2) for c in want_c],
                       lambda o: engine.paillier_encrypt(ap.key, tm_, negate=True, out=o), count, 2 * nw, m=tm_)
            want_r = [pow(r, n, n2) for r in rhos]
            for who, scheme, call in (("public", ap, "randomizer_public"), ("key holder", bp, "randomizer_crt")):
                before = engine.launch_counts()
                tim._check(engine, f"{tag} randomizer ({who})", want_r, lambda o: engine.paillier_randomize(scheme.key, None, tr, out=o), count, 2 * nw, rho=tr)
                _assert_launched(engine, before, ins, call, tag)
            # ciphertexts: N^2 - 1 and 1 + (N - 1) N (the largest unrandomized one) first, then randomized encryptions
            cs = ([n2 - 1, 1 + (n - 1) * n][ci:] + [c * r % n2 for c, r in zip(want_c, want_r)])[:count]
            tc = up(cs, 2 * nw)
            for who, scheme in (("public", ap), ("key holder", bp)):
                tim._check(engine, f"{tag} randomize ({who})", [c * r % n2 for c, r in zip(cs, want_r)],
                           lambda o: engine.paillier_randomize(scheme.key, tc, tr, out=o), count, 2 * nw, c=tc, rho=tr)
            assert torch.equal(ap.randomizer_batch(tr), bp.randomizer_batch(tr)) and engine.download(ap.randomize_batch(tc, tr)) == [c * r % n2 for c, r in zip(cs, want_r)]
            # decryption: CRT on / off, pairs on / off, every fork mode
            want_m = [sk.dec_raw(c) for c in cs]
            assert want_m[len([n2 - 1, 1 + (n - 1) * n][ci:]):] == ms[:count - len([n2 - 1, 1 + (n - 1) * n][ci:])]
            for use_crt in (True, False):
                for use_pairs in (True, False):
                    bob = bobs[(use_crt, use_pairs)]
                    call = "decrypt_" + ("crt" if use_crt else "no_crt") + ("" if use_pairs else "_no_pairs")
                    for fork in ((0, 1, 2) if use_crt else (1,)):
                        engine.set_fork_mode(fork)
                        clone = tc.clone()
                        before = engine.launch_counts()
                        got = engine.download(bob.decrypt_raw_batch(tc))
                        assert got == want_m, (tag, call, fork)
                        assert torch.equal(tc, clone)
                        _assert_launched(engine, before, ins, call, f"{tag} fork {fork}")
                        if use_crt:
                            assert engine.download(bob.randomizer_batch(tr)) == want_r, (tag, call, fork, "randomizer")
                    engine.set_fork_mode(1)
            # the homomorphisms
            others = cs[::-1]
            to = up(others, 2 * nw)
            tim._check(engine, f"{tag} add", [a * b % n2 for a, b in zip(cs, others)], lambda o: engine.modmul(ap.mod_n2, tc, to, out=o), count, 2 * nw, a=tc, b=to)
            tim._check(engine, f"{tag} neg", [pow(c, -1, n2) for c in cs], lambda o: engine.modinv(ap.mod_n2, tc, out=o), count, 2 * nw, a=tc)
            assert engine.download(ap.add_batch(tc, to)) == [a * b % n2 for a, b in zip(cs, others)]
            assert engine.download(ap.neg_batch(tc)) == [pow(c, -1, n2) for c in cs]
            ks = ([0, 1, (1 << 96) - 1][ci:] + [rng.getrandbits(96) for _ in range(count)])[:count]
            tk = up(ks, 3)
            clone = tc.clone()
            assert engine.download(ap.scalar_mul_batch(tc, tk)) == [pow(c, e, n2) for c, e in zip(cs, ks)], (tag, "scalar_mul")
            assert torch.equal(tc, clone)


def test_the_1025_bit_key_runs_where_the_padding_puts_it(engine):
    """Observed, not derived: N^2 (2049 bits in 66 words) on (4,27), not on the (4,18) its length alone would take; N's pair calls on the
    (4,14) NEG1 twin; both CRT halves on ONE pair instance, k_pvm<2,18>, and one single-modulus instance each for the primes ((2,18):
    the shorter prime padded to 17 words left (1,18)) and their squares ((2,27)) -- the padding joins what the lengths would part."""
    key = KEYS[1025]
    sk, ap, bp = _schemes(engine, 1025)
    rho = engine.upload([3, key.n - 1, 5], key.nw)
    with _PoliciesOff(engine):
        before = engine.launch_counts()
        ap.randomizer_batch(rho)
        pub = _interpreter_launches(engine, before)
        before = engine.launch_counts()
        c = bp.randomizer_batch(rho)
        crt = _interpreter_launches(engine, before)
        before = engine.launch_counts()
        bp.decrypt_raw_batch(c)
        dec = _interpreter_launches(engine, before)
    vm = lambda g, l: ("vm", g, l, 29, False, False, False)  # noqa: E731
    assert pub == {("pvm", 4, 14, 29, True, False, False), vm(4, 27)}
    half = ("pvm", 2, 18, 29, False, False, False)
    assert crt == {half, vm(2, 18), vm(2, 27), vm(4, 27)}
    assert dec == {half, vm(2, 18), vm(2, 27)}
    assert vm(4, 18) not in pub | crt | dec and vm(1, 18) not in crt | dec


# ---- step-level families -----------------------------------------------------------------------------------------------------------------
def _count(key):
    return K.batch_sizes(key)[1]


@pytest.mark.parametrize("bits", SIZES)
def test_multiplication_steps(engine, bits):
    """Four columns at unaligned offsets whose last field ends at nbits - 2 (and a single column on the smallest key, where two fields
    of at most 255 bits reach the end)."""
    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    for cols in ((1, 4) if bits == SIZES[0] else (4,)):
        mw = K.mul_widths(key, cols)
        count = _count(key)
        tmul._steps(engine, sk, ap, bp, mw["kappa"], mw["wx"], mw["wy"], True, bits + cols, bits, count, rows=list(range(count)))


def test_multiplication_one_bit_past_the_fit_limit_is_refused_with_nothing_launched(engine):
    from protocols.secure_comparison_amd import secure_multiply_batch

    for bits in SIZES:
        key = KEYS[bits]
        sk, ap, bp = _schemes(engine, bits)
        kappa, wx, wy = K.mul_widths(key)["refused"]
        x_t = engine.upload([sk.enc_raw(1)] * 2, 2 * key.nw)
        y_t = torch.stack([x_t] * len(wy)).contiguous()
        before = engine.launch_counts()
        with pytest.raises(ValueError, match=f"column {len(wy) - 1}"):
            secure_multiply_batch(x_t, y_t, wx, wy, ap, bp, signed=True, kappa=kappa)
        with pytest.raises(ValueError, match=f"column {len(wy) - 1}"):           # the library's own copy of the rule
            engine.keyholder_mul(bp.key, kappa, wx, list(wy), x_t, torch.zeros((len(wy), 2, key.nw), dtype=torch.int32, device=engine.device))
        assert engine.launch_counts() == before


@pytest.mark.parametrize("mode", ["one message", "two messages", "square"])
@pytest.mark.parametrize("bits", SIZES)
def test_inner_product_steps(engine, bits, mode):
    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    square = mode == "square"
    dw = K.dot_widths(key, square)
    k = dw["g"] if mode == "one message" else dw["g"] + 1
    count = _count(key)
    lay = tdot._steps(engine, sk, ap, bp, dw["kappa"], dw["wx"], dw["wy"], True, square, k, bits + k, bits, count, rows=list(range(count)))
    assert (lay.g, lay.M) == (dw["g"], 1 if mode == "one message" else 2)


@pytest.mark.parametrize("bits", SIZES)
def test_one_hot_steps_with_a_partial_last_message(engine, bits):
    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    ow = K.onehot_widths(key)
    count = _count(key)
    lay = tlook._steps(engine, sk, ap, bp, ow["kappa"], ow["index_bits"], ow["k"], ow["m"], bits, bits, count, rows=list(range(count)))
    assert (lay.g, lay.M, lay.m % lay.g) == (ow["g"], 2, 1)


def _select_steps(engine, key, sk, ap, bp, nf, count, seed):
    """select_pack -> select_mult -> select_finish and cx_finish against tests/_select_model.py on every row: sigma, d_j = a_j - b_j +
    2^w_j and b_j as randomized ciphertexts, widths whose last field ends at nbits - 2, draws at both ends of their ranges first."""
    from protocols.secure_comparison_amd.selection import SelectDraws, select_finish, select_mult, select_pack
    from protocols.secure_comparison_amd.sorting import cx_finish

    sw = K.select_widths(key, nf)
    lay, kappa, widths = sw["layout"], sw["kappa"], sw["widths"]
    n, n2, nw = key.n, key.n2, key.nw
    rng = random.Random(seed)
    sig = [i % 2 for i in range(count)]
    a = [[[0, (1 << w) - 1][(i + j) % 2] if i < 4 else rng.getrandbits(w) for i in range(count)] for j, w in enumerate(widths)]
    b = [[[(1 << w) - 1, 0][(i // 2 + j) % 2] if i < 4 else rng.getrandbits(w) for i in range(count)] for j, w in enumerate(widths)]
    draws = []
    for i in range(count):
        d = smodel.draw(rng, kappa, widths, n)
        if i < 2:       # all masks 0, all masks at their maximum
            d = (i * ((1 << kappa) - 1), [i * ((1 << (w + 1 + kappa)) - 1) for w in widths], d[2], d[3])
        draws.append(d)
    enc = lambda v: smodel.enc(sk, v, rng.randrange(1, n))  # noqa: E731
    sig_c = [enc(s) for s in sig]
    d_c = [[enc(a[j][i] - b[j][i] + (1 << widths[j])) for i in range(count)] for j in range(nf)]
    a_c = [[enc(a[j][i]) for i in range(count)] for j in range(nf)]
    b_c = [[enc(b[j][i]) for i in range(count)] for j in range(nf)]
    bw = (max(lay.fbits) + 31) // 32
    planes = lambda f, w: torch.stack([engine.upload([f(d, j) for d in draws], w) for j in range(nf)]).contiguous()  # noqa: E731
    sd = SelectDraws(r_a=engine.upload([d[0] for d in draws], 2), r_b=planes(lambda d, j: d[1][j], bw),
                     rho_p=engine.upload([d[2] for d in draws], nw), rho_products=planes(lambda d, j: d[3][j], nw))
    s_t = engine.upload(sig_c, 2 * nw)
    stack = lambda cols: torch.stack([engine.upload(r, 2 * nw) for r in cols]).contiguous()  # noqa: E731
    d_t, a_t, b_t = stack(d_c), stack(a_c), stack(b_c)
    clones = [t.clone() for t in (s_t, d_t, a_t, b_t)]
    col = lambda cs, i: [cs[j][i] for j in range(nf)]  # noqa: E731
    rows = lambda t: engine.download(t.reshape(-1, t.shape[-1]).contiguous())  # noqa: E731

    P, plain = select_pack(lay, s_t, d_t, sd, ap)
    want_P = [smodel.pack(sk, kappa, widths, sig_c[i], col(d_c, i), draws[i][0], draws[i][1], draws[i][2]) for i in range(count)]
    assert engine.download(P) == want_P, (key.bits, nf, "pack")
    prods = select_mult(lay, P, bp, sd.rho_products)
    want = [smodel.mult(sk, kappa, widths, want_P[i], draws[i][3]) for i in range(count)]
    assert not any(w[2] for w in want)
    pc = rows(prods)
    assert pc == [want[i][0][j] for j in range(nf) for i in range(count)], (key.bits, nf, "mult")
    out = select_finish(lay, s_t, d_t, b_t, prods, plain, sd, ap)
    want_out = [smodel.finish(sk, kappa, widths, sig_c[i], col(d_c, i), col(b_c, i), want[i][0], draws[i][0], draws[i][1]) for i in range(count)]
    got = rows(out)
    assert got == [want_out[i][j] for j in range(nf) for i in range(count)], (key.bits, nf, "finish")
    assert engine.download(bp.decrypt_raw_batch(out.reshape(nf * count, -1).contiguous())) == \
        [a[j][i] if sig[i] else b[j][i] for j in range(nf) for i in range(count)]
    # the compare-exchange: hi = F ab T^-1 (the finish with base F = a), lo = G T ab^-1 with G = b
    both = cx_finish(lay, s_t, d_t, a_t, b_t, prods, plain, sd, ap)
    hi = [smodel.finish(sk, kappa, widths, sig_c[i], col(d_c, i), col(a_c, i), want[i][0], draws[i][0], draws[i][1]) for i in range(count)]
    t_inv = [smodel.finish(sk, kappa, widths, sig_c[i], col(d_c, i), [1] * nf, [1] * nf, draws[i][0], draws[i][1]) for i in range(count)]
    lo = [[b_c[j][i] * pow(t_inv[i][j], -1, n2) % n2 * pow(want[i][0][j], -1, n2) % n2 for j in range(nf)] for i in range(count)]
    assert rows(both[0]) == [lo[i][j] for j in range(nf) for i in range(count)], (key.bits, nf, "cx lo")
    assert rows(both[1]) == [hi[i][j] for j in range(nf) for i in range(count)], (key.bits, nf, "cx hi")
    assert all(torch.equal(t, c) for t, c in zip((s_t, d_t, a_t, b_t), clones))


@pytest.mark.parametrize("nf", [1, 2, 3, 4])
@pytest.mark.parametrize("bits", SIZES)
def test_selection_and_compare_exchange_steps(engine, bits, nf):
    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    _select_steps(engine, key, sk, ap, bp, nf, _count(key), 10 * bits + nf)


# ---- comparison-based families -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", COMPARED)
def test_minimum_maximum_argmin(engine, keys, bits):
    from protocols.secure_comparison_amd.selection import secure_argmax_batch, secure_argmin_batch, secure_maximum_batch, secure_minimum_batch

    sk, ap, ad, bp, bd = tsel._players(engine, _with_odd(keys, bits), bits, "dgk_1024_l16")
    rng = random.Random(bits)
    top = (1 << L) - 1
    xs = [0, 0, top, top, 1, top - 1, 5] + [rng.getrandbits(L) for _ in range(17)]
    ys = [0, top, 0, top, 1, top, 5] + [rng.getrandbits(L) for _ in range(17)]
    nw2 = ap.mod_n2.nwords
    enc = lambda vs: engine.upload([smodel.enc(sk, v, rng.randrange(1, sk.n)) for v in vs], nw2)  # noqa: E731
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, nw2).contiguous()))  # noqa: E731
    x_t, y_t = enc(xs), enc(ys)
    mn, d1 = secure_minimum_batch(x_t, y_t, L, ap, ad, bp, bd)
    mx, d2 = secure_maximum_batch(x_t, y_t, L, ap, ad, bp, bd)
    assert dec(mn) == [min(x, y) for x, y in zip(xs, ys)] and dec(mx) == [max(x, y) for x, y in zip(xs, ys)]
    assert dec(d1) == dec(d2) == [int(x <= y) for x, y in zip(xs, ys)]
    k, B = 5, 12
    rows = [[rng.choice([0, 1, top, rng.getrandbits(L)]) for _ in range(k)] for _ in range(B)]                  # many ties
    v = torch.stack([enc(r) for r in rows]).contiguous()
    mv, mi = secure_argmin_batch(v, L, ap, ad, bp, bd)
    xv, xi = secure_argmax_batch(v, L, ap, ad, bp, bd)
    assert dec(mv) == [min(r) for r in rows] and dec(mi) == [r.index(min(r)) for r in rows]
    assert dec(xv) == [max(r) for r in rows] and dec(xi) == [r.index(max(r)) for r in rows]
    model_rng = random.Random(1)
    for r in rows[:3]:                                     # the tournament's own order, through the model
        assert smodel.argext(sk, r, L, model_rng) == (min(r), r.index(min(r)))


@pytest.mark.parametrize("k,m", [(5, 2), (8, 8)], ids=["top-2 of 5", "sort of 8"])
@pytest.mark.parametrize("bits", COMPARED)
def test_sort_and_top_m_follow_the_network(engine, keys, bits, k, m):
    """Values, two payload columns and indices of every row (tied rows included) against tests/_topk_model.py over topk_network:
    m = k is the sort."""
    ttopk._check_topk(engine, _with_odd(keys, bits), k, m, L, bits, "dgk_1024_l16")


# ---- axis families -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", SIZES)
def test_axis_sum_running_sum_and_linear_map(engine, bits):
    from protocols.secure_comparison_amd.aggregate import cumsum_planes_batch, sum_planes_batch
    from protocols.secure_comparison_amd.linear import linear_planes_batch

    key = KEYS[bits]
    sk, ap, bp = _schemes(engine, bits)
    n, n2, nw = key.n, key.n2, key.nw
    assert K.has_axis_instance(key)                        # (a key without one would have to be refused: tests/test_odd_keys_cpu.py lists none)
    g, l = K.configs(key)["n2"]
    rng = random.Random(bits)
    Kp, B = 3, _count(key)
    W = [[3, -5, (1 << 64) - 1], [0, 0, 0], [-1, 1, 1]]
    bias = [7, -(n // 3), 0]
    xb = K.linear_x_bits(key, W)
    half = 1 << (xb - 1)
    vals = [[[-half, half - 1, 0, -1][(kk + b) % 4] if b < 4 else rng.randrange(-half, half) for b in range(B)] for kk in range(Kp)]
    cs = [smodel.enc(sk, v, rng.randrange(1, n)) for pl in vals for v in pl]
    cs[0], cs[1] = n2 - 1, 1 + (n - 1) * n                 # a ciphertext with every word of N^2's own length set; the largest bare one
    vals[0][0], vals[0][1] = sk.dec_raw(n2 - 1), -1
    x = engine.upload(cs, 2 * nw).reshape(Kp, B, 2 * nw).contiguous()
    clone = x.clone()
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, 2 * nw).contiguous()))  # noqa: E731
    rows = lambda t: engine.download(t.reshape(-1, 2 * nw).contiguous())  # noqa: E731
    grew = lambda before: {k[0] for k in tim._grew(engine, before) if k[1:3] == (g, l)}  # noqa: E731

    before = engine.launch_counts()
    total = sum_planes_batch(x, ap)
    assert "reduce" in grew(before)
    assert rows(total) == R.prod_axis(n2, cs, 1, Kp, B)
    assert dec(total) == [sum(vals[kk][b] for kk in range(Kp)) % n for b in range(B)]
    before = engine.launch_counts()
    run = cumsum_planes_batch(x, ap)
    assert "scan" in grew(before)
    assert rows(run) == S.scan_axis(n2, cs, 1, Kp, B)
    assert dec(run) == [sum(vals[j][b] for j in range(kk + 1)) % n for kk in range(Kp) for b in range(B)]
    before = engine.launch_counts()
    lin = linear_planes_batch(x, W, ap, bias=bias, x_bits=xb)
    assert {"lin", "lift"} <= grew(before)
    want = LM.signed_map(W, bias, vals)
    assert dec(lin) == [v % n for row in want for v in row]
    assert rows(lin[1]) == [sk.enc_raw(bias[1])] * B        # the zero weight row: the bare [[bias]]
    before = engine.launch_counts()
    with pytest.raises(ValueError, match="row 0"):
        linear_planes_batch(x, W, ap, bias=bias, x_bits=xb + 1)
    assert engine.launch_counts() == before
    assert torch.equal(x, clone)


# ---- two players ---------------------------------------------------------------------------------------------------------------------------
def test_players_multiply_and_top_m_on_the_1025_bit_key(engine, keys):
    """Initiator and KeyHolder over the in-process communicator: the key holder's header checks accept widths taken from this key (a
    multiplication whose last field ends at nbits - 2), and a top-2 of 5 with payload and indices follows the network."""
    from protocols.secure_comparison_amd import InMemoryCommunicator, Initiator, KeyHolder
    from protocols.secure_comparison_amd.sorting import topk_network

    bits = 1025
    key = KEYS[bits]
    sk, ap, ad, bp, bd = tsel._players(engine, _with_odd(keys, bits), bits, "dgk_1024_l16")
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=600.0)
    alice = Initiator(L, communicator=comm, other_party="keyholder")
    bob = KeyHolder(L, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    mw = K.mul_widths(key)
    rng = random.Random(bits)
    B = _count(key)
    xs, ys, _ = tmul._case(rng, sk, mw["kappa"], mw["wx"], mw["wy"], True, B)
    _, _, x_t, y_t = tmul._encrypt(engine, sk, ap, rng, xs, ys)
    k, m = 5, 2
    trows, v, p, tuples = ttopk._case(engine, sk, ap, rng, 6, k, L)

    async def run():
        prod, _ = await asyncio.gather(
            alice.perform_secure_multiply_batch(x_t, y_t, mw["wx"], tuple(mw["wy"]), signed=True, kappa=mw["kappa"], engine=engine),
            bob.perform_secure_multiply_batch(mw["wx"], tuple(mw["wy"]), signed=True, kappa=mw["kappa"]))
        top, _ = await asyncio.gather(
            alice.perform_secure_topk_batch(v, m, payload=p, payload_bits=ttopk.WP, return_indices=True, engine=engine),
            bob.perform_secure_topk_batch(k, m, payload_bits=ttopk.WP, return_indices=True))
        return prod, top

    prod, (out, pay, idx) = asyncio.run(run())
    dec = lambda t: engine.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    assert dec(prod) == [x * y % sk.n for col in ys for x, y in zip(xs, col)]
    want = ttopk.model.apply(topk_network(k, m), tuples, False)
    assert ttopk._got(engine, bp, out, pay, idx, 6, m) == [[tuple(t) for t in r[:m]] for r in want]


# ---- majority, quantile and one chain ---------------------------------------------------------------------------------------------------------
def _world(engine, keys, bits):
    """(engine, sk, ap, ad, bp, bd): the tuple the aggregate, scan and pipeline modules call `world`, on an odd key."""
    sk, ap, ad, bp, bd = tsel._players(engine, _with_odd(keys, bits), bits, "dgk_1024_l16")
    return engine, sk, ap, ad, bp, bd


@pytest.mark.parametrize("k,m", [(3, 4), (5, 3)])
@pytest.mark.parametrize("bits", COMPARED)
def test_majority_with_planted_ties(engine, keys, bits, k, m):
    """Rows 0 .. 2 are ties (every label evenly, unanimous, the two highest labels): the lowest label wins, as the argmax's network does."""
    from protocols.secure_comparison_amd import secure_majority_batch

    w = _world(engine, keys, bits)
    _, sk, ap, ad, bp, bd = w
    rng = random.Random(f"odd-vote:{bits}:{k}:{m}")
    count = 24
    labels = [[rng.randrange(k) for _ in range(count)] for _ in range(m)]
    for q in range(m):
        labels[q][0], labels[q][1], labels[q][2] = (k - 1 - q) % k, k - 1, (k - 1) if q % 2 else (k - 2)
    enc = tagg._enc(w, rng, [v for row in labels for v in row]).reshape(m, count, -1).contiguous()
    clone = enc.clone()
    label, top = secure_majority_batch(enc, k, ap, ad, bp, bd)
    hist = tagg._hist(labels, k)
    cols = [[hist[t][b] for t in range(k)] for b in range(count)]
    assert tagg._dec(w, top) == [max(c) for c in cols]
    assert tagg._dec(w, label) == [c.index(max(c)) for c in cols]
    model_rng = random.Random(2)
    for c in cols[:3]:                                     # the tied rows through the tournament's own model
        assert smodel.argext(sk, c, 16, model_rng, want_max=True) == (max(c), c.index(max(c)))
    assert torch.equal(enc, clone)


@pytest.mark.parametrize("bits", COMPARED)
def test_quantile_of_every_rank(engine, keys, bits):
    """k = 3 bins, m = 5 indices per row with the planted rows of tests/test_gpu_scan.py (one bin, the end bins, an index at or above
    k): the bin of every public rank, of encrypted per-row ranks, and the median, decrypted on every row."""
    from protocols.secure_comparison_amd import secure_histogram_median_batch, secure_quantile_batch
    from protocols.secure_comparison_amd.lookup import default_index_bits

    w = _world(engine, keys, bits)
    _, sk, ap, ad, bp, bd = w
    k, m, count = 3, 5, 24
    rng = random.Random(f"odd-quantile:{bits}")
    ib = default_index_bits(k) + 1
    idx = tscan._planted(rng, k, m, ib, count)
    enc = tagg._enc(w, rng, [v for row in idx for v in row]).reshape(m, count, -1).contiguous()
    clone = enc.clone()
    for kth in range(m):
        got = secure_quantile_batch(enc, k, kth, ap, ad, bp, bd, index_bits=ib)
        assert tagg._dec(w, got) == [tscan._sorted_bins(idx, k, b)[kth] for b in range(count)], kth
    ranks = [b % m for b in range(count)]
    got = secure_quantile_batch(enc, k, tagg._enc(w, rng, ranks), ap, ad, bp, bd, index_bits=ib)
    assert tagg._dec(w, got) == [tscan._sorted_bins(idx, k, b)[ranks[b]] for b in range(count)]
    got = secure_histogram_median_batch(enc, k, ap, ad, bp, bd, index_bits=ib)
    assert tagg._dec(w, got) == [tscan._sorted_bins(idx, k, b)[(m - 1) // 2] for b in range(count)]
    assert torch.equal(enc, clone)


def test_knn_classify_chain_on_the_1025_bit_key(engine, keys):
    """Chain 1 of tests/test_gpu_pipelines.py through its own builder: squared distance -> top-m with labels -> votes -> majority, every
    intermediate decrypted on all rows against tests/_pipeline_model.py, outputs handed on as they are."""
    tpipe.test_knn_classify(_world(engine, keys, 1025), "handed-on")


# ---- the library's own draws ---------------------------------------------------------------------------------------------------------------
DRAW_KEY = bytes((13 * i + 5) & 0xFF for i in range(32))


@pytest.fixture()
def seeded(engine):
    try:
        yield engine
    finally:
        engine.rng_seed(None)


@pytest.mark.parametrize("bits", (521, 1025))
def test_own_draws_below_a_bound_with_a_partial_top_word(seeded, bits):
    """uniform_below(N) on the device generator: every draw below N (and nonzero when asked), and the words those of the generator
    restated by oracle/chacha_rng.py at the same call numbers.  At 1025 bits the top word of the bound is a single bit."""
    from protocols.secure_comparison_amd.randomness import uniform_below

    engine, n = seeded, KEYS[bits].n
    rp = dr.Replay(DRAW_KEY)
    engine.rng_seed(DRAW_KEY)
    for count, nonzero in ((1, True), (24, True), (70, True), (24, False)):
        got = engine.download(uniform_below(n, count, engine, nonzero=nonzero))
        assert all((1 if nonzero else 0) <= v < n for v in got), (count, nonzero)
        assert got == rp.below(n, count, nonzero, range(count)), (count, nonzero)
    assert len({v >> (bits - 1) for v in engine.download(uniform_below(n, 70, engine, nonzero=True))}) == 2, "both values of N's top bit occur"
    rp.below(n, 70, True, range(1))
    assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(DRAW_KEY, rp.call, 64, 4)


@pytest.mark.parametrize("bits", (521, 1025))
def test_own_draws_multiply(seeded, bits):
    """secure_multiply_batch with no draws argument: bit for bit the replay of tests/_draw_replay.py, and it decrypts to the products."""
    from protocols.secure_comparison_amd import secure_multiply_batch

    engine = seeded
    sk, ap, bp = _schemes(engine, bits)
    rng, B = random.Random(bits), 24
    wx, wy = 16, [16, 7]
    half = lambda w: 1 << (w - 1)  # noqa: E731
    xs = [-half(wx), half(wx) - 1, 0, -1] + [rng.randrange(-half(wx), half(wx)) for _ in range(B - 4)]
    ys = [[[half(w) - 1, -half(w), -1, 0][i] if i < 4 else rng.randrange(-half(w), half(w)) for i in range(B)] for w in wy]
    x_c = [smodel.enc(sk, v, rng.randrange(1, sk.n)) for v in xs]
    y_c = [[smodel.enc(sk, v, rng.randrange(1, sk.n)) for v in col] for col in ys]
    x_t = engine.upload(x_c, 2 * KEYS[bits].nw)
    y_t = torch.stack([engine.upload(col, 2 * KEYS[bits].nw) for col in y_c]).contiguous()
    d = dr.Driver(sk, None, L, 400, DRAW_KEY)
    engine.rng_seed(DRAW_KEY)
    out = secure_multiply_batch(x_t, y_t, wx, tuple(wy), ap, bp, signed=True)
    want = d.multiply(x_c, y_c, range(B), B, wx, wy, True)
    assert [engine.download(out[j]) for j in range(len(wy))] == want
    assert engine.download(bp.decrypt_raw_batch(out.reshape(len(wy) * B, -1).contiguous())) == [x * y % sk.n for col in ys for x, y in zip(xs, col)]
    assert d.calls[0] == 3 + len(wy)
    assert engine.download(engine.rng_bits(64, 4)) == cr.rng_bits(DRAW_KEY, d.calls[0], 64, 4)

"""The scheme-level selection / compare-exchange entries of include/sc_amd.h on the GPU, driven the way a C host drives them: ctypes,
sc_malloc / sc_memcpy_*, none of this package's scheme classes, Engine or selection.py on the path under test (DESIGN.md §8b, §8c;
INTEGRATION.md "Selection and sort from C").  Every message and result is compared bit for bit with the pure-Python models
(tests/_select_model.py, tests/_sort_model.py) on the rows Host.model_rows picks -- the six edge rows at the head, the last row and
random rows from the middle and the tail, seeded by the case: a full-size Python pow takes 16 / 120 / 380 ms at 1024 / 2048 / 3072
bits -- and every row of every result is decrypted (sc_paillier_decrypt) and
compared with Python's min / max; the Python path (selection.py / sorting.py) must give the very same words on all rows."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

from conftest import GOLDEN, oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _select_model as sm  # noqa: E402
import _sort_model as sortm  # noqa: E402

pytestmark = pytest.mark.gpu

RBITS, KAPPA = 400, 40
MODEL_ROWS = {1024: 16, 2048: 10, 3072: 9}       # rows per batch that go through the Python model, by key size
SC_ERR_ARG, SC_ERR_UNSUPPORTED, SC_ERR_LAYOUT = -1, -4, -5


def _dgk(keys, name, wide):
    if not wide:
        return oracle_dgk(keys, name)
    from oracle import sc_oracle as o

    k = json.load(open(os.path.join(GOLDEN, "keys_wide.json")))[name]
    p, q = int(k["p"], 16), int(k["q"], 16)
    return o.DGKKey(p * q, int(k["g"], 16), int(k["h"], 16), int(k["u"], 16), k["t"], p, q, int(k["v_p"], 16), int(k["v_q"], 16))


class Host:
    """A C host's view of the library: one context, device buffers through sc_malloc / sc_memcpy_*, keys through the key objects."""

    def __init__(self, sk, dgk):
        from protocols.secure_comparison_amd import _lib
        from protocols.secure_comparison_amd.limbs import ints_to_words, words_to_ints

        self.lib, self.to_words, self.to_ints = _lib.load(), ints_to_words, words_to_ints
        self.ctx = C.c_void_p()
        assert self.lib.sc_ctx_create(0, C.byref(self.ctx)) == 0
        self.live = []
        self.sk, self.dgk = sk, dgk
        self.nw = (sk.n.bit_length() + 31) // 32
        hw = (max(sk.p.bit_length(), sk.q.bit_length()) + 31) // 32
        w = lambda v, words: ints_to_words([v], words)  # noqa: E731
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        kn, kp, kq = w(sk.n, self.nw), w(sk.p, hw), w(sk.q, hw)
        self.a_key, self.b_key = C.c_int(), C.c_int()
        assert self.lib.sc_paillier_key_create(self.ctx, p(kn), self.nw, None, None, 0, 0, C.byref(self.a_key)) == 0, self.err()
        assert self.lib.sc_paillier_key_create(self.ctx, p(kn), self.nw, p(kp), p(kq), hw, 0, C.byref(self.b_key)) == 0, self.err()
        if dgk is None:
            return
        self.nd, self.ew, self.er = (dgk.n.bit_length() + 31) // 32, (dgk.u.bit_length() + 31) // 32, (RBITS + 31) // 32
        pw, vw = (max(dgk.p.bit_length(), dgk.q.bit_length()) + 31) // 32, (max(dgk.v_p.bit_length(), dgk.v_q.bit_length()) + 31) // 32
        dk = [w(dgk.n, self.nd), w(dgk.g, self.nd), w(dgk.h, self.nd), w(dgk.u, self.ew), w(dgk.p, pw), w(dgk.q, pw), w(dgk.v_p, vw), w(dgk.v_q, vw)]
        self.a_dgk, self.b_dgk = C.c_int(), C.c_int()
        assert self.lib.sc_dgk_key_create(self.ctx, p(dk[0]), p(dk[1]), p(dk[2]), self.nd, p(dk[3]), self.ew, dgk.t, None, None, 0, None, None, 0,
                                          RBITS, 8, 0, None, -1, C.byref(self.a_dgk)) == 0, self.err()
        assert self.lib.sc_dgk_key_create(self.ctx, p(dk[0]), p(dk[1]), p(dk[2]), self.nd, p(dk[3]), self.ew, dgk.t, p(dk[4]), p(dk[5]), pw, p(dk[6]),
                                          p(dk[7]), vw, RBITS, 8, 0, None, -1, C.byref(self.b_dgk)) == 0, self.err()

    def err(self):
        return self.lib.sc_last_error(self.ctx).decode()

    def dev(self, host):
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        assert self.lib.sc_malloc(self.ctx, max(host.nbytes, 4), C.byref(p)) == 0
        assert self.lib.sc_memcpy_h2d(self.ctx, p, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0
        self.live.append(p)
        return p

    def up(self, ints, words):
        return self.dev(self.to_words(list(ints), words))

    def empty(self, *shape, dtype=np.uint32):
        return self.dev(np.zeros(shape, dtype=dtype))

    def back(self, p, *shape, dtype=np.uint32):
        out = np.zeros(shape, dtype=dtype)
        assert self.lib.sc_memcpy_d2h(self.ctx, out.ctypes.data_as(C.c_void_p), p, out.nbytes) == 0
        return out

    def ints(self, p, rows, words):
        return self.to_ints(self.back(p, rows, words))

    def encrypt(self, values, rng):
        """Randomized encryptions of `values` made by the library itself: (device array, the ciphertexts as ints)."""
        count = len(values)
        d_m, d_rho = self.up(values, self.nw), self.up([rng.randrange(1, self.sk.n) for _ in values], self.nw)
        d_c = self.empty(count, 2 * self.nw)
        assert self.lib.sc_paillier_encrypt(self.ctx, self.a_key, d_m, self.nw, 0, d_c, count) == 0, self.err()
        assert self.lib.sc_paillier_randomize(self.ctx, self.a_key, d_c, d_rho, d_c, count) == 0, self.err()
        return d_c, self.ints(d_c, count, 2 * self.nw)

    def decrypt(self, p, count):
        d_m = self.empty(count, self.nw)
        assert self.lib.sc_paillier_decrypt(self.ctx, self.b_key, p, d_m, count) == 0, self.err()
        return self.ints(d_m, count, self.nw)

    def model_rows(self, B, rng):
        """The rows that go through the Python model: the six edge rows of _values, the last row, and random rows in between."""
        m = min(B, MODEL_ROWS.get(32 * ((self.sk.n.bit_length() + 31) // 32), 16))
        return sorted(set(range(6)) | {B - 1} | set(rng.sample(range(6, B - 1), max(0, m - 7))))

    def at(self, p, word_offset):
        return C.c_void_p(p.value + 4 * word_offset)

    def close(self):
        for p in self.live:
            self.lib.sc_free(self.ctx, p)
        self.lib.sc_ctx_destroy(self.ctx)


@pytest.fixture()
def host_factory():
    made = []

    def make(sk, dgk):
        made.append(Host(sk, dgk))
        return made[-1]

    yield make
    for h in made:
        h.close()


def _compare(h, l, d_x, d_y, xs, ys, drs, randomize_z=True):
    """The five comparison calls on device arrays; returns what a selection needs: [[delta]], step 1's [[z]] and r, and [[delta]] as
    ints.  Every [[delta]] is decrypted and compared with x <= y (the ciphertexts themselves are pinned by the comparison's tests)."""
    lib, ctx, B, nw, nd, lw = h.lib, h.ctx, len(xs), h.nw, h.nd, (l + 63) // 64
    planes = lambda rows, w: np.stack([h.to_words([rows[b][i] for b in range(B)], w) for i in range(l + 1)])  # noqa: E731
    u64 = lambda *s: h.empty(*s, dtype=np.uint64)  # noqa: E731
    d_r = h.up([d.r for d in drs], nw)
    d_rho_z = h.up([d.rho_z for d in drs], nw) if randomize_z else None
    d_z, d_alpha, d_alpha_t, d_rsmall, d_rshift = h.empty(B, 2 * nw), u64(B, lw), u64(B, lw), u64(B), h.empty(B, nw)
    assert lib.sc_initiator_step1(ctx, h.a_key, l, d_x, d_y, d_r, d_rho_z, 0, d_z, d_alpha, d_alpha_t, d_rsmall, d_rshift, B) == 0, h.err()
    d_rb = h.dev(planes([[d.r_d] + d.r_beta for d in drs], h.er))
    d_zp, d_beta, d_dbit, d_z1, d_z2, d_db = h.empty(B, nw), u64(B, lw), u64(B), h.empty(B, nw), h.empty(B, nw), h.empty(l + 1, B, nd)
    assert lib.sc_keyholder_step2_4b(ctx, h.b_key, h.b_dgk, l, d_z, d_rb, h.er, 0, d_zp, d_beta, d_dbit, d_z1, d_z2, d_db, B) == 0, h.err()
    shuffled = drs[0].perm is not None
    rc_pre = [list(d.r_c) for d in drs]
    if shuffled:                               # the oracle randomizes output k = c_{perm[k]} after the shuffle
        for b, d in enumerate(drs):
            for k, src in enumerate(d.perm):
                rc_pre[b][src] = d.r_c[k]
    d_rhos, d_ra = h.dev(planes([d.rhos for d in drs], h.ew)), h.dev(planes(rc_pre, h.er))
    d_perm = h.dev(np.array([d.perm for d in drs], dtype=np.int64)) if shuffled else None
    d_da = h.dev(np.array([d.delta_a for d in drs], dtype=np.uint64))
    d_c = h.empty(l + 1, B, nd)
    assert lib.sc_initiator_step4(ctx, h.a_dgk, l, d_db, h.at(d_db, B * nd), d_alpha, d_alpha_t, d_rsmall, d_da, d_rhos, h.ew, d_perm, d_ra, h.er, 0,
                                  None, d_c, B) == 0, h.err()
    d_rho3 = h.dev(np.concatenate([h.to_words([getattr(d, f) for d in drs], nw) for f in ("rho_zeta1", "rho_zeta2", "rho_delta_b")]))
    d_delta_b, d_out3 = u64(B), h.empty(3, B, 2 * nw)
    assert lib.sc_keyholder_step4j_5(ctx, h.b_key, h.b_dgk, l, d_c, d_z1, d_z2, d_rho3, 0, d_delta_b, d_out3, B) == 0, h.err()
    d_delta = h.empty(B, 2 * nw)
    assert lib.sc_initiator_step67(ctx, h.a_key, d_da, h.at(d_out3, 2 * B * 2 * nw), d_out3, h.at(d_out3, B * 2 * nw), d_rsmall, d_rshift, 0,
                                   d_delta, B) == 0, h.err()
    assert h.decrypt(d_delta, B) == [int(x <= y) for x, y in zip(xs, ys)]
    return d_delta, d_z, d_r, h.ints(d_delta, B, 2 * nw)


def _widths(widths):
    return (C.c_int * len(widths))(*widths)


def _select_draws(h, rng, widths, B):
    """Injected selection draws: the host lists and their device arrays (r_a [B][2], r_b [nf][B][bw], rho_p [B][nw], rho_products)."""
    draws = [sm.draw(rng, KAPPA, widths, h.sk.n) for _ in range(B)]
    nf = len(widths)
    bw = (max(w + KAPPA + 2 for w in widths) + 31) // 32
    dev = dict(r_a=h.up([d[0] for d in draws], 2), r_b=h.dev(np.stack([h.to_words([d[1][j] for d in draws], bw) for j in range(nf)])),
               rho_p=h.up([d[2] for d in draws], h.nw), rho_q=h.dev(np.stack([h.to_words([d[3][j] for d in draws], h.nw) for j in range(nf)])))
    return draws, dev, bw, bw                    # ew = bw: both hold max_j (w_j + kappa + 2) bits


def _exchange(h, widths, d_sigma, d_d, sigma, d_cols, draws, dev, bw, ew, B, rows):
    """select_pack | keyholder_select_mult, P and the products checked against the model on `rows`; returns (products, e, rab, the
    device's products as ints [nf][B])."""
    lib, ctx, nw, nf = h.lib, h.ctx, h.nw, len(widths)
    wp = _widths(widths)
    d_P, d_e, d_rab = h.empty(B, 2 * nw), h.empty(nf, B, ew), h.empty(nf, B, nw)
    assert lib.sc_initiator_select_pack(ctx, h.a_key, KAPPA, nf, wp, d_sigma, d_d, dev["r_a"], 2, dev["r_b"], bw, dev["rho_p"], ew, d_P, d_e,
                                        d_rab, B) == 0, h.err()
    got_P = h.ints(d_P, B, 2 * nw)
    want_P = {i: sm.pack(h.sk, KAPPA, widths, sigma[i], [c[i] for c in d_cols], draws[i][0], draws[i][1], draws[i][2]) for i in rows}
    assert [got_P[i] for i in rows] == [want_P[i] for i in rows]
    d_prod = h.empty(nf, B, 2 * nw)
    assert lib.sc_keyholder_select_mult(ctx, h.b_key, KAPPA, nf, wp, d_P, dev["rho_q"], d_prod, B) == 0, h.err()
    flat = h.ints(d_prod, nf * B, 2 * nw)
    prods = [flat[j * B:(j + 1) * B] for j in range(nf)]
    for i in rows:
        want, _, bad = sm.mult(h.sk, KAPPA, widths, want_P[i], draws[i][3])
        assert not bad and [prods[j][i] for j in range(nf)] == want
    return d_prod, d_e, d_rab, prods


def _values(rng, l, B):
    """x, y with ties and the extremes 0 and 2^l - 1 (the first six rows)."""
    top = (1 << l) - 1
    xs = [rng.getrandbits(l) for _ in range(B)]
    ys = [xs[i] if i % 4 == 0 else rng.getrandbits(l) for i in range(B)]
    for i, (x, y) in enumerate([(0, 0), (top, top), (0, top), (top, 0), (top, top - 1 if top else 0), (0, min(1, top))]):
        xs[i], ys[i] = x, y
    return xs, ys


def _minmax(h, l, B, seed):
    from oracle import sc_oracle as o

    sk, nw, n, n2 = h.sk, h.nw, h.sk.n, h.sk.n2
    rng = random.Random(seed)
    rows = h.model_rows(B, rng)
    xs, ys = _values(rng, l, B)
    drs = [o.draw(rng, l, sk, h.dgk, RBITS) for _ in range(B)]
    (d_x, x_enc), (d_y, _) = h.encrypt(xs, rng), h.encrypt(ys, rng)
    d_delta, d_z, d_r, delta = _compare(h, l, d_x, d_y, xs, ys, drs)
    z = h.ints(d_z, B, 2 * nw)
    d_d = h.empty(1, B, 2 * nw)
    assert h.lib.sc_initiator_select_d(h.ctx, h.a_key, d_z, d_r, d_d, B) == 0, h.err()
    d_col = [zc * (1 - dr.r * n) % n2 for zc, dr in zip(z, drs)]
    assert h.ints(d_d, B, 2 * nw) == d_col
    assert h.decrypt(d_d, B) == [y - x + (1 << l) for x, y in zip(xs, ys)]
    for want_max in (False, True):
        if want_max:
            d_sigma, sigma = d_delta, delta
        else:
            d_sigma = h.empty(B, 2 * nw)
            assert h.lib.sc_paillier_one_minus(h.ctx, h.a_key, d_delta, d_sigma, B) == 0, h.err()
            sigma = h.ints(d_sigma, B, 2 * nw)
            assert sigma == [(n + 1) * pow(c, -1, n2) % n2 for c in delta]
        draws, dev, bw, ew = _select_draws(h, rng, [l], B)
        d_prod, d_e, d_rab, prods = _exchange(h, [l], d_sigma, d_d, sigma, [d_col], draws, dev, bw, ew, B, rows)
        d_out = h.empty(1, B, 2 * nw)
        assert h.lib.sc_initiator_select_finish(h.ctx, h.a_key, KAPPA, 1, _widths([l]), d_sigma, d_d, d_x, d_prod, dev["r_a"], 2, d_e, ew, d_rab,
                                                d_out, B) == 0, h.err()
        got = h.ints(d_out, B, 2 * nw)
        want = [sm.finish(sk, KAPPA, [l], sigma[i], [d_col[i]], [x_enc[i]], [prods[0][i]], draws[i][0], draws[i][1])[0] for i in rows]
        assert [got[i] for i in rows] == want
        assert h.decrypt(d_out, B) == [(max if want_max else min)(x, y) for x, y in zip(xs, ys)]


# key sizes 1024 / 2048 / 3072 = the three pair configurations with a per-row instance; l in {1, 32, 64, 255} at 1024 bits
@pytest.mark.parametrize("pbits,dname,l,wide", [(1024, "dgk_1024_l16", 1, False), (1024, "dgk_2048_l32", 32, False),
                                                (1024, "dgk_2048_l64", 64, False), (1024, "dgk_1024_l255", 255, True),
                                                (2048, "dgk_2048_l32", 32, False), (3072, "dgk_3072_l64", 64, False)])
def test_minimum_and_maximum_from_c(host_factory, keys, pbits, dname, l, wide):
    h = host_factory(oracle_paillier(keys, pbits), _dgk(keys, dname, wide))
    pair = C.c_int()
    assert h.lib.sc_paillier_key_mods(h.ctx, h.a_key, C.byref(pair), None) == 0
    assert h.lib.sc_mod_supports_sq(h.ctx, pair) == 1
    _minmax(h, l, 64, 1000 * pbits + l)


def _key_without_per_row_instance(h_factory, dgk):
    """A Paillier key whose modulus has no pair kernel with per-row exponents, found by asking the library: sc_mod_supports_sq, and
    -- for a modulus that has pair arithmetic but no per-row instance -- sc_modexp_var_sq's own SC_ERR_UNSUPPORTED on one row."""
    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd.keygen import rand_prime

    rng = random.Random(4242)
    for bits in (512, 768, 1280, 1536):
        p, q = rand_prime(bits // 2, rng.getrandbits), rand_prime(bits // 2, rng.getrandbits)
        if p == q:
            continue
        h = h_factory(o.PaillierKey(p * q, p, q), dgk)
        mod_n, mod_n2 = C.c_int(), C.c_int()
        assert h.lib.sc_paillier_key_mods(h.ctx, h.a_key, C.byref(mod_n), C.byref(mod_n2)) == 0
        if h.lib.sc_mod_supports_sq(h.ctx, mod_n) == 0:
            return h
        one = h.up([1], 2 * h.nw)
        if h.lib.sc_modexp_var_sq(h.ctx, mod_n, mod_n2, 1, one, 2 * h.nw, one, 1, 1, None, h.empty(1, 2 * h.nw), 1) == SC_ERR_UNSUPPORTED:
            return h
    pytest.fail("every candidate key has a per-row pair instance")


def test_minimum_and_maximum_without_a_per_row_pair_instance(host_factory, keys):
    """The entries fall back to exponentiations modulo N^2 themselves: the caller never sees SC_ERR_UNSUPPORTED."""
    h = _key_without_per_row_instance(host_factory, oracle_dgk(keys, "dgk_1024_l16"))
    _minmax(h, 16, 64, 99)


def test_one_argmin_round_from_c(host_factory, keys):
    """One tournament round over the pairs (L, R) with a value and an index column: the comparison, select_d, one_minus,
    cx_differences (the index column's [[R.i - L.i + 2^wi]]), the exchange and select_finish with base L: (min, its index), ties left."""
    from oracle import sc_oracle as o

    h = host_factory(oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16"))
    sk, nw, n, n2, l, wi, B = h.sk, h.nw, h.sk.n, h.sk.n2, 16, 3, 64
    widths = [l, wi]
    rng = random.Random(31)
    rows = h.model_rows(B, rng)
    lv, rv = _values(rng, l, B)
    li, ri = [rng.randrange(8) for _ in range(B)], [rng.randrange(8) for _ in range(B)]
    drs = [o.draw(rng, l, sk, h.dgk, RBITS) for _ in range(B)]
    d_f, f_c = h.encrypt(lv + li, rng)                       # F = [L.v, L.i], G = [R.v, R.i] as [2][B] arrays
    d_g, g_c = h.encrypt(rv + ri, rng)
    d_delta, d_z, d_r, delta = _compare(h, l, d_f, d_g, lv, rv, drs)
    d_dv = h.empty(B, 2 * nw)
    assert h.lib.sc_initiator_select_d(h.ctx, h.a_key, d_z, d_r, d_dv, B) == 0, h.err()
    d_sigma = h.empty(B, 2 * nw)
    assert h.lib.sc_paillier_one_minus(h.ctx, h.a_key, d_delta, d_sigma, B) == 0, h.err()
    sigma = h.ints(d_sigma, B, 2 * nw)
    assert sigma == [(n + 1) * pow(c, -1, n2) % n2 for c in delta]
    d_d = h.empty(2, B, 2 * nw)
    assert h.lib.sc_initiator_cx_differences(h.ctx, h.a_key, KAPPA, 2, _widths(widths), d_f, d_g, d_dv, d_d, B) == 0, h.err()
    dv = h.ints(d_dv, B, 2 * nw)
    di = [g * pow(f, -1, n2) % n2 * (1 + (1 << wi) * n) % n2 for f, g in zip(f_c[B:], g_c[B:])]
    assert h.ints(d_d, 2 * B, 2 * nw) == dv + di
    draws, dev, bw, ew = _select_draws(h, rng, widths, B)
    d_prod, d_e, d_rab, prods = _exchange(h, widths, d_sigma, d_d, sigma, [dv, di], draws, dev, bw, ew, B, rows)
    d_out = h.empty(2, B, 2 * nw)
    assert h.lib.sc_initiator_select_finish(h.ctx, h.a_key, KAPPA, 2, _widths(widths), d_sigma, d_d, d_f, d_prod, dev["r_a"], 2, d_e, ew, d_rab,
                                            d_out, B) == 0, h.err()
    got = h.ints(d_out, 2 * B, 2 * nw)
    for i in rows:
        want = sm.finish(sk, KAPPA, widths, sigma[i], [dv[i], di[i]], [f_c[i], f_c[B + i]], [prods[0][i], prods[1][i]], draws[i][0], draws[i][1])
        assert [got[i], got[B + i]] == want
    dec = h.decrypt(d_out, 2 * B)
    assert list(zip(dec[:B], dec[B:])) == [(a, ia) if a <= b else (b, ib) for a, ia, b, ib in zip(lv, li, rv, ri)]


# B = 37, four columns: a column boundary of cx_differences falls inside a wave, and both of its ratio operands are in use
@pytest.mark.parametrize("B,widths", [(64, [16, 8, 20]), (37, [16, 8, 20, 5])])
@pytest.mark.parametrize("indexed", [False, True])
def test_compare_exchange_with_payload_columns_from_c(host_factory, keys, indexed, B, widths):
    """Key and two or three payload columns against _sort_model.compare_exchange; with index rows, rows >= out_rows stay untouched."""
    from oracle import sc_oracle as o

    h = host_factory(oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16"))
    sk, nw, n, n2, l, nf = h.sk, h.nw, h.sk.n, h.sk.n2, widths[0], len(widths)
    rng = random.Random(57 + indexed + B)
    rows = h.model_rows(B, rng)
    fv, gv = _values(rng, l, B)
    f_plain = [fv] + [[rng.getrandbits(w) for _ in range(B)] for w in widths[1:]]
    g_plain = [gv] + [[rng.getrandbits(w) for _ in range(B)] for w in widths[1:]]
    d_f, f_flat = h.encrypt(sum(f_plain, []), rng)
    d_g, g_flat = h.encrypt(sum(g_plain, []), rng)
    f_c, g_c = [f_flat[j * B:(j + 1) * B] for j in range(nf)], [g_flat[j * B:(j + 1) * B] for j in range(nf)]
    drs = [o.draw(rng, l, sk, h.dgk, RBITS) for _ in range(B)]
    # [[z]] unrandomized: the key column's [[d]] = [[G]] [[F]]^-1 (1 + 2^l N) is then the model's own integer
    d_delta, d_z, d_r, delta = _compare(h, l, d_f, d_g, fv, gv, drs, randomize_z=False)
    d_dk = h.empty(B, 2 * nw)
    assert h.lib.sc_initiator_select_d(h.ctx, h.a_key, d_z, d_r, d_dk, B) == 0, h.err()
    d_d = h.empty(nf, B, 2 * nw)
    wp = _widths(widths)
    assert h.lib.sc_initiator_cx_differences(h.ctx, h.a_key, KAPPA, nf, wp, d_f, d_g, d_dk, d_d, B) == 0, h.err()
    d_cols = [[g * pow(f, -1, n2) % n2 * (1 + (1 << w) * n) % n2 for f, g in zip(fc, gc)] for fc, gc, w in zip(f_c, g_c, widths)]
    assert h.ints(d_d, nf * B, 2 * nw) == sum(d_cols, [])
    draws, dev, bw, ew = _select_draws(h, rng, widths, B)
    d_prod, d_e, d_rab, _ = _exchange(h, widths, d_delta, d_d, delta, d_cols, draws, dev, bw, ew, B, rows)
    want = {i: sortm.compare_exchange(sk, KAPPA, widths, delta[i], [c[i] for c in f_c], [c[i] for c in g_c], draws[i]) for i in rows}
    items = nf * B
    args = (h.ctx, h.a_key, KAPPA, nf, wp, d_delta, d_d, d_f, d_g, d_prod, dev["r_a"], 2, d_e, ew, d_rab)
    d_ref = h.empty(2, nf, B, 2 * nw)                                       # the contiguous form: (lo, hi)
    assert h.lib.sc_initiator_cx_finish(*args, None, None, d_ref, 2 * items, B) == 0, h.err()
    ref = h.ints(d_ref, 2 * items, 2 * nw)
    for i in rows:
        assert [ref[j * B + i] for j in range(nf)] == want[i][0] and [ref[items + j * B + i] for j in range(nf)] == want[i][1]
    dec = h.decrypt(d_ref, 2 * items)
    lo, hi = dec[:items], dec[items:]
    for i in range(B):
        keep = fv[i] <= gv[i]                                                # equal keys are not exchanged
        assert [lo[j * B + i] for j in range(nf)] == [(f_plain if keep else g_plain)[j][i] for j in range(nf)]
        assert [hi[j * B + i] for j in range(nf)] == [(g_plain if keep else f_plain)[j][i] for j in range(nf)]
    if not indexed:
        return
    rows_out = 2 * items - 9                                                 # the last destinations lie at or past out_rows: not written
    dest = rng.sample(range(2 * items + 5), 2 * items)
    pattern = np.full((2 * items + 5, 2 * nw), 0xA5A5A5A5, dtype=np.uint32)
    d_out = h.dev(pattern)
    lo_i, hi_i = h.dev(np.array(dest[:items], dtype=np.uint64)), h.dev(np.array(dest[items:], dtype=np.uint64))
    assert h.lib.sc_initiator_cx_finish(*args, lo_i, hi_i, d_out, rows_out, B) == 0, h.err()
    expect = pattern.copy()
    words = h.back(d_ref, 2 * items, 2 * nw)
    for k, r in enumerate(dest):
        if r < rows_out:
            expect[r] = words[k]
    assert sum(r >= rows_out for r in dest) > 0
    assert np.array_equal(h.back(d_out, 2 * items + 5, 2 * nw), expect)


def test_python_path_and_c_path_are_one(engine, host_factory, keys):
    """selection.secure_minimum_batch and sorting.secure_compare_exchange_batch under the same injected draws give the words the C
    calls give, on every row."""
    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.batch import BatchDraws
    from protocols.secure_comparison_amd.selection import SelectDraws, secure_minimum_batch
    from protocols.secure_comparison_amd.sorting import secure_compare_exchange_batch

    sk, dgk = oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_1024_l16")
    h = host_factory(sk, dgk)
    nw, l, B = h.nw, 16, 64
    rng = random.Random(808)
    xs, ys = _values(rng, l, B)
    drs = [o.draw(rng, l, sk, dgk, RBITS, shuffle=False) for _ in range(B)]
    (d_x, x_enc), (d_y, y_enc) = h.encrypt(xs, rng), h.encrypt(ys, rng)
    draws, dev, bw, ew = _select_draws(h, rng, [l], B)
    wp = _widths([l])
    # the C path: minimum, then the compare-exchange of the same comparison
    d_delta, d_z, d_r, _ = _compare(h, l, d_x, d_y, xs, ys, drs)
    d_d, d_sigma = h.empty(1, B, 2 * nw), h.empty(B, 2 * nw)
    assert h.lib.sc_initiator_select_d(h.ctx, h.a_key, d_z, d_r, d_d, B) == 0, h.err()
    assert h.lib.sc_paillier_one_minus(h.ctx, h.a_key, d_delta, d_sigma, B) == 0, h.err()
    c_out = {}
    for name, sel in (("min", d_sigma), ("cx", d_delta)):
        d_P, d_e, d_rab, d_prod = h.empty(B, 2 * nw), h.empty(1, B, ew), h.empty(1, B, nw), h.empty(1, B, 2 * nw)
        assert h.lib.sc_initiator_select_pack(h.ctx, h.a_key, KAPPA, 1, wp, sel, d_d, dev["r_a"], 2, dev["r_b"], bw, dev["rho_p"], ew, d_P, d_e,
                                              d_rab, B) == 0, h.err()
        assert h.lib.sc_keyholder_select_mult(h.ctx, h.b_key, KAPPA, 1, wp, d_P, dev["rho_q"], d_prod, B) == 0, h.err()
        if name == "min":
            d_out = h.empty(1, B, 2 * nw)
            assert h.lib.sc_initiator_select_finish(h.ctx, h.a_key, KAPPA, 1, wp, sel, d_d, d_x, d_prod, dev["r_a"], 2, d_e, ew, d_rab, d_out,
                                                    B) == 0, h.err()
            c_out[name] = h.ints(d_out, B, 2 * nw)
            assert h.decrypt(d_out, B) == [min(x, y) for x, y in zip(xs, ys)]
        else:
            d_out = h.empty(2, 1, B, 2 * nw)
            assert h.lib.sc_initiator_cx_finish(h.ctx, h.a_key, KAPPA, 1, wp, sel, d_d, d_x, d_y, d_prod, dev["r_a"], 2, d_e, ew, d_rab, None, None,
                                                d_out, 2 * B, B) == 0, h.err()
            c_out[name] = h.ints(d_out, 2 * B, 2 * nw)
    # the Python path
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=engine)
    alice_p = bob_p.public_copy()
    bob_d = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=engine, randomizer_bits=RBITS)
    alice_d = bob_d.public_copy()
    up = engine.upload
    bm = lambda rws, w: torch.stack([up([rws[b][i] for b in range(B)], w) for i in range(l + 1)])  # noqa: E731
    bd = BatchDraws(r=up([d.r for d in drs], nw), delta_a=engine.upload_u64([d.delta_a for d in drs]), rhos=bm([d.rhos for d in drs], h.ew),
                    permutation=None, rho_z=up([d.rho_z for d in drs], nw), r_bob_dgk=bm([[d.r_d] + d.r_beta for d in drs], h.er),
                    r_alice_dgk=bm([d.r_c for d in drs], h.er), rho_zeta_1=up([d.rho_zeta1 for d in drs], nw),
                    rho_zeta_2=up([d.rho_zeta2 for d in drs], nw), rho_delta_b=up([d.rho_delta_b for d in drs], nw))
    sd = SelectDraws(r_a=up([d[0] for d in draws], 2), r_b=up([d[1][0] for d in draws], bw).unsqueeze(0).contiguous(),
                     rho_p=up([d[2] for d in draws], nw), rho_products=up([d[3][0] for d in draws], nw).unsqueeze(0).contiguous())
    xt, yt = up(x_enc, 2 * nw), up(y_enc, 2 * nw)
    got_min, _ = secure_minimum_batch(xt, yt, l, alice_p, alice_d, bob_p, bob_d, bd, sd, kappa=KAPPA)
    assert engine.download(got_min) == c_out["min"]
    lo, hi = secure_compare_exchange_batch(xt, yt, l, alice_p, alice_d, bob_p, bob_d, bd, sd, kappa=KAPPA)
    assert engine.download(lo.contiguous()) + engine.download(hi.contiguous()) == c_out["cx"]


def test_argument_errors_are_host_checks(host_factory, keys):
    """A layout too wide for the key names its column, a null rho_p is refused, and a key holder with a narrower layout than the
    initiator packed gets SC_ERR_LAYOUT: argument checks (and one verdict word), never a device fault."""
    sk = oracle_paillier(keys, 1024)
    h = host_factory(sk, None)
    nw, B = h.nw, 8
    rng = random.Random(5)
    buf = lambda *s: h.empty(*s)  # noqa: E731
    d_ct = h.up([sm.enc(sk, 1)] * (4 * B), 2 * nw)
    d_small, d_out = buf(4 * B, nw), buf(2 * 4 * B, 2 * nw)
    # column 1 does not fit: 1024-bit N, kappa 40, widths (400, 600)
    wide = _widths([400, 600])
    calls = [
        lambda: h.lib.sc_initiator_cx_differences(h.ctx, h.a_key, KAPPA, 2, wide, d_ct, d_ct, d_ct, d_out, B),
        lambda: h.lib.sc_initiator_select_pack(h.ctx, h.a_key, KAPPA, 2, wide, d_ct, d_ct, d_small, 2, d_small, nw, d_small, nw, d_out, d_small, d_small, B),
        lambda: h.lib.sc_keyholder_select_mult(h.ctx, h.b_key, KAPPA, 2, wide, d_ct, d_small, d_out, B),
        lambda: h.lib.sc_initiator_select_finish(h.ctx, h.a_key, KAPPA, 2, wide, d_ct, d_ct, d_ct, d_ct, d_small, 2, d_small, nw, d_small, d_out, B),
        lambda: h.lib.sc_initiator_cx_finish(h.ctx, h.a_key, KAPPA, 2, wide, d_ct, d_ct, d_ct, d_ct, d_ct, d_small, 2, d_small, nw, d_small, None, None,
                                             d_out, 4 * B, B),
    ]
    for call in calls:
        assert call() == SC_ERR_ARG
        assert "column 1" in h.err(), h.err()
    assert h.lib.sc_initiator_select_pack(h.ctx, h.a_key, 63, 1, _widths([16]), d_ct, d_ct, d_small, 2, d_small, 2, d_small, 2, d_out, d_small,
                                          d_small, B) == SC_ERR_ARG and "kappa" in h.err()
    # rho_p null: no P without fresh randomness
    assert h.lib.sc_initiator_select_pack(h.ctx, h.a_key, KAPPA, 1, _widths([16]), d_ct, d_ct, d_small, 2, d_small, 2, None, 2, d_out, d_small,
                                          d_small, B) == SC_ERR_ARG
    assert "rho_p" in h.err()
    # the key holder needs the secret key
    assert h.lib.sc_keyholder_select_mult(h.ctx, h.a_key, KAPPA, 1, _widths([16]), d_ct, d_small, d_out, B) == SC_ERR_ARG
    # the initiator packs (l = 64, kappa = 40), the key holder announces (l = 16, kappa = 20): the documented layout error
    big, small = [64], [16]
    draws = [sm.draw(rng, KAPPA, big, sk.n) for _ in range(B)]
    bw = (64 + KAPPA + 2 + 31) // 32
    d_sigma = h.up([sm.enc(sk, 1)] * B, 2 * nw)
    d_d = h.up([sm.enc(sk, (1 << 64) + 12345)] * B, 2 * nw)
    d_P, d_e, d_rab = buf(B, 2 * nw), buf(1, B, bw), buf(1, B, nw)
    assert h.lib.sc_initiator_select_pack(h.ctx, h.a_key, KAPPA, 1, _widths(big), d_sigma, d_d, h.up([d[0] for d in draws], 2), 2,
                                          h.up([d[1][0] for d in draws], bw), bw, h.up([d[2] for d in draws], nw), bw, d_P, d_e, d_rab, B) == 0, h.err()
    d_rho = h.up([d[3][0] for d in draws], nw)
    assert h.lib.sc_keyholder_select_mult(h.ctx, h.b_key, 20, 1, _widths(small), d_P, d_rho, d_out, B) == SC_ERR_LAYOUT
    assert "exceeds the announced field layout" in h.err()
    assert h.lib.sc_keyholder_select_mult(h.ctx, h.b_key, KAPPA, 1, _widths(big), d_P, d_rho, d_out, B) == 0, h.err()

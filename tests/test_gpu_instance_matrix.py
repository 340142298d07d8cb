"""Deterministic parity matrix: every compiled k_vm / k_pvm instance (tests/_instance_matrix.py) is reached on purpose -- the launch
counters prove it -- and every primitive it can run is compared bit for bit with Python integers, at the smallest and largest moduli
of its configuration, with low limbs = -1, = 1 and random, at batch sizes around one wave and once around the grid-stride loop, every
output inside guard rows.  No tolerance anywhere: all comparisons are equalities of Python integers or of whole tensors."""
import math
import random

import pytest
import torch

import _instance_matrix as M

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
REACHED: dict = {}            # instance -> launches seen by this module


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def _guarded(eng, rows, words, dtype=torch.int32, fill=GUARD):
    """(buffer with one guard row on each side, the rows in between)."""
    buf = torch.full((rows + 2, words), fill, dtype=dtype, device=eng.device)
    return buf, buf[1:rows + 1]


def _guards_intact(buf, fill=GUARD):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


def _check(eng, label, expect, fn, rows, words, **inputs):
    """Run fn(out) on a guarded output; guards and inputs unchanged, result equal to `expect` (Python integers)."""
    buf, out = _guarded(eng, rows, words)
    clones = {k: v.clone() for k, v in inputs.items()}
    fn(out)
    torch.cuda.synchronize()
    assert _guards_intact(buf), (label, "a guard row was written")
    for k, v in clones.items():
        assert torch.equal(inputs[k], v), (label, f"input {k} was modified")
    got = eng.download(out)
    if got != expect:
        bad = [i for i, (a, b) in enumerate(zip(got, expect)) if a != b]
        raise AssertionError(f"{label}: {len(bad)} of {len(expect)} rows differ, first at row {bad[0]}")


def _grew(eng, before):
    after = eng.launch_counts()
    return {k: v - before.get(k, 0) for k, v in after.items() if v > before.get(k, 0)}


class _Switches:
    def __init__(self, eng, case):
        self.eng, self.case = eng, case

    def __enter__(self):
        self.eng.set_latency_mode(self.case.latency)
        self.eng.set_onelane_mode(self.case.onelane)
        self.eng.set_chip_share(self.case.chip_share)

    def __exit__(self, *exc):                 # the session engine's defaults (tests/conftest.py)
        self.eng.set_latency_mode(0)
        self.eng.set_onelane_mode(1)
        self.eng.set_chip_share(1)


def _num_cu(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def _tile(eng, rows, count):
    """`count` rows that repeat the distinct rows of `rows` ([TILE][words]) in order."""
    idx = torch.arange(count, device=eng.device) % rows.shape[0]
    return rows[idx].contiguous()


# ---- single-modulus primitives on one modulus ---------------------------------------------------------------------------------------
def _vm_case(eng, inst, case, j):
    n, ng = case.n, M.items_per_wave(inst)
    mod = eng.modulus(n)
    nw = mod.nwords
    counts = M.counts_for(inst)
    tag = f"{M.instance_id(inst)}/{case.label}"
    up = eng.upload
    onelane = inst[1:4] == M.ONE_LANE
    rng = random.Random(f"vm:{tag}")

    if not onelane:                                     # (the one-lane twin runs shared exponents only)
        for ci, count in enumerate(counts):
            a, b = M.operands(n, inst, count, ci), M.operands(n, inst, count, ci + 5)[::-1]
            ta, tb = up(a, nw), up(b, nw)
            _check(eng, f"{tag} modmul[{count}]", M.expected_modmul(n, a, b), lambda o: eng.modmul(mod, ta, tb, out=o), count, nw, a=ta, b=tb)
            one_b, one_a = up(b[:1], nw), up(a[:1], nw)
            _check(eng, f"{tag} modmul b broadcast[{count}]", M.expected_modmul(n, a, b[:1]), lambda o: eng.modmul(mod, ta, one_b, out=o), count, nw, a=ta, b=one_b)
            _check(eng, f"{tag} modmul a broadcast[{count}]", M.expected_modmul(n, a[:1], b), lambda o: eng.modmul(mod, one_a.reshape(nw), tb, out=o), count, nw, a=one_a, b=tb)
            c0, c1 = b[0], (n - 1 if ci % 2 else a[-1])
            _check(eng, f"{tag} modmul_const[{count}]", M.expected_modmul_const(n, a, c1), lambda o: eng.modmul_const(mod, ta, c1, out=o), count, nw, a=ta)
            fl = [(i * 7 + ci) % 3 == 0 for i in range(count)]
            fbuf, flags = _guarded(eng, count, 1, dtype=torch.uint8, fill=0x5A)
            flags = flags.reshape(count)
            flags.copy_(torch.tensor(fl, dtype=torch.uint8))
            for k0, k1 in ((c0, c1), (None, c1)):
                _check(eng, f"{tag} modmul_const_sel[{count}]", M.expected_modmul_const_sel(n, a, k0, k1, fl),
                       lambda o: eng.modmul_const_sel(mod, ta, k0, k1, flags, out=o), count, nw, a=ta, flags=fbuf)

    # shared exponents: every exponent at some count, the full-width one on NG - 1 items, the 400-bit one on NG + 1
    exps = M.shared_exponents(n)
    for k, e in enumerate(exps):
        count = counts[1] if k == len(exps) - 1 else (counts[3] if k == len(exps) - 2 else counts[(k + j) % 5])
        if onelane and e.bit_length() <= 64:
            continue
        xs = M.operands(n, inst, count, k + j)
        tx = up(xs, nw)
        if k % 2 == 0:
            _check(eng, f"{tag} modexp_shared e#{k}[{count}]", M.expected_modexp_shared(n, xs, e), lambda o: eng.modexp_shared(mod, tx, e, out=o), count, nw, x=tx)
        else:
            ys = M.operands(n, inst, count, k + j + 3)[::-1]
            ty = up(ys, nw)
            _check(eng, f"{tag} modexp_shared mul_into e#{k}[{count}]", M.expected_modexp_shared(n, xs, e, ys),
                   lambda o: eng.modexp_shared(mod, tx, e, mul_into=ty, out=o), count, nw, x=tx, mul_into=ty)
    count = counts[4]
    e = exps[6] if onelane else (3 if j % 2 else exps[6])
    for width in (2 * nw, 2 * nw + 2):
        wide = [rng.getrandbits(32 * width) for _ in range(count - 2)] + [(1 << (32 * width)) - 1, n]
        tw = up(wide, width)
        _check(eng, f"{tag} modexp_shared {width}-word operands", [pow(x % n, e, n) for x in wide], lambda o: eng.modexp_shared(mod, tw, e, out=o), count, nw, x=tw)

    # is-one flags with planted true cases: x = 1 and x = n - 1 (order 2) under the even exponent 2^64 + 2^65; no true case but 1 under 2^160 + 1
    for e in ((1 << 64) + (1 << 65), exps[6]):
        xs = M.operands(n, inst, count, 0)
        xs[5 % count] = n - 1
        xs[-1] = 1
        tx = up(xs, nw)
        want = M.expected_isone(n, xs, e)
        assert want[-1] == 1 and (e % 2 or want[5 % count] == 1)
        fbuf = torch.full((count + 32,), 0x5A, dtype=torch.uint8, device=eng.device)
        eng._sync_stream()
        eng._check(eng.lib.sc_modexp_shared_isone(eng.ctx, mod.id, eng.exponent(e), eng._ptr(tx), nw, fbuf[16:].data_ptr(), count))
        torch.cuda.synchronize()
        assert fbuf[16:16 + count].tolist() == want, f"{tag} isone"
        assert bool((fbuf[:16] == 0x5A).all()) and bool((fbuf[16 + count:] == 0x5A).all()), f"{tag} isone guards"
        inner = ng + 1
        planes = [M.operands(n, inst, inner, 2), M.operands(n, inst, inner, 4)]
        planes[1][0], planes[0][inner - 1] = 1, n - 1
        flat = planes[0] + planes[1]
        tf = up(flat, nw)
        abuf = torch.full((inner + 2,), GUARD, dtype=torch.int64, device=eng.device)
        eng._sync_stream()
        eng._check(eng.lib.sc_modexp_shared_isone_any(eng.ctx, mod.id, eng.exponent(e), eng._ptr(tf), nw, inner, abuf[1:].data_ptr(), 2 * inner))
        torch.cuda.synchronize()
        want = M.expected_isone_any(n, flat, e, inner)
        assert want[0] == 1 and abuf[1:inner + 1].tolist() == want and abuf[0].item() == GUARD and abuf[-1].item() == GUARD, f"{tag} isone_any"
    if onelane:
        return

    # per-row exponents, the fixed-base tail, the scattered store, fixed-base powers
    base = M.operands(n, inst, 12, 1)[11] | 2
    tables = {w: eng.fixed_base(mod, base, 10, window=w) for w in (1, 5)}
    for vi, ebits in enumerate(M.VAR_EBITS):
        count = counts[(vi + j) % 5]
        xs, es = M.operands(n, inst, count, vi), M.row_exponents(ebits, count, vi + j)
        tx, te = up(xs, nw), up(es, (ebits + 31) // 32)
        _check(eng, f"{tag} modexp_var ebits {ebits}[{count}]", M.expected_modexp_var(n, xs, es), lambda o: eng.modexp_var(mod, tx, te, ebits, out=o), count, nw, x=tx, e=te)
        e2 = M.row_exponents(10, count, vi)
        t2 = up(e2, 1)
        fb = tables[1 if vi % 2 else 5]
        _check(eng, f"{tag} modexp_var + table ebits {ebits}[{count}]", M.expected_modexp_var(n, xs, es, base, e2),
               lambda o: eng.modexp_var(mod, tx, te, ebits, fb, t2, out=o), count, nw, x=tx, e=te, e2=t2)
        perm = list(range(count))
        rng.shuffle(perm)
        dest = torch.tensor(perm, dtype=torch.int64, device=eng.device)
        _check(eng, f"{tag} modexp_var_scatter ebits {ebits}[{count}]", M.expected_modexp_var(n, xs, es, dest=perm),
               lambda o: eng.modexp_var(mod, tx, te, ebits, out=o, dest=dest), count, nw, x=tx, e=te, dest=dest)
        ys = M.operands(n, inst, count, vi + 2)[::-1]
        ty = up(ys, nw)
        _check(eng, f"{tag} fixedbase_pow window {fb.window}[{count}]", M.expected_fixedbase_pow(n, base, e2), lambda o: eng.fixedbase_pow(fb, t2, out=o), count, nw, e=t2)
        _check(eng, f"{tag} fixedbase_pow mul_into window {fb.window}[{count}]", M.expected_fixedbase_pow(n, base, e2, ys),
               lambda o: eng.fixedbase_pow(fb, t2, mul_into=ty, out=o), count, nw, e=t2, mul_into=ty)

    # inversion (division-step kernel: the instance is not involved below SC_INV_TOP, the operand set is the matrix's)
    count = counts[4]
    inv = M.coprime_operands(n, inst, count, j)
    ti = up(inv, nw)
    _check(eng, f"{tag} modinv", M.expected_modinv(n, inv), lambda o: eng.modinv(mod, ti, out=o), count, nw, x=ti)

    # exact-limb ops: L(x) k (OP_SUB1, OP_QUOT) on x = 1 + m n, m incl. 0 and n - 1
    count = counts[(j + 3) % 5]
    ms = [0, n - 1, 1][:count] + [rng.randrange(n) for _ in range(max(0, count - 3))]
    xs, k = [1 + m * n for m in ms], M.operands(n, inst, 9, 2)[8] | 1
    tx = up(xs, 2 * nw)
    _check(eng, f"{tag} paillier_l_mul[{count}]", M.expected_paillier_l_mul(n, k, xs), lambda o: eng.paillier_l_mul(mod, k, tx, out=o), count, nw, x=tx)
    # CRT recombination with this modulus as m_p and a 64-bit matrix modulus as m_q
    mq = M.make_modulus(64, "one")
    if (n * mq).bit_length() <= M.MAX_BITS and math.gcd(n, mq) == 1 and n > mq:
        full = eng.modulus(n * mq)
        a_p, a_q = M.operands(n, inst, count, 6), [0, mq - 1, 1][:count] + [rng.randrange(mq) for _ in range(max(0, count - 3))]
        tp, tq = up(a_p, nw), up(a_q, 2)
        _check(eng, f"{tag} crt_combine[{count}]", M.expected_crt_combine(n, mq, a_p, a_q), lambda o: eng.crt_combine(mod, full, mq, tp, tq, out=o),
               count, full.nwords, a_p=tp, a_q=tq)
    # Paillier's unrandomized encryption and its inverse (OP_NEG, OP_ADD1 + OP_CANON) where the modulus is a square N^2
    if case.label.endswith("square"):
        big_n = math.isqrt(n)
        assert big_n * big_n == n
        bw = (big_n.bit_length() + 31) // 32
        for count in counts:
            ms = [0, 1, big_n - 1, big_n, (1 << (32 * bw)) - 1][:count] + [rng.getrandbits(32 * bw) for _ in range(max(0, count - 5))]
            tm = up(ms, bw)
            _check(eng, f"{tag} paillier_encrypt_raw[{count}]", M.expected_paillier_encrypt_raw(big_n, ms), lambda o: eng.paillier_encrypt_raw(mod, big_n, tm, out=o), count, nw, m=tm)
            _check(eng, f"{tag} paillier_encrypt_raw_neg[{count}]", M.expected_paillier_encrypt_raw(big_n, ms, True),
                   lambda o: eng.paillier_encrypt_raw_neg(mod, big_n, tm, out=o), count, nw, m=tm)

    # compare-exchange finish (table entry, seven products, contiguous and indexed stores)
    nf, count = 2, ng + 1
    items = nf * count
    t, ab = M.coprime_operands(n, inst, items, 1), M.coprime_operands(n, inst, items, 2)[::-1]
    f, g = M.operands(n, inst, items, 3), M.operands(n, inst, items, 4)[::-1]
    u_inv = [pow(a * b % n, -1, n) for a, b in zip(t, ab)]
    lo, hi = M.expected_select_finish_cx(n, t, ab, u_inv, f, g)
    tt, tab, tu = up(t, nw), up(ab, nw), up(u_inv, nw)
    tf, tg = up(f, nw).reshape(nf, count, nw), up(g, nw).reshape(nf, count, nw)
    buf, out = _guarded(eng, 2 * items, nw)
    eng.select_finish_cx(mod, tt, tab, tu, tf, tg, out=out.view(2, nf, count, nw))
    torch.cuda.synchronize()
    assert _guards_intact(buf) and eng.download(out) == lo + hi, f"{tag} select_finish_cx"
    rows = 2 * items + 5
    where = rng.sample(range(rows), 2 * items)
    li = torch.tensor(where[:items], dtype=torch.int64, device=eng.device).reshape(nf, count)
    hi_i = torch.tensor(where[items:], dtype=torch.int64, device=eng.device).reshape(nf, count)
    buf, out = _guarded(eng, rows, nw)
    eng.select_finish_cx(mod, tt, tab, tu, tf, tg, lo_index=li, hi_index=hi_i, out=out)
    torch.cuda.synchronize()
    want = [int.from_bytes(b"\x5a" * (4 * nw), "little")] * rows
    for r, v in zip(where, lo + hi):
        want[r] = v
    assert _guards_intact(buf) and eng.download(out) == want, f"{tag} select_finish_cx indexed"

    # DGK step 4c .. 4h against the oracle's step arithmetic
    g_dgk = M.coprime_operands(n, inst, 12, 3)[11]
    for l in (1, 5):
        count = counts[(l + j) % 5]
        beta = [M.coprime_operands(n, inst, count, 10 + i) for i in range(l)]
        d = M.coprime_operands(n, inst, count, 9)
        alpha, alpha_t = [rng.getrandbits(l) for _ in range(count)], [rng.getrandbits(l) for _ in range(count)]
        rsmall, delta_a = [rng.getrandbits(1) for _ in range(count)], [rng.getrandbits(1) for _ in range(count)]
        want = M.expected_dgk_step4(n, g_dgk, l, beta, d, alpha, alpha_t, rsmall, delta_a)
        flat = [v for row in beta for v in row]
        tb, tbi = up(flat, nw), up([pow(v, -1, n) for v in flat], nw)
        td, tdi = up(d, nw), up([pow(v, -1, n) for v in d], nw)
        ta, tat, trs, tda = (eng.upload_u64(v) for v in (alpha, alpha_t, rsmall, delta_a))
        buf, out = _guarded(eng, (l + 1) * count, nw)
        ins = dict(beta=tb, beta_inv=tbi, d=td, d_inv=tdi, alpha=ta, alpha_tilde=tat, rsmall=trs, delta_a=tda)
        clones = {k: v.clone() for k, v in ins.items()}
        eng._sync_stream()
        eng._check(eng.lib.sc_dgk_step4(eng.ctx, mod.id, eng.constant(mod, g_dgk), eng.constant(mod, pow(g_dgk, -1, n)), l, eng._ptr(tb), eng._ptr(tbi),
                                        eng._ptr(td), eng._ptr(tdi), eng._ptr(ta), eng._ptr(tat), eng._ptr(trs), eng._ptr(tda), eng._ptr(out), count))
        torch.cuda.synchronize()
        assert _guards_intact(buf) and all(torch.equal(ins[k], v) for k, v in clones.items()), f"{tag} dgk_step4 l={l} guards"
        assert eng.download(out) == [v for row in want for v in row], f"{tag} dgk_step4 l={l}[{count}]"


# ---- pair primitives on one modulus -------------------------------------------------------------------------------------------------
def _pair_case(eng, inst, case, j, counts):
    n = case.n
    n2 = n * n
    mod, mod2 = eng.modulus(n), eng.modulus(n2)
    nw, nw2 = mod.nwords, mod2.nwords
    tag = f"{M.instance_id(inst)}/{case.label}"
    rng = random.Random(f"pair:{tag}")
    up = eng.upload
    if inst[6]:                                     # DIG: exponents per row, one to three bases
        for nb in (1, 2, 3):
            count, ebits = counts[(nb + j) % 5], (5, 35, 67)[(nb + j) % 3]
            xs = [[0, 1, n2 - 1, n][:count] + [rng.randrange(n2) for _ in range(max(0, count - 4))] for _ in range(nb)]
            es = [M.row_exponents(ebits, count, b + j) for b in range(nb)]
            tx = torch.stack([up(r, nw2) for r in xs]).contiguous()
            te = torch.stack([up(r, (ebits + 31) // 32) for r in es]).contiguous()
            mi = [rng.randrange(n2) for _ in range(count)]
            tm = up(mi, nw2)
            call = lambda o, m: eng._check(eng.lib.sc_modexp_var_sq(eng.ctx, mod.id, mod2.id, nb, eng._ptr(tx), nw2, eng._ptr(te), te.shape[-1], ebits,  # noqa: E731
                                                                    eng._ptr(m), eng._ptr(o), count))      # the pair kernel itself: no fallback
            eng._sync_stream()
            _check(eng, f"{tag} modexp_var_sq nb {nb} ebits {ebits}[{count}]", M.expected_modexp_var_sq(n2, xs, es), lambda o: call(o, None), count, nw2, x=tx, e=te)
            _check(eng, f"{tag} modexp_var_sq mul_into nb {nb}[{count}]", M.expected_modexp_var_sq(n2, xs, es, mi), lambda o: call(o, tm), count, nw2, x=tx, e=te, mul_into=tm)
        return
    # x^2 of a 4-chunk operand on every modulus: the call that came out wrong while a modulus whose multiple M = c n needs a word more
    # than the limbs hold still ran modulo M (the top bits of each full chunk were dropped)
    count = counts[1]
    xs = [0, 1, n2 - 1, n][:count] + [rng.randrange(n2) for _ in range(max(0, count - 4))]
    tx = up(xs, 4 * nw)
    _check(eng, f"{tag} modexp_shared_sq e = 2, 4 chunks[{count}]", [pow(x, 2, n2) for x in xs], lambda o: eng.modexp_shared_sq(mod, mod2, tx, 2, out=o), count, nw2, x=tx)
    exps = [e for e in M.shared_exponents(n) if e]
    for k, e in enumerate(exps):
        count = counts[1] if k == len(exps) - 1 else (counts[3] if k == len(exps) - 2 else counts[(k + j) % 5])
        chunks = (1, 2, 4)[(k + j) % 3]
        width = chunks * nw
        if chunks == 1:
            xs = M.operands(n, inst, count, k)
        else:
            xs = [0, 1, n2 - 1, n][:count] + [rng.randrange(n2) for _ in range(max(0, count - 4))]
        tx = up(xs, width)
        if k % 2:
            _check(eng, f"{tag} modexp_shared_sq e#{k} {chunks} chunk(s)[{count}]", [pow(x, e, n2) for x in xs],
                   lambda o: eng.modexp_shared_sq(mod, mod2, tx, e, out=o), count, nw2, x=tx)
        else:
            mi = [n2 - 1, 0, 1][:count] + [rng.randrange(n2) for _ in range(max(0, count - 3))]
            tm = up(mi, nw2)
            _check(eng, f"{tag} modexp_shared_sq mul_into e#{k} {chunks} chunk(s)[{count}]", [pow(x, e, n2) * v % n2 for x, v in zip(xs, mi)],
                   lambda o: eng.modexp_shared_sq(mod, mod2, tx, e, mul_into=tm, out=o), count, nw2, x=tx, mul_into=tm)


# ---- the grid-stride loop -------------------------------------------------------------------------------------------------------------
def _over_one_round(eng, inst, case):
    """Once per instance: more items than the resident waves of a full chip hold, so every wave loops and re-uses its scratch-table
    slot.  257 distinct operands tiled; the reference is tiled on the host side of the comparison and every row is compared."""
    n = case.n
    count = M.over_one_round(inst, _num_cu(eng))
    tag = f"{M.instance_id(inst)}/{case.label} over one round [{count}]"
    xs = M.operands(n, inst, M.TILE, 7)
    if inst[0] == "vm":
        mod = eng.modulus(n)
        nw = mod.nwords
        rows = eng.upload(xs, nw)
        tx = _tile(eng, rows, count)
        # 2^16 + 1; the one-lane twin only takes exponents of more than 64 bits: 2^64 + 2^16 + 1 there
        e = (1 << 16) + 1 + ((1 << 64) if inst[1:4] == M.ONE_LANE else 0)
        buf, out = _guarded(eng, count, nw)
        eng.modexp_shared(mod, tx, e, out=out)
        want = _tile(eng, eng.upload(M.expected_modexp_shared(n, xs, e), nw), count)
        assert torch.equal(out, want) and _guards_intact(buf) and torch.equal(tx, _tile(eng, rows, count)), f"{tag} modexp_shared"
        if inst[1:4] != M.ONE_LANE:
            es = M.row_exponents(5, M.TILE, 1)
            te = _tile(eng, eng.upload(es, 1), count)
            buf, out = _guarded(eng, count, nw)
            eng.modexp_var(mod, tx, te, 5, out=out)
            want = _tile(eng, eng.upload(M.expected_modexp_var(n, xs, es), nw), count)
            assert torch.equal(out, want) and _guards_intact(buf), f"{tag} modexp_var"
        return
    n2 = n * n
    mod, mod2 = eng.modulus(n), eng.modulus(n2)
    rows = eng.upload(xs, mod.nwords)
    tx = _tile(eng, rows, count)
    buf, out = _guarded(eng, count, mod2.nwords)
    if inst[6]:
        es = M.row_exponents(5, M.TILE, 1)
        te = _tile(eng, eng.upload(es, 1), count)
        eng._sync_stream()
        eng._check(eng.lib.sc_modexp_var_sq(eng.ctx, mod.id, mod2.id, 1, eng._ptr(tx), mod.nwords, eng._ptr(te), 1, 5, None, eng._ptr(out), count))
        want = [pow(x, e, n2) for x, e in zip(xs, es)]
    else:
        e = (1 << 16) + 1
        eng.modexp_shared_sq(mod, mod2, tx, e, out=out)
        want = [pow(x, e, n2) for x in xs]
    torch.cuda.synchronize()
    assert torch.equal(out, _tile(eng, eng.upload(want, mod2.nwords), count)) and _guards_intact(buf), tag


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", [i for i in M.INSTANCES if not i[5]], ids=M.instance_id)
def test_instance(engine, inst):
    """Every case of the instance, then the grid-stride batch.  Every modulus must land on the instance (its counter grows),
    whatever else its calls launch."""
    eng = engine
    cases = M.cases_for(inst)
    for j, case in enumerate(cases):
        before = eng.launch_counts()
        try:
            with _Switches(eng, case):
                if inst[0] == "vm":
                    _vm_case(eng, inst, case, j)
                else:
                    _pair_case(eng, inst, case, j, M.pair9_counts(inst, _num_cu(eng)) if case.pair9 else M.counts_for(inst))
        finally:                                     # reached or not is a fact of its own: a parity failure does not hide it
            REACHED[inst] = REACHED.get(inst, 0) + _grew(eng, before).get(inst, 0)
        assert _grew(eng, before).get(inst, 0) > 0, f"{M.instance_id(inst)}/{case.label}: no launch landed on the instance ({_grew(eng, before)})"
    # the grid-stride loop, on the last random modulus; k_pvm<2G, 9> only exists below the small-batch threshold (no public switch
    # makes it loop: _instance_matrix.py)
    if not (inst[0] == "pvm" and inst[2] == 9):
        case = [c for c in cases if c.label.endswith(("-rand", "-neg1"))][-1]
        before = eng.launch_counts()
        with _Switches(eng, case):
            _over_one_round(eng, inst, case)
        assert _grew(eng, before).get(inst, 0) > 0, f"{M.instance_id(inst)}: the large batch did not land on the instance"


def test_stamp_twin_is_reached_through_the_clock_probe(engine):
    """k_pvm<4, 18, NEG1, STAMP> runs inside sc_clock_probe only, which discards the residues: the matrix can observe its launch and
    the clock it reads, not its arithmetic (the same source as k_pvm<4, 18, NEG1>, plus the stamps)."""
    inst = ("pvm", 4, 18, 29, True, True, False)
    n = M.make_modulus(2048, "rand")
    key = engine.paillier_key(n)
    rho = engine.upload(M.coprime_operands(n, inst, 2 * 16 + 3), key.mod_n.nwords)
    keep = rho.clone()
    before = engine.launch_counts()
    ghz, ms = engine.clock_probe(key, rho)
    assert ghz > 0 and ms > 0 and torch.equal(rho, keep)
    grew = _grew(engine, before)
    assert grew.get(inst, 0) == 1 and ("pvm", 4, 18, 29, True, False, False) not in grew
    REACHED[inst] = 1


@pytest.mark.parametrize("which", [0, 1], ids=["small", "large"])
def test_modinv_across_the_tree_threshold(engine, which):
    """Batches of SC_INV_TOP - 1, SC_INV_TOP, SC_INV_TOP + 1 and 2 SC_INV_TOP + 1 residues (the division-step kernel alone, then one level
    of the product tree above it), bit-exact; and a single residue without an inverse -- first, last, at index SC_INV_TOP -- is an
    error return that names exactly that element."""
    from protocols.secure_comparison_amd.engine import NotInvertibleError

    factor, cofactor = M.NOT_INVERTIBLE[which]
    n = factor * cofactor
    mod = engine.modulus(n)
    inst = ("vm",) + M.first_fit(n.bit_length()) + (29, False, False, False)
    xs = M.coprime_operands(n, inst, M.TILE)
    rows, inv_rows = engine.upload(xs, mod.nwords), engine.upload(M.expected_modinv(n, xs), mod.nwords)
    for count in M.INV_COUNTS:
        tx = _tile(engine, rows, count)
        buf, out = _guarded(engine, count, mod.nwords)
        engine.modinv(mod, tx, out=out)
        assert torch.equal(out, _tile(engine, inv_rows, count)) and _guards_intact(buf) and torch.equal(tx, _tile(engine, rows, count)), count
    count = M.INV_COUNTS[-1]
    bad_row = engine.upload([factor], mod.nwords)[0]
    for index in (0, count - 1, M.INV_TOP):
        tx = _tile(engine, rows, count)
        tx[index] = bad_row
        with pytest.raises(NotInvertibleError) as err:
            engine.modinv(mod, tx)
        assert err.value.index == index
    assert engine.download(engine.modinv(mod, rows[:5].contiguous())) == M.expected_modinv(n, xs[:5])       # the engine works on


def test_every_compiled_instance_was_reached():
    """The union over this module: all 37 instances (run the whole module; a deselected instance shows up here as missing)."""
    missing = [M.instance_id(i) for i in M.INSTANCES if not REACHED.get(i)]
    print(f"instances reached: {len(M.INSTANCES) - len(missing)} of {len(M.INSTANCES)}")
    assert not missing, f"not reached: {missing}"

"""The plain-word kernels of the multiplication, the inner product and the one-hot encoding at their own edges (the MUL_, DOT_, ONEHOT_
and ROTATE_ tables of tests/_kernel_edges.py), through the dev entry points sc_mul_prep / sc_mul_split, sc_dot_prep / sc_dot_split and
sc_onehot_prep / sc_onehot_split / sc_onehot_rotate: no key, no encryption, no interpreter.  Every word of every output row is compared
with Python integers; every output lies between guard rows and starts as the guard pattern, every input is compared with a clone."""
import ctypes as C

import numpy as np
import pytest
import torch

import _kernel_edges as K
from test_gpu_instance_matrix import GUARD, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

SC_ERR_ARG = -1


def _tile(seq, count):
    return [seq[i % len(seq)] for i in range(count)]


def _flat(planes):
    return [v for plane in planes for v in plane]


class _Call:
    """One call of a dev entry point: guarded outputs, cloned inputs, and the comparison of both afterwards."""

    def __init__(self, engine, label):
        self.e, self.label, self.ins, self.outs = engine, label, [], []

    def modulus(self, nbits):
        n = K.family_modulus(nbits)
        return self.e._host_n_words(n, K.words_of(nbits))[1]

    def inp(self, name, values, words):
        t = self.e.upload(values, words)
        self.ins.append((name, t, t.clone()))
        return self.e._ptr(t)

    def inp_i32(self, name, values):
        t = torch.tensor(values, dtype=torch.int32, device=self.e.device)
        self.ins.append((name, t, t.clone()))
        return self.e._ptr(t)

    def out(self, name, rows, words):
        buf, view = _guarded(self.e, rows, words)
        self.outs.append((name, buf, view))
        return self.e._ptr(view)

    def verdict(self):
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.e.device)
        return self.e._ptr(self.bad)

    def run(self, fn, *args, expect_rc=0):
        self.e._sync_stream()
        rc = fn(self.e.ctx, *args)
        self.e.synchronize()
        assert rc == expect_rc, (self.label, rc, self.e.lib.sc_last_error(self.e.ctx))
        for name, buf, _ in self.outs:
            assert _guards_intact(buf), (self.label, name, "a guard row was written")
        for name, t, keep in self.ins:
            assert torch.equal(t, keep), (self.label, name, "an input was modified")

    def check(self, name, want, shape=None):
        """Every word of the output `name` against the integers `want` (flat, row-major)."""
        view = next(v for n, _, v in self.outs if n == name)
        got = view.reshape(-1).tolist() if shape == "i32" else self.e.download(view)
        if got != want:
            first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
            diff = got[first] ^ want[first] if shape != "i32" else 0
            raise AssertionError(f"{self.label}: {name}: {sum(a != b for a, b in zip(got, want))} of {len(want)} rows differ, first at flat row "
                                 f"{first}, lowest differing word {((diff & -diff).bit_length() - 1) // 32 if diff else '-'}")

    def untouched(self):
        for name, _, view in self.outs:
            assert bool((view == GUARD).all()), (self.label, name, "written by a refused call")

    def check_verdict(self, want, rows, ends):
        got = int(self.bad.item())
        assert got == want, (self.label, f"verdict {got}, expected {want}", "first (row, message, bit) above its end:", K.first_over(rows, ends))


def _wy(c):
    return np.array(c.wy, dtype=np.int32)


# ==== multiplication =================================================================================================================
def _mul_id(c):
    return f"{c.nbits}-k{c.kappa}-{c.wx}x" + "x".join(str(w) for w in c.wy) + ("-s" if c.signed else "")


def _mul_prep(engine, c, draws, label, wy=None, expect_rc=0):
    nw, nf, count = K.words_of(c.nbits), len(c.wy), len(draws)
    call = _Call(engine, label)
    wy = _wy(c) if wy is None else wy
    args = (call.modulus(c.nbits), nw, c.kappa, c.wx, nf, wy.ctypes.data_as(C.c_void_p), int(c.signed),
            call.inp("r_a", [d[0] for d in draws], c.aw), c.aw, call.inp("r_b", [d[1][j] for j in range(nf) for d in draws], c.bw), c.bw, c.ew,
            call.out("R", count, nw), call.out("e", (nf + 1) * count, c.ew), call.out("rab", nf * count, nw), count)
    call.run(engine.lib.sc_mul_prep, *args, expect_rc=expect_rc)
    return call


def _mul_split(engine, c, ps, label, wy=None, expect_rc=0):
    nw, nf, count = K.words_of(c.nbits), len(c.wy), len(ps)
    call = _Call(engine, label)
    wy = _wy(c) if wy is None else wy
    call.run(engine.lib.sc_mul_split, call.modulus(c.nbits), nw, c.kappa, c.wx, nf, wy.ctypes.data_as(C.c_void_p), call.inp("P", ps, nw),
             call.out("prod", nf * count, nw), call.verdict(), count, expect_rc=expect_rc)
    return call


@pytest.mark.parametrize("c", K.MUL_LAYOUTS, ids=_mul_id)
def test_mul_prep(engine, c):
    all_draws = K.mul_draws(c)
    for count in (K.BLOCK_BATCHES if c == K.MUL_LAYOUTS[0] else (len(all_draws),)):
        draws = all_draws[10:11] if count == 1 else _tile(all_draws, count)      # (one row: all ones against all ones)
        call = _mul_prep(engine, c, draws, f"k_mul_prep {_mul_id(c)} [{count}]")
        want = K.expected_mul_prep(c, draws)
        call.check("R", want["R"])
        call.check("e", _flat(want["e"]))
        call.check("rab", _flat(want["rab"]))


@pytest.mark.parametrize("c", K.MUL_LAYOUTS, ids=_mul_id)
def test_mul_split(engine, c):
    nw = K.words_of(c.nbits)
    _, _, _, end = K.mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    all_ps = K.mul_p_rows(c)
    for count in (K.BLOCK_BATCHES if c == K.MUL_LAYOUTS[0] else (len(all_ps),)):
        ps = _tile(all_ps, count)                                # the first row has its highest bit at end - 1
        call = _mul_split(engine, c, ps, f"k_mul_split {_mul_id(c)} [{count}]")
        call.check("prod", _flat(K.expected_mul_split(c, ps)["prod"]))
        call.check_verdict(0, [ps], [end])
    # one row above the layout, in the first and in the second block: the verdict is 1, the products are still written
    clean = _tile(all_ps, 257)
    for row in (3, 256):
        for name, bit in K.bad_bits(end, nw).items():
            ps = K.plant([clean], 0, row, bit)[0]
            call = _mul_split(engine, c, ps, f"k_mul_split {_mul_id(c)} row {row} bit {bit} ({name})")
            want = K.expected_mul_split(c, ps)
            call.check("prod", _flat(want["prod"]))
            call.check_verdict(1, [ps], [end])


@pytest.mark.parametrize("c", [c for c in K.MUL_LAYOUTS if "end in the top word of N (the largest)" in K.mul_conditions(c)], ids=_mul_id)
def test_mul_one_bit_more_is_refused_with_nothing_launched(engine, c):
    wider = np.array(c.wy[:-1] + (c.wy[-1] + 1,), dtype=np.int32)
    _mul_prep(engine, c, K.mul_draws(c)[:4], f"sc_mul_prep {_mul_id(c)} + 1 bit", wy=wider, expect_rc=SC_ERR_ARG).untouched()
    call = _mul_split(engine, c, K.mul_p_rows(c)[:4], f"sc_mul_split {_mul_id(c)} + 1 bit", wy=wider, expect_rc=SC_ERR_ARG)
    call.untouched()
    assert int(call.bad.item()) == 0


# ==== inner product ==================================================================================================================
def _dot_id(c):
    return f"{c.nbits}-k{c.kappa}-{c.wx}x{c.wy}-n{c.k}" + ("-s" if c.signed else "") + ("-sq" if c.square else "")


def _dot_prep(engine, c, draws, label):
    nw, count, M_ = K.words_of(c.nbits), len(draws), K.dot_of(c)[4]
    call = _Call(engine, label)
    ra = call.inp("r_a", [d[0][j] for j in range(c.k) for d in draws], c.aw)
    rb = C.c_void_p(0) if c.square else call.inp("r_b", [d[1][j] for j in range(c.k) for d in draws], c.bw)
    call.run(engine.lib.sc_dot_prep, call.modulus(c.nbits), nw, c.kappa, c.wx, c.wy, int(c.signed), int(c.square), c.k, ra, c.aw, rb, c.bw, c.ew,
             call.out("e", (c.k if c.square else 2 * c.k) * count, c.ew), call.out("R", M_ * count, nw), call.out("S", count, nw), count)
    return call


def _dot_split(engine, c, P, label):
    nw, count, M_ = K.words_of(c.nbits), len(P[0]), K.dot_of(c)[4]
    call = _Call(engine, label)
    call.run(engine.lib.sc_dot_split, call.modulus(c.nbits), nw, c.kappa, c.wx, c.wy, int(c.square), c.k, call.inp("P", _flat(P), nw),
             call.out("D", count, nw), call.verdict(), count)
    return call


@pytest.mark.parametrize("c", K.DOT_LAYOUTS, ids=_dot_id)
def test_dot_prep(engine, c):
    all_draws = K.dot_draws(c)
    for count in (K.BLOCK_BATCHES if c == K.DOT_LAYOUTS[0] else (len(all_draws),)):
        draws = _tile(all_draws, count)                          # the first row has every mask at its maximum
        call = _dot_prep(engine, c, draws, f"k_dot_prep {_dot_id(c)} [{count}]")
        want = K.expected_dot_prep(c, draws)
        call.check("e", _flat(want["e"]))
        call.check("R", _flat(want["R"]))
        call.check("S", want["S"])


@pytest.mark.parametrize("c", K.DOT_LAYOUTS, ids=_dot_id)
def test_dot_split(engine, c):
    nw, ends = K.words_of(c.nbits), K.dot_ends(c)
    all_P = K.dot_p_rows(c)
    for count in (K.BLOCK_BATCHES if c == K.DOT_LAYOUTS[0] else (len(all_P[0]),)):
        P = [_tile(row, count) for row in all_P]                 # the first row: every field all ones, every message up to its end - 1
        call = _dot_split(engine, c, P, f"k_dot_split {_dot_id(c)} [{count}]")
        call.check("D", K.expected_dot_split(c, P)["D"])
        call.check_verdict(0, P, ends)
    # every message against its OWN end: one bit in the first, a middle and the last message, in the last row (the smallest layout: row
    # 256, the second block)
    clean = [_tile(row, 257) for row in all_P] if c == K.DOT_LAYOUTS[0] else all_P
    row = len(clean[0]) - 1
    for mm in K.dot_bad_messages(c):
        for name, bit in K.bad_bits(ends[mm], nw).items():
            P = K.plant(clean, mm, row, bit)
            call = _dot_split(engine, c, P, f"k_dot_split {_dot_id(c)} message {mm} row {row} bit {bit} ({name})")
            call.check("D", K.expected_dot_split(c, P)["D"])
            call.check_verdict(1, P, ends)


# ==== one-hot ========================================================================================================================
def _onehot_id(c):
    return f"{c.nbits}-k{c.kappa}-ib{c.ib}-n{c.k}-m{c.m}"


def _onehot_split(engine, c, P, label):
    nw, count = K.words_of(c.nbits), len(P[0])
    call = _Call(engine, label)
    call.run(engine.lib.sc_onehot_split, call.modulus(c.nbits), nw, c.kappa, c.ib, c.k, c.m, call.inp("P", _flat(P), nw),
             call.out("prod", c.m * c.k * count, nw), call.verdict(), count)
    return call


@pytest.mark.parametrize("c", K.ONEHOT_LAYOUTS, ids=_onehot_id)
def test_onehot_prep(engine, c):
    nw, M_ = K.words_of(c.nbits), K.onehot_of(c)[2]
    all_draws = K.onehot_draws(c)
    for count in (K.BLOCK_BATCHES if c == K.ONEHOT_LAYOUTS[0] else (c.count,)):          # one thread per message: M count items
        draws = _tile(all_draws, count)
        call = _Call(engine, f"k_onehot_prep {_onehot_id(c)} [{count}]")
        call.run(engine.lib.sc_onehot_prep, call.modulus(c.nbits), nw, c.kappa, c.ib, c.k, c.m,
                 call.inp("r", [d[q] for q in range(c.m) for d in draws], c.rw), c.rw, call.out("R", M_ * count, nw), call.out("rot", c.m * count, 1),
                 count)
        want = K.expected_onehot_prep(c, draws)
        call.check("R", _flat(want["R"]))
        call.check("rot", _flat(want["rot"]), shape="i32")


@pytest.mark.parametrize("c", K.ONEHOT_LAYOUTS, ids=_onehot_id)
def test_onehot_split(engine, c):
    ends, M_ = K.onehot_ends(c), K.onehot_of(c)[2]
    all_P = K.onehot_p_rows(c)
    for count in (K.WAVE_ROWS if c == K.ONEHOT_LAYOUTS[0] else (c.count,)):              # one wave per row: m k count rows, four to a block
        P = [_tile(row, count) for row in all_P]                 # the first row: every field all ones
        call = _onehot_split(engine, c, P, f"k_onehot_split {_onehot_id(c)} [{count}]")
        want = K.expected_onehot_split(c, P)
        call.check("prod", [v for q in want["prod"] for t in q for v in t])              # a row's value: the mark in word 0, every other word 0
        call.check_verdict(0, P, ends)
    for mm in sorted({0, M_ - 1}):
        for name, bit in K.onehot_bad_bits(c, mm).items():
            P = K.plant(all_P, mm, len(all_P[0]) - 1, bit)
            call = _onehot_split(engine, c, P, f"k_onehot_split {_onehot_id(c)} message {mm} bit {bit} ({name})")
            want = K.expected_onehot_split(c, P)
            call.check("prod", [v for q in want["prod"] for t in q for v in t])
            call.check_verdict(1, P, ends)


@pytest.mark.parametrize("case", K.ROTATE_CASES, ids=lambda v: "x".join(str(x) for x in v))
def test_onehot_rotate(engine, case):
    words, k, m, count = case
    e, rot = K.rotate_input(words, k, m, count), K.rotate_rot(k, m, count)
    call = _Call(engine, f"k_onehot_rotate {case}")
    call.run(engine.lib.sc_onehot_rotate, words, k, m, call.inp("e", [v for q in e for t in q for v in t], words), call.inp_i32("rot", rot),
             call.out("out", m * k * count, words), count)
    call.check("out", [v for q in K.expected_rotate(k, m, count, e, rot) for t in q for v in t])


def test_onehot_rotate_refuses_an_output_that_overlaps_its_input(engine):
    words, k, m, count = 65, 5, 1, 1
    e = K.rotate_input(words, k, m, count)
    for shift in (0, 1, k - 1):                                  # the same array, and arrays that share their first or last row
        call = _Call(engine, f"sc_onehot_rotate, out {shift} rows above e")
        buf = call.e.upload([v for q in e for t in q for v in t] + [0] * (k * shift), words)
        keep = buf.clone()
        engine._sync_stream()
        rc = engine.lib.sc_onehot_rotate(engine.ctx, words, k, m, engine._ptr(buf), call.inp_i32("rot", [[1]]), engine._ptr(buf[shift:]), count)
        engine.synchronize()
        assert rc == SC_ERR_ARG and b"overlaps" in engine.lib.sc_last_error(engine.ctx) and torch.equal(buf, keep), (shift, rc)

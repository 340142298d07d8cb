"""csrc/sc_plain_words.h, the bit-field and multi-word helpers under the plain-word kernels of the four families, against Python
integers -- without a GPU and without the library: a small program that includes the header alone is built with g++ and answers every
query of this module in one run.  Comparison is by equality.  The inputs are the smallest at which each helper can go wrong: shifts of
0, 31, 32 and 33 bits, fields that end in a row's last bit, words asked for past a field and past a row, carries that run through
every word, streams that end on and one bit behind a word boundary, a bit planted just below and just at an end."""
import os
import random
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc")
MASK = 0xffffffff
JUNK = 0xdeadbeef                 # what a row holds before the stream writer has been over it, and the word behind the row for good

PROGRAM = r"""
#include "sc_plain_words.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace sc;

static void put(const uint32_t* w, int n) { for (int i = 0; i < n; i++) printf(i + 1 < n ? "%u " : "%u\n", w[i]); }

template <int N>
static void add(const std::vector<uint32_t>& x, int xw, int bit) {
  uint32_t v[N];
  add_bit(x.data(), xw, bit, v);
  put(v, N);
}
// fields of N words each, as (bits, words) .., pushed into a row of nw words of junk with one more word of junk behind it
template <int N>
static void stream(const std::vector<uint32_t>& q, int nw) {
  std::vector<uint32_t> row(nw + 1, 0xdeadbeefu);
  BitStream s = {row.data(), 0, 0};
  for (size_t at = 0; at + N < q.size(); at += N + 1) {
    uint32_t v[N];
    for (int w = 0; w < N; w++) v[w] = q[at + 1 + w];
    stream_push(s, v, (int)q[at]);
  }
  stream_finish(s, row.data() + nw);
  put(row.data(), nw + 1);
}

int main() {
  std::string line, cmd;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    long long p[5] = {0};
    in >> cmd;
    const int np = cmd == "field" ? 4 : cmd == "over" ? 4 : cmd == "stream" ? 2 : 3;      // the parameters, then the words
    for (int i = 0; i < np; i++) in >> p[i];
    std::vector<uint32_t> w;
    for (unsigned long long v; in >> v;) w.push_back((uint32_t)v);
    w.push_back(0u);                                                                      // never an empty array
    const int n = (int)w.size() - 1;
    if (cmd == "field") printf("%u\n", field_word(w.data(), (int)p[0], (int)p[1], (int)p[2], (int)p[3]));
    else if (cmd == "shl") printf("%u\n", shl_word(w.data(), (int)p[0], (int)p[1], (int)p[2]));
    else if (cmd == "add" && p[0] == 3) add<3>(w, (int)p[1], (int)p[2]);
    else if (cmd == "add" && p[0] == 10) add<10>(w, (int)p[1], (int)p[2]);
    else if (cmd == "stream" && p[0] == 3) { w.pop_back(); stream<3>(w, (int)p[1]); }
    else if (cmd == "stream" && p[0] == 10) { w.pop_back(); stream<10>(w, (int)p[1]); }
    else if (cmd == "over") printf("%d\n", (int)(bits_from(w.data(), (int)p[0], (int)p[1], (int)p[2], (int)p[3]) != 0u));
    else if (cmd == "mul64") {
      const uint64_t a = ((uint64_t)(uint32_t)p[1] << 32) | (uint32_t)p[0];
      const int nw = (int)p[2], bw = n;
      std::vector<uint32_t> out(nw);
      const uint32_t* b = w.data();
      mul64_words(a, [=](int k) { return k < bw ? b[k] : 0u; }, out.data(), nw);
      put(out.data(), nw);
    } else { fprintf(stderr, "unknown query: %s\n", line.c_str()); return 2; }
  }
  return 0;
}
"""


def words(x, n):
    return [(x >> (32 * i)) & MASK for i in range(n)]


class Queries:
    """Collects the queries of one run with the answer Python expects for each; `run` compares them all."""

    def __init__(self):
        self.lines, self.want = [], []

    def ask(self, want, cmd, *args):
        self.lines.append(" ".join([cmd] + [str(int(a)) for a in args]))
        self.want.append([int(v) for v in want] if isinstance(want, (list, tuple)) else [int(want)])

    def run(self, exe):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(self.lines)
        for line, got, want in zip(self.lines, out, self.want):
            assert [int(t) for t in got.split()] == want, line
        return len(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    d = tmp_path_factory.mktemp("plain_words")
    src, out = d / "plain_words.cpp", d / "plain_words"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", CSRC, str(src), "-o", str(out)], check=True)
    return str(out)


def rows_of(nw, seed):
    """Row contents of nw words: every bit set, and a fixed random pattern with both end bits set."""
    rng = random.Random(1000 * nw + seed)
    return [(1 << (32 * nw)) - 1, rng.getrandbits(32 * nw) | 1 | 1 << (32 * nw - 1)]


def test_header_is_plain_cxx_without_the_gpu_runtime():
    text = open(os.path.join(CSRC, "sc_plain_words.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "namespace sc {" in text
    assert [ln for ln in text.splitlines() if ln.startswith("#include")] == ["#include <stdint.h>"]
    assert [ln for ln in text.splitlines() if ln.startswith(("#if", "#elif"))] == ["#ifdef __HIPCC__"]           # no slice per unit
    for unit in ("sc_kernel_plain.h", "sc_launch_mul.hip", "sc_launch_dot.hip", "sc_launch_lookup.hip"):
        assert '#include "sc_plain_words.h"' in open(os.path.join(CSRC, unit)).read(), unit
    for unit in ("sc_launch_mul.hip", "sc_launch_dot.hip", "sc_launch_lookup.hip"):                             # their kernels are their own
        assert "sc_kernel_plain.h" not in open(os.path.join(CSRC, unit)).read(), unit


POSITIONS = (0, 31, 32, 33, 63)
FIELD_BITS = (1, 31, 32, 33, 64, 95)


def test_field_word_and_shl_word(exe):
    q = Queries()
    ends_in_last_bit = 0
    for nw in (1, 2, 3):
        for x in rows_of(nw, 1):
            for bits in FIELD_BITS:
                last = [32 * nw - bits] if 32 * nw >= bits else []              # the field that ends in the row's last bit
                ends_in_last_bit += len(last)
                for pos in sorted(set(POSITIONS) | set(last)):
                    field = (x >> pos) & ((1 << bits) - 1)
                    for k in range((bits + 31) // 32 + 2):                      # two words past the field; past the row where pos is high
                        q.ask((field >> (32 * k)) & MASK, "field", nw, pos, bits, k, *words(x, nw))
            for pos in POSITIONS:
                for k in range(nw + 4):                                         # x << 63 ends in word nw + 1: two words past that
                    q.ask(((x << pos) >> (32 * k)) & MASK, "shl", nw, pos, k, *words(x, nw))
    assert ends_in_last_bit == 2 * (3 + 5 + 6)
    q.run(exe)


def test_add_bit(exe):
    q = Queries()
    for n in (3, 10):
        top, full = 32 * n - 1, (1 << (32 * n)) - 1
        for bit in (-1, 0, 31, 32, top):
            low = (1 << bit) - 1 if bit >= 0 else 0
            # nothing; all ones below the bit; all ones from the bit up (the carry runs through every word above); all ones
            for x in (0, low, full ^ low, full):
                q.ask(words((x + (1 << bit if bit >= 0 else 0)) & full, n), "add", n, n, bit, *words(x, n))
            for x in (0, MASK, 1 << 31):                                        # one word under a wider array
                q.ask(words(x + (1 << bit if bit >= 0 else 0), n), "add", n, 1, bit, x)
        # words of x past the array are not looked at
        q.ask(words(5 + (1 << 31), n), "add", n, 1, 31, 5, MASK, MASK)
    assert q.run(exe) == 2 * (5 * 7 + 1)


STREAM_BITS = (3, 32, 33, 64, 95)


def stream_query(q, n, nw, fields):
    """`fields`, (bits, value) each, packed low bits first into a row of nw words; the word behind the row keeps its junk."""
    args, total, at = [], 0, 0
    for bits, v in fields:
        assert v >> bits == 0 and bits <= 32 * n
        args += [bits] + words(v, n)
        total |= v << at
        at += bits
    assert at <= 32 * nw
    q.ask(words(total, nw) + [JUNK], "stream", n, nw, *args)
    return at


def test_bit_stream(exe):
    q = Queries()
    rng = random.Random(7)
    ends = set()
    for n in (3, 10):
        for nw in (1, 2, 3, 4, 7, 8, 11, 15):
            for start in range(len(STREAM_BITS)):
                for ones in (True, False):
                    fields, at, i = [], 0, start
                    while at + STREAM_BITS[i % 5] <= 32 * nw:                   # until the next field no longer fits the row
                        bits = STREAM_BITS[i % 5]
                        fields.append((bits, (1 << bits) - 1 if ones else rng.getrandbits(bits) | 1 << (bits - 1)))
                        at, i = at + bits, i + 1
                    ends.add((stream_query(q, n, nw, fields) % 32, nw - (at + 31) // 32))
        # nothing pending at the end, with and without words left to fill; one bit pending; an empty stream
        assert stream_query(q, n, 5, [(32, MASK), (64, (1 << 64) - 1)]) == 96
        assert stream_query(q, n, 6, [(32, MASK), (64, (1 << 64) - 1)] * 2) == 32 * 6
        assert stream_query(q, n, 3, [(33, (1 << 33) - 1)]) == 33
        assert stream_query(q, n, 4, [(32, 1 << 31), (64, 1 << 63), (1, 1)]) == 97
        assert stream_query(q, n, 4, [(95, (1 << 95) - 1), (33, 1 << 32)]) == 32 * 4
        assert stream_query(q, n, 2, []) == 0
    # the sequences themselves end on a boundary and off it, with a full row and with words left to fill
    assert {e for e, _ in ends} >= {0, 1, 3} and {0, 1, 2} <= {left for _, left in ends}
    q.run(exe)


def over_reference(x, nw, end, first, step):
    """Has one of the words (end >> 5) + first, + step, .. of x a bit at or above `end`?"""
    return any((x >> max(end, 32 * k)) & ((1 << (32 * (k + 1) - max(end, 32 * k))) - 1) for k in range((end >> 5) + first, nw, step))


def test_bits_from(exe):
    q = Queries()
    for nw in (1, 2, 3):
        for end in sorted({0, 31, 32, 32 * nw - 1, 32 * nw} & set(range(32 * nw + 1))):
            below = (1 << end) - 1
            rows = [(0, 0), (below, 0)]                                         # nothing; every bit below the end
            if end:
                rows += [(1 << (end - 1), 0)]                                   # the bit just below: clean
            if end < 32 * nw:
                rows += [(1 << end, 1), (below | 1 << end, 1), (1 << (32 * nw - 1), 1)]
            for x, want in rows:
                assert over_reference(x, nw, end, 0, 1) == bool(want) == bool(x >> end)
                q.ask(want, "over", nw, end, 0, 1, *words(x, nw))
    shares = set()
    for nw in (65, 128):
        for end in (0, 31, 32, 32 * 64, 32 * nw - 1, 32 * nw):
            planted = [0, (1 << end) - 1] + [1 << b for b in (end - 1, end, end + 32, 32 * 64, 32 * 64 + 31, 32 * nw - 1) if 0 <= b < 32 * nw]
            for x in planted:
                caught = 0
                for lane in range(64):
                    want = over_reference(x, nw, end, lane, 64)
                    caught += want
                    shares.add((nw, lane, len(range((end >> 5) + lane, nw, 64)) > 0))
                    q.ask(want, "over", nw, end, lane, 64, *words(x, nw))
                assert caught == (1 if x >> end else 0)                        # one planted bit: the one lane whose word it is in
    for nw in (65, 128):                                                        # every lane's share is empty once and non-empty once
        assert all((nw, lane, some) in shares for lane in range(64) for some in (False, True))
    q.run(exe)


def test_mul64_words(exe):
    q = Queries()
    rng = random.Random(11)
    for bw in (1, 2, 3):
        b_ones = (1 << (32 * bw)) - 1
        for nw in (1, 2, bw + 2):
            for a in ((1 << 64) - 1, MASK, 1 << 32, 1, 0, rng.getrandbits(64)):
                for b in (b_ones, rng.getrandbits(32 * bw)):
                    q.ask(words((a * b) & ((1 << (32 * nw)) - 1), nw), "mul64", a & MASK, a >> 32, nw, *words(b, bw))
    assert q.run(exe) == 3 * 3 * 6 * 2

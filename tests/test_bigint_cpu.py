"""csrc/sc_bigint.h, the set-up-time integers every key object, Montgomery constant and fixed-base table is derived through, against
Python integers -- without a GPU and without the library: a small program that includes the header alone is built with g++ and answers
every query of this module in ONE run.  Comparison is by equality.  The inputs are the smallest at which each helper can go wrong:
dividends below, at and at a multiple of the divisor and with every bit set, operands of 1, 2 and 5 words, divisors shorter than the
dividend; shifts by nothing and across a word, of operands at and above the modulus; exponents 0, 1 and with an empty top word; inverses
of 1, of m - 1 and of a random unit modulo 1 and 3 words; limbs whose last one straddles the end of the last word with one more wholly
beyond it.  The last test holds the shape of the host sources: no header with an unnamed namespace, no unit included by another."""
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc")
MASK = 0xffffffff

PROGRAM = r"""
#include "sc_bigint.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace sc_host;

static void put(const Big& w) { for (size_t i = 0; i < w.size(); i++) printf(i ? " %u" : "%u", w[i]); }
static void line(const Big& w) { put(w); printf("\n"); }

// a query: the helper, its integer parameters, then `;` before every operand's words
int main() {
  std::string text, cmd, tok;
  while (std::getline(std::cin, text)) {
    std::istringstream in(text);
    in >> cmd;
    std::vector<long long> p;
    std::vector<Big> v;
    while (in >> tok) {
      if (tok == ";") v.push_back(Big());
      else if (v.empty()) p.push_back(std::stoll(tok));
      else v.back().push_back((uint32_t)std::stoull(tok));
    }
    if (cmd == "mul") line(big_mul(v[0], v[1]));
    else if (cmd == "divmod") { Big q, r; big_divmod(v[0], v[1], &q, &r); put(q); printf(" ; "); line(r); }
    else if (cmd == "shl") line(big_shl_mod(v[0], v[1], (int)p[0]));
    else if (cmd == "pow") line(big_powmod(v[0], v[1], v[2]));
    else if (cmd == "inv") line(big_modinv_odd(v[0], v[1]));
    else if (cmd == "limbs") line(to_limbs(v[0], (int)p[0], (int)p[1]));
    else if (cmd == "bits") printf("%d\n", big_bits(v[0]));
    else if (cmd == "trim") line(big_trimmed(v[0]));
    else { fprintf(stderr, "unknown query: %s\n", text.c_str()); return 2; }
  }
  return 0;
}
"""


def words(x, n):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & MASK for i in range(n)]


def ones(n):
    return (1 << (32 * n)) - 1


def full(rng, n):
    """A random number that fills n words: its top bit is set."""
    return rng.getrandbits(32 * n) | 1 << (32 * n - 1)


class Queries:
    """The queries of one group with the answer Python expects for each."""

    def __init__(self):
        self.lines, self.want = [], []

    def ask(self, want, cmd, params, *operands):
        """want: one list of words per `;`-separated part of the answer"""
        self.lines.append(" ".join([cmd] + [str(int(p)) for p in params] + [t for op in operands for t in [";"] + [str(w) for w in op]]))
        self.want.append([[int(w) for w in part] for part in want])


# ---- the queries, group by group ---------------------------------------------------------------------------------------------------
def mul_queries(q):
    rng = random.Random(1)
    for aw in (1, 2, 5):
        for bw in (1, 2, 5):
            for a in (ones(aw), full(rng, aw), 1, 0):
                for b in (ones(bw), full(rng, bw), 1):
                    q.ask([words(a * b, aw + bw)], "mul", [], words(a, aw), words(b, bw))
    return 3 * 3 * 4 * 3


def divmod_queries(q):
    rng = random.Random(2)
    shorter = 0
    for mw in (1, 2, 5):
        for m in (full(rng, mw), ones(mw), 1 << (32 * mw - 1), 3):
            for xw in (1, 2, 5, 6):
                limit = 1 << (32 * xw)
                k = rng.getrandbits(32) | 1
                # below the divisor, the divisor itself, two multiples of it, one more than a multiple, every bit set
                xs = [x for x in (m - 1, m, 3 * m, k * m, k * m + 1) if x < limit] + [ones(xw)]
                for x in xs:
                    shorter += mw < xw
                    q.ask([words(x // m, xw), words(x % m, mw)], "divmod", [], words(x, xw), words(m, mw))
        # a divisor with an empty top word
        q.ask([words(ones(mw) // 5, mw), words(ones(mw) % 5, mw + 1)], "divmod", [], words(ones(mw), mw), words(5, mw + 1))
    assert shorter > 50
    return len(q.lines)


def shl_queries(q):
    rng = random.Random(3)
    for nw in (1, 2, 5):
        for n in (full(rng, nw) | 1, ones(nw), rng.getrandbits(32 * nw - 2) | 1 << (32 * nw - 3) | 1):
            below = [1, n - 1, rng.randrange(n), 1 << (32 * nw - 1) if 1 << (32 * nw - 1) < n else n >> 1]
            # at and above the modulus, as far as nw words hold it
            above = [x for x in (n, n + 1, 2 * n + 1, 3 * n - 1, ones(nw)) if x < 1 << (32 * nw)]
            assert len(above) >= 2
            for x in below + above:
                for k in (0, 1, 31, 32, 33, 32 * nw + 5):
                    q.ask([words((x << k) % n, nw)], "shl", [k], words(x, nw), words(n, nw))
        # the modulus under an empty top word (what sc_const_create passes for a short constant)
        n = full(rng, nw) | 1
        q.ask([words((n + 2 << 29) % n, nw + 1)], "shl", [29], words(n + 2, nw + 1), words(n, nw + 1))
    return len(q.lines)


def pow_queries(q):
    rng = random.Random(4)
    for mw in (1, 2, 3):
        for m in (full(rng, mw) | 1, ones(mw), 1 << (32 * mw - 1), 1):
            for base in (0, 1, m - 1, m, m + 1 if m + 1 < 1 << (32 * mw) else 2, rng.getrandbits(32 * mw)):
                for e, ew in ((0, 1), (0, 2), (1, 1), (1, 2), (rng.getrandbits(32) | 1 << 31, 2), (2, 1), (65537, 1), (full(rng, 2), 2), (full(rng, 2), 3)):
                    q.ask([words(pow(base, e, m), mw)], "pow", [], words(base, mw), words(e, ew), words(m, mw))
    # a base wider than the modulus
    q.ask([words(pow(ones(3), 5, 7), 1)], "pow", [], words(ones(3), 3), [5], [7])
    return len(q.lines)


def inv_queries(q):
    rng = random.Random(5)
    for mw in (1, 3):
        for m in (full(rng, mw) | 1, ones(mw), 3 if mw == 1 else (1 << 64) + 1):
            units = [1, m - 1]
            while len(units) < 5:
                a = rng.randrange(1, m)
                if _coprime(a, m):
                    units.append(a)
            for a in units:
                inv = pow(a, -1, m)
                assert a * inv % m == 1
                q.ask([words(inv, mw)], "inv", [], words(a, mw), words(m, mw))
    # no inverse: a factor in common, and zero
    for a, m in ((3, 15), (0, 15), (15, 15), (5 * 7, 5 * ((1 << 70) + 1))):
        mw = (m.bit_length() + 31) // 32
        q.ask([[]], "inv", [], words(a, mw), words(m, mw))
    # an operand wider than the modulus is reduced first
    q.ask([words(pow(ones(2), -1, 0xfffffffb), 1)], "inv", [], words(ones(2), 2), [0xfffffffb])
    return len(q.lines)


def _coprime(a, b):
    while b:
        a, b = b, a % b
    return a == 1


def limb_queries(q):
    rng = random.Random(6)
    straddles = 0
    for W in (28, 29):
        for nw in (1, 2, 3, 5, 33):
            end = 32 * nw
            if end % W == 0:
                continue
            S = end // W + 2                  # limb S - 2 straddles the end of the last word, limb S - 1 lies wholly beyond it
            assert W * (S - 2) < end < W * (S - 1)
            straddles += 1
            for x in (ones(nw), full(rng, nw), 1 << (end - 1), 1):
                for s in (S, S - 1, 1):
                    q.ask([[(x >> (W * i)) & ((1 << W) - 1) for i in range(s)]], "limbs", [s, W], words(x, nw))
    assert straddles >= 8
    # the shapes the library asks for: a 1024-bit number in the (2, 18, 29) configuration, a 2048-bit one in (1, 37, 28)'s twice
    for nw, S, W in ((32, 36, 29), (64, 74, 28)):
        x = full(rng, nw)
        q.ask([[(x >> (W * i)) & ((1 << W) - 1) for i in range(S)]], "limbs", [S, W], words(x, nw))
    return len(q.lines)


def small_queries(q):
    for x, n in ((0, 1), (0, 3), (1, 1), (1 << 31, 1), (1 << 32, 2), (ones(5), 5), (5, 3)):
        q.ask([[x.bit_length()]], "bits", [], words(x, n))
        q.ask([words(x, max(1, (x.bit_length() + 31) // 32))], "trim", [], words(x, n))
    return len(q.lines)


GROUPS = {"mul": mul_queries, "divmod": divmod_queries, "shl": shl_queries, "pow": pow_queries, "inv": inv_queries, "limbs": limb_queries,
          "small": small_queries}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every group's (query, answer, expected answer) rows, from one run of the program."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    d = tmp_path_factory.mktemp("bigint")
    src, exe = d / "bigint.cpp", d / "bigint"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    groups = {}
    for name, fill in GROUPS.items():
        groups[name] = Queries()
        assert fill(groups[name]) == len(groups[name].lines) > 0
    lines = [ln for q in groups.values() for ln in q.lines]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    rows, at = {}, 0
    for name, q in groups.items():
        got = [[[int(t) for t in part.split()] for part in ln.split(";")] for ln in out[at:at + len(q.lines)]]
        rows[name] = list(zip(q.lines, got, q.want))
        at += len(q.lines)
    return rows


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_helpers_against_python_integers(answers, group):
    for query, got, want in answers[group]:
        assert got == want, query


def test_host_sources_keep_their_shape():
    names = sorted(os.listdir(CSRC))
    text = {n: open(os.path.join(CSRC, n)).read() for n in names if n.endswith((".h", ".hip"))}
    big = text["sc_bigint.h"]
    assert "hip" not in big.replace("HIP-free", "") and "sc_ctx" not in big and "namespace sc_host {" in big
    assert [ln for ln in big.splitlines() if ln.startswith("#include")] == ["#include <cstddef>", "#include <cstdint>", "#include <vector>"]
    for n, t in text.items():
        if n.endswith(".h"):
            assert not re.search(r"namespace\s*\{", t), n                        # an unnamed namespace in a header: a type per unit
        assert not re.search(r'#\s*include\s+"[^"]*\.hip"', t), n               # no unit is stitched into another
        for gone in ("sc_families.h", "sc_schemes.h", "sc_topk.h"):
            assert not re.search(r'#\s*include\s+"%s"' % re.escape(gone), t), (n, gone)
            assert gone not in names
    for n in names:                                                              # the kernel units never see the host's integers
        if n.startswith("sc_launch_"):
            assert "sc_bigint.h" not in text[n] and "sc_host.h" not in text[n], n
    assert '#include "sc_bigint.h"' in text["sc_host.h"] and "sc_bigint.h" not in "".join(ln for ln in text["sc_internal.h"].splitlines() if ln.startswith("#include"))

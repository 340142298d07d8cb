"""Secure division without a GPU: the digit loop of csrc/div/sc_divmod_words.h -- the very code k_divmod_words runs --
compiled into a stand-alone host program (AddressSanitizer and UBSan where the compiler has them) and run over the edge table and 10^4
random rows against Python's divmod, branch tallies included; every branch of the loop taken by a table row; the fit rule one bit either
side, the C copy equal to the Python copy; the whole protocol, both players, on the stand-in engine with the golden 1024-bit key; the
refusals; the ledger of the kernels under csrc/div/."""
import asyncio
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, oracle_dgk, oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _div_model as model  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402

CSRC = os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc")
DIV = os.path.join(CSRC, "div")

PROGRAM = r"""
#include "sc_divmod_words.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// a line "nw d x_0 .. x_{nw-1}" -> "q_0 .. q_{nw-1} rem saturated first second", divided apart and then in place (both must agree);
// the rows are heap arrays of exactly nw words, so a read or write past a row is the sanitizer's
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int nw; unsigned long long d;
    in >> nw >> d;
    std::vector<uint32_t> x(nw), q(nw, 0xdeadbeefu), y(nw);
    for (int i = 0; i < nw; i++) { unsigned long long v; in >> v; x[i] = y[i] = (uint32_t)v; }
    uint32_t tally[sc::DIV_BRANCHES] = {0, 0, 0};
    const uint64_t rem = sc::divmod_row(x.data(), nw, d, q.data(), tally);
    const uint64_t rem2 = sc::divmod_row(y.data(), nw, d, y.data(), nullptr);
    if (rem2 != rem || y != q) { printf("in-place mismatch\n"); continue; }
    for (int i = 0; i < nw; i++) printf("%u ", q[i]);
    printf("%llu %u %u %u\n", (unsigned long long)rem, tally[0], tally[1], tally[2]);
  }
  return 0;
}
"""


def _words(x, n):
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    d = tmp_path_factory.mktemp("divmod")
    src, out = d / "divmod.cpp", d / "divmod"
    src.write_text(PROGRAM)
    base = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", DIV, str(src), "-o", str(out)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:                                          # a compiler without the sanitizers' runtimes: a plain build
        subprocess.run(base, check=True)
    return str(out)


def _run(exe, rows):
    text = "\n".join(" ".join(str(v) for v in [nw, d] + _words(x, nw)) for x, nw, d in rows) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    for (x, nw, d), line in zip(rows, out):
        got = [int(t) for t in line.split()]
        q, r, tally = model.digit_loop(x, nw, d)
        assert (q, r) == divmod(x, d)
        assert got == _words(q, nw) + [r] + tally, (hex(x), nw, hex(d))


def test_header_is_plain_cxx_without_the_gpu_runtime():
    text = open(os.path.join(DIV, "sc_divmod_words.h")).read()
    assert "hip_runtime" not in text and "__global__" not in text and "asm" not in text
    assert [ln for ln in text.splitlines() if ln.startswith("#include")] == ["#include <stdint.h>"]
    assert '#include "sc_divmod_words.h"' in open(os.path.join(DIV, "sc_kernel_divmod.h")).read()
    assert '#include "div/sc_kernel_divmod.h"' in open(os.path.join(CSRC, "sc_launch_misc.hip")).read()


def test_digit_loop_edge_table(exe):
    rows = model.edge_rows()
    assert {nw for _, nw, _ in rows} >= set(model.NWS) and {d for _, _, d in rows} >= set(model.DIVISORS)
    _run(exe, rows)


def test_digit_loop_random_rows(exe):
    _run(exe, model.random_rows(10000, 20261))


def test_every_branch_is_taken_by_a_table_row():
    taken = [0, 0, 0]
    for x, nw, d in model.edge_rows():
        for i, t in enumerate(model.digit_loop(x, nw, d)[2]):
            taken[i] += t > 0
    for name, rows in zip(model.BRANCHES, taken):
        assert rows >= 1, f"no table row takes the branch: {name}"


def test_restated_loop_is_exact_for_every_row_of_small_digits():
    """Digits of 3 bits: every divisor below 2^6 against every dividend of up to three digits -- the estimate never needs a third
    correction (the loop's own assertion R < v), every branch occurs, and one path serves one- and two-digit divisors alike."""
    seen = [0, 0, 0]
    for nw in (1, 2, 3):
        for d in range(1, 64):
            for x in range(1 << (3 * nw)):
                q, r, tally = model.digit_loop(x, nw, d, 3)
                assert (q, r) == divmod(x, d)
                seen = [a + b for a, b in zip(seen, tally)]
    assert all(seen)


# ---- the fit rule ------------------------------------------------------------------------------------------------------------------------
def test_fit_rule_one_bit_either_side_and_the_c_copy():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.division import div_fits, div_width

    c_fits = _lib.load().sc_div_fits
    for nbits in (512, 1024, 1025, 2048, 3072):
        for kappa in (1, 40, 62):
            edge = nbits - 1 - kappa - 2 - 1                                   # the widest dividend that fits
            for signed in (False, True):
                for x_bits in (1, 8, 62, 63, 64, edge - 3, edge - 2, edge - 1, edge, edge + 1, edge + 2):
                    want = div_width(x_bits, signed) + kappa + 2 < nbits - 1
                    assert div_fits(nbits, kappa, x_bits, signed) is want == bool(c_fits(nbits, kappa, x_bits, int(signed))), (nbits, kappa, x_bits, signed)
            assert div_fits(nbits, kappa, edge, False) and not div_fits(nbits, kappa, edge + 1, False)
            assert div_fits(nbits, kappa, edge - 2, True) and not div_fits(nbits, kappa, edge - 1, True)
    for bad in ((1024, 0, 8), (1024, 63, 8), (1024, 40, 0)):
        assert not div_fits(*bad) and not c_fits(*bad, 0)
    assert div_width(8, True) == 65 and div_width(100, True) == 102 and div_width(100, False) == 100


# ---- the protocol on the stand-in engine -------------------------------------------------------------------------------------------------
class Engine(model.DivisionEntries, OracleEngine):
    pass


@pytest.fixture(scope="module")
def world(keys):
    from protocols.secure_comparison_amd import DGK, Paillier

    sk, dk = oracle_paillier(keys, 1024), oracle_dgk(keys, "dgk_2048_l64")
    eng = Engine()
    eng.rng_seed(b"\x07" * 32)
    bp = Paillier(sk.n, sk.p, sk.q, engine=eng)
    bd = DGK(dk.n, dk.g, dk.h, dk.u, dk.t, dk.p, dk.q, dk.v_p, dk.v_q, engine=eng, randomizer_bits=50)
    return sk, dk, eng, bp.public_copy(), bd.public_copy(), bp, bd


def _enc(sk, eng, values, rng):
    n, n2 = sk.n, sk.n * sk.n
    return eng.upload([(1 + (v % n) * n) * pow(rng.randrange(1, n), n, n2) % n2 for v in values], 2 * ((n.bit_length() + 31) // 32))


def _dec(sk, eng, t, signed=True):
    n = sk.n
    out = [sk.dec_raw(v) for v in eng.download(t)]
    return [v - n if signed and v > n // 2 else v for v in out]


def planted(divs, x_bits, rbits, signed, rng):
    """(xs, rs) per row of divs: zm < rm, zm == rm, zm > rm in turn (zm = (x' + r) mod d, rm = r mod d, x' the dividend after the signed
    offset), then the dividends 0, d - 1, d, 2^x_bits - 1 and for signed input -1, -d, -d - 1, -2^x_bits under random r."""
    xs, rs = [], []
    top = (1 << x_bits) - 1
    extra = [0, None, None, top] + ([-1, None, None, -(1 << x_bits)] if signed else [])
    for i, d in enumerate(divs):
        r = rng.getrandbits(rbits)
        kind = i % (3 + len(extra))
        if kind < 3:
            r = min(r | (1 << 70), (1 << rbits) - 1) if rbits > 70 else r
            r -= r % d
            x = rng.getrandbits(x_bits)
            c = -(-(1 << x_bits) // d) if signed else 0
            off = (c * d) % d                                                                  # 0: the offset is a multiple of d
            assert off == 0
            want = (1 % d, 0, 1 % d)[kind]                                                     # x mod d
            x = max(0, x - x % d) + want if x - x % d + want <= top else want
            r += (d - 1, 0, 0)[kind]
            if r >> rbits:
                r -= d * (-(-(r - (1 << rbits) + 1) // d))
        else:
            x = extra[kind - 3]
            if x is None:
                x = (d - 1, d)[kind - 4] if kind in (4, 5) else (-d, -d - 1)[kind - 8]
            if not -(1 << x_bits) * signed <= x <= top:
                x = top
        xs.append(x)
        rs.append(r)
    return xs, rs


def _draws(world, layout, count, rs):
    from protocols.secure_comparison_amd.division import draw_div

    sk, dk, eng, ap, ad, bp, bd = world
    draws = draw_div(count, layout, ap, ad)
    draws.r = eng.upload(rs, ap.mod_n.nwords)
    return draws


CASES = [(1, 8), (2, 8), (3, 32), (10, 32), (1000, 200), (1 << 16, 32), ((1 << 32) + 1, 200), ("mixed", 64)]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("divisor,x_bits", CASES)
def test_whole_division_on_the_stand_in_engine(world, divisor, x_bits, signed):
    from protocols.secure_comparison_amd.division import DivLayout, div_batch, mod_from_quotient

    sk, dk, eng, ap, ad, bp, bd = world
    rng = random.Random(hash((str(divisor), x_bits, signed)) & 0xffff)
    B = 11 if signed else 7
    divs = [1, 2, 3, 10, 1000, 1 << 16, (1 << 32) + 1, 7, (1 << 20) - 1, 5, 1 << 31][:B] if divisor == "mixed" else [divisor] * B
    layout = DivLayout(40, x_bits, signed, sk.n.bit_length(), tuple(divs), dk.u)
    assert layout.l == max(1, (max(divs) - 1).bit_length())
    xs, rs = planted(divs, x_bits, layout.rbits, signed, rng)
    draws = _draws(world, layout, B, rs)
    x_enc = _enc(sk, eng, xs, rng)
    q_enc = div_batch(layout, x_enc, ap, bp, ad, bd, draws)
    assert _dec(sk, eng, q_enc) == [x // d for x, d in zip(xs, divs)], (xs, divs)
    assert _dec(sk, eng, mod_from_quotient(layout, x_enc, q_enc, ap)) == [x % d for x, d in zip(xs, divs)]
    # the three planted relations all occur (d = 1 has zm == rm == 0 alone)
    offs = [c * d for c, d in zip(layout.c, divs)]
    rel = {((x + o + r) % d > r % d) - ((x + o + r) % d < r % d) for x, o, r, d in zip(xs, offs, rs, divs)}
    assert rel == ({0} if max(divs) == 1 else {-1, 0, 1})


def test_planted_sub_comparison_equals_the_oracle_steps(world):
    """What div_blind and div_open plant -- alpha = alpha~ = rm, r_small = 1, r_shift = rq; beta = zm, the bit d = 1, zeta_1 = zeta_2 = zq --
    taken from the stand-in run itself and put through the library's steps 4a-4j with injected draws: the [c_i] of step 4h and delta_B
    equal what oracle/sc_oracle.py's steps give for the same plaintexts and draws, row by row, and delta_B decides [zm < rm]."""
    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import Initiator, KeyHolder
    from protocols.secure_comparison_amd.division import DivLayout, div_blind, div_open

    sk, dk, eng, ap, ad, bp, bd = world
    rng = random.Random(5)
    divs = [1000, 1000, 1000, 7, 1, 1000, 999]
    xs, rs = [2001, 3000, 3001, 20, 5, 999, 0], [5999, 123000, 123000, 6, 77, 0, 998]          # zm < rm, ==, >, <, d = 1, >, <
    B = len(divs)
    layout = DivLayout(40, 12, False, sk.n.bit_length(), tuple(divs), dk.u)
    l = layout.l
    draws = _draws(world, layout, B, rs)
    z_enc, a_plain = div_blind(layout, _enc(sk, eng, xs, rng), draws, ap)
    b_plain = div_open(layout, z_enc, bp)
    want = [(divmod(x + r, d), divmod(r, d)) for x, r, d in zip(xs, rs, divs)]
    assert [v & model.MASK64 for v in a_plain.alpha.tolist()] == [w[1][1] for w in want] and a_plain.alpha_tilde is a_plain.alpha
    assert eng.download(a_plain.r_shift) == [w[1][0] for w in want] and a_plain.r_small.tolist() == [1] * B
    assert [v & model.MASK64 for v in b_plain.beta.tolist()] == [w[0][1] for w in want] and b_plain.d.tolist() == [1] * B
    assert eng.download(b_plain.zeta_1) == [w[0][0] for w in want] and b_plain.zeta_2 is b_plain.zeta_1
    d_enc, beta_enc = KeyHolder.step_4a_4b_batch(b_plain, l, bd, bp, None)
    c_sent, c_h = Initiator.step_4_batch(d_enc, beta_enc, a_plain, draws.delta_a, ad, draws.rhos, draws.permutation, None, want_unblinded=True)
    delta_b = KeyHolder.step_4j_5_batch(c_sent, b_plain, bp, bd, None)[0].tolist()
    rhos, perm = [eng.download(draws.rhos[:, b].contiguous()) for b in range(B)], draws.permutation.tolist()
    for b, ((zq, zm), (rq, rm)) in enumerate(want):
        delta_a = int(draws.delta_a[b])
        alpha = o.to_bits(rm, l)
        d0 = o.step_4c(o.step_4a(0, dk, sk, l), 0, dk, sk)                      # z = r = 0 stand for "below (N - 1) / 2": the planted bits
        beta = o.step_4b(zm, l, dk)
        w = o.step_4f(o.step_4d(alpha, beta, dk), dk)                           # alpha~ == alpha: step 4e changes nothing
        c = o.step_4h(1 - 2 * delta_a, alpha, alpha, d0, beta, w, delta_a, dk)
        assert eng.download(c_h[:, b].contiguous()) == c, b
        assert eng.download(c_sent[:, b].contiguous()) == o.step_4i(c, dk, rhos[b], perm[b]), b
        assert delta_b[b] == o.step_4j(c, dk)
        lt = delta_b[b] if delta_a == 1 else 1 - delta_b[b]
        assert lt == int(zm < rm) and zq - rq - lt == xs[b] // divs[b], b


def test_two_players_on_the_stand_in_engine(world):
    from protocols.secure_comparison_amd import InMemoryCommunicator, Initiator, KeyHolder

    sk, dk, eng, ap, ad, bp, bd = world
    rng = random.Random(9)
    divs = [7, 1000, 3, 1 << 16, 10]
    xs = [-50, 999, -3, (1 << 20) - 1, 0]
    comm = InMemoryCommunicator(device_tensors=True, timeout_s=60.0)
    alice = Initiator(16, communicator=comm, other_party="keyholder")
    bob = KeyHolder(16, communicator=comm.peer(), other_party="initiator", scheme_paillier=bp, scheme_dgk=bd)
    x_enc = _enc(sk, eng, xs, rng)

    async def run(theirs):
        return await asyncio.gather(alice.perform_secure_modulo_batch(x_enc, divs, 20, signed=True, engine=eng, with_quotient=True),
                                    bob.perform_secure_divide_batch(len(xs), divs, **theirs))

    (q_enc, m_enc), _ = asyncio.run(run(dict(x_bits=20, signed=True)))
    assert _dec(sk, eng, q_enc) == [x // d for x, d in zip(xs, divs)] and _dec(sk, eng, m_enc) == [x % d for x, d in zip(xs, divs)]
    with pytest.raises(ValueError, match="announces"):
        asyncio.run(run(dict(x_bits=21, signed=True)))


def test_refusals_before_anything_is_sent(world, keys):
    from protocols.secure_comparison_amd import DGK, secure_divide_batch, secure_shift_right_batch
    from protocols.secure_comparison_amd.division import divisors_of

    sk, dk, eng, ap, ad, bp, bd = world
    x_enc = _enc(sk, eng, [1, 2, 3], random.Random(1))
    calls = []
    eng.initiator_div_blind, keep = (lambda *a, **k: calls.append(a)), eng.initiator_div_blind
    try:
        for divisor, msg in ((0, "expected 1 <= d"), (1 << 64, "expected 1 <= d"), ([1, 2], "2 divisors for 3 rows"), ([3, 0, 3], "row 1"),
                             (torch.tensor([1.0, 2.0, 3.0]), "int64"), (torch.tensor([1, -2, 3]), "row 1")):
            with pytest.raises(ValueError, match=msg):
                secure_divide_batch(x_enc, divisor, 8, ap, bp, ad, bd)
        with pytest.raises(ValueError, match="does not fit"):
            secure_divide_batch(x_enc, 3, 1024 - 1 - 40 - 2, ap, bp, ad, bd)
        with pytest.raises(ValueError, match="kappa"):
            secure_divide_batch(x_enc, 3, 8, ap, bp, ad, bd, kappa=63)
        small = oracle_dgk(keys, "dgk_1024_l16")                          # u just above 2^18: divisors of up to 16 bits
        sd = DGK(small.n, small.g, small.h, small.u, small.t, engine=eng, randomizer_bits=50)
        with pytest.raises(ValueError, match="DGK key with u"):
            secure_divide_batch(x_enc, (1 << 16) + 1, 8, ap, bp, sd, sd)
        with pytest.raises(ValueError, match="0 <= t <= 63"):
            secure_shift_right_batch(x_enc, 64, 8, ap, bp, ad, bd)
    finally:
        eng.initiator_div_blind = keep
    assert not calls
    assert divisors_of(torch.tensor([5, 6], dtype=torch.int64), 2) == (5, 6) and divisors_of(9, 3) == (9, 9, 9)


def test_shift_right_and_groupby_mean_signature(world):
    from protocols.secure_comparison_amd import secure_shift_right_batch

    sk, dk, eng, ap, ad, bp, bd = world
    xs = [-1, -8, 7, 8, 1023, -1024]
    x_enc = _enc(sk, eng, xs, random.Random(2))
    assert _dec(sk, eng, secure_shift_right_batch(x_enc, 3, 10, ap, bp, ad, bd, signed=True)) == [x >> 3 for x in xs]
    assert _dec(sk, eng, secure_shift_right_batch(x_enc, 0, 10, ap, bp, ad, bd, signed=True)) == xs


# ---- ledgers -----------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_under_div_has_an_owner():
    files = sorted(os.listdir(DIV))
    assert files == sorted(model.DIV_HEADERS), "csrc/div/ holds the digit loop and the kernel's file, nothing else"
    found = {}
    for f in files:
        text = open(os.path.join(DIV, f)).read()
        names = re.findall(r"__global__\s+void\b.*?\b(k_\w+)\s*\(", text, re.S)
        assert len(names) == len(re.findall(r"__global__", text))
        found.update({k: "div/" + f for k in names})
    assert found == {k: v[0] for k, v in model.KERNELS.items()}
    for kernel, (_, owner) in model.KERNELS.items():
        path, test = owner.split("::")
        assert re.search(rf"^def {test}\(", open(os.path.join(ROOT, path)).read(), re.M), owner
    # the launch is written in the subdirectory, once, and the misc unit is the one unit that compiles it
    launches = re.findall(r"hipLaunchKernelGGL\(\s*(?:sc::)?(\w+)", open(os.path.join(DIV, "sc_kernel_divmod.h")).read())
    assert launches == ["k_divmod_words"]
    users = [f for f in os.listdir(CSRC) if f.endswith((".h", ".hip")) and '#include "div/sc_kernel_divmod.h"' in open(os.path.join(CSRC, f)).read()]
    assert users == ["sc_launch_misc.hip"]


def test_symbols_units_and_exports():
    import protocols.secure_comparison_amd as pkg
    from protocols.secure_comparison_amd import _lib, build

    for name in ("sc_plain_divmod", "sc_div_fits", "sc_initiator_div_blind", "sc_keyholder_div_open"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 5 and len(build.ALL_UNITS) == 17 and len(build.UNITS) == 13
    assert not [u for u in build.ALL_UNITS if "div" in u[1]]
    assert any(d.endswith(os.path.join("div", "sc_divmod_words.h")) for d in build.DEPS)              # a change there rebuilds the library
    assert os.path.join(DIV, "sc_divmod_words.h") in {os.path.normpath(p) for p in build._closure(os.path.join(CSRC, "sc_launch_misc.hip"))}
    for name in ("DivLayout", "DivDraws", "draw_div", "secure_divide_batch", "secure_modulo_batch", "secure_divmod_batch",
                 "secure_shift_right_batch", "secure_groupby_mean_batch"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for cls in (pkg.Initiator, pkg.KeyHolder):
        assert hasattr(cls, "perform_secure_divide_batch") and hasattr(cls, "perform_secure_modulo_batch")
    from protocols.secure_comparison_amd.engine import Engine as Real

    assert hasattr(Real, "plain_divmod")

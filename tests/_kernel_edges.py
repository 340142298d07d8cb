"""The kernels outside the interpreter as data: deterministic rows at the edges of the division-step inversion kernel (k_xgcd, four
WPL instances), the plain-word kernels (k_plain_alice / k_plain_bob, four flag-word counts each) and the selection kernels
(k_select_prep / k_select_split), with plain-integer references for every output.

Pure Python (no torch at import, nothing from the package under test): tests/test_kernel_edges_cpu.py checks the table against
the launcher sources and the inversion model on a machine without a GPU; tests/test_gpu_kernel_edges.py runs it.  The references
use Python integers only: pow(x, -1, n), shifts, %.

The edges are the kernels' own, not the interpreter's:
* launch_xgcd picks WPL from need = nw + 2 <= 64 WPL, so the lane layout changes at nw = 62 | 63, 126 | 127 and 254 | 255, and just
  above a multiple of WPL words the top lane holds one word;
* the plain kernels read 64-bit words of an nw-word number (an odd nw ends in half a word), shift by l / 32 words and l % 32 bits,
  and carry a borrow across LW = ceil(l / 64) flag words;
* the selection kernels cut fields at arbitrary bit offsets out of nw words and multiply them by a value of up to 63 bits.
"""
from __future__ import annotations

import functools
import math
import random

import _instance_matrix as M

# ==== inversion ====================================================================================================================
MAX_WORDS = M.size_range(M.K_CONFIGS[-1])[1] // 32          # the widest whole-word modulus sc_mod_create accepts
# WPL -> the first and last nw launch_xgcd sends to the instance, and one size just above a multiple of WPL words
XGCD_WORDS = {1: (2, 3, 61, 62), 2: (63, 64, 65, 125, 126), 4: (127, 128, 129, 253, 254), 8: (255, 256, 257, MAX_WORDS)}
XGCD_SHAPES = ("allones", "top-plus-one", "top-word-one", "alternating", "one-mod-2^30", "minus-one-mod-2^30", "rand")
RANDOM_FILL = 6


def wpl_for(nw: int) -> int:
    """launch_xgcd, restated: need = nw + 2 words (|d| < 2^11 n and the sign) on 64 lanes of WPL words."""
    need = nw + 2
    for wpl in (1, 2, 4, 8):
        if need <= 64 * wpl:
            return wpl
    raise ValueError(f"{nw} words: no instance")


def xgcd_modulus(nw: int, shape: str) -> int:
    """An odd modulus of exactly nw words; every shape but top-word-one has its top bit on the last bit of the top word."""
    bits = 32 * nw
    rng = random.Random(f"kernel-edges:xgcd:{nw}:{shape}")
    top = 1 << (bits - 1)
    if shape == "allones":
        return M.make_modulus(bits, "allones")
    if shape == "top-plus-one":
        return top | 1
    if shape == "top-word-one":                       # 32 (nw - 1) + 1 bits: the guard's slowest case, a nearly empty top word
        return M.make_modulus(bits - 31, "rand")
    if shape == "alternating":
        return int("a" * (bits // 4), 16) | 1          # 1010 ... 1011
    if shape == "one-mod-2^30":
        return ((rng.getrandbits(bits) | top) >> 30 << 30) | 1
    if shape == "minus-one-mod-2^30":
        return rng.getrandbits(bits) | top | ((1 << 30) - 1)
    assert shape == "rand"
    return M.make_modulus(bits, "rand")


def adversarial_operands(n: int, bits: int, rng) -> tuple:
    """Operands that keep the division steps adding or exchanging for long stretches (one draw from rng)."""
    return (1, 2, n - 1, n - 2, (n + 1) // 2, n >> 1, (1 << (bits - 2)) - 1, int("5" * (bits // 4 - 1), 16) % n, rng.randrange(1, n))


def adversarial_pairs(bits, rng):
    """(n, x) over all-ones / single-bit / alternating / random moduli of `bits` bits (tests/test_xgcd_model_cpu.py)."""
    n_all_ones = (1 << bits) - 1
    while n_all_ones % 3 == 0 or n_all_ones % 5 == 0:
        n_all_ones -= 2
    alt = int("a" * (bits // 4), 16) | 1                      # 1010...1011
    ns = [n_all_ones, (1 << (bits - 1)) | 1, alt | (1 << (bits - 1)), rng.getrandbits(bits) | (1 << (bits - 1)) | 1]
    for n in ns:
        for x in adversarial_operands(n, bits, rng):
            yield n, x % n


def xgcd_candidates(n: int, nw: int) -> dict:
    """Named operand groups for one modulus, before the coprimality filter."""
    wpl, bits, nbits = wpl_for(nw), 32 * nw, n.bit_length()
    rng = random.Random(f"kernel-edges:xgcd-ops:{nw}:{n & 0xffffffff}:{nbits}")
    r = rng.getrandbits(max(1, nbits - 61)) | 1
    while math.gcd(r, n) != 1:                      # (the shifted operands must survive the coprimality filter)
        r += 2
    return {
        "adversarial": list(adversarial_operands(n, bits, rng)),
        "powers": [1 << 30, 1 << 31, 1 << 32, 1 << (32 * wpl), (1 << (32 * wpl)) - 1, 1 << (bits - 2)],
        "low-zeros": [r << 30, r << 60],                                   # 30 and 60 low zero bits: whole rounds of pure halving
        "n-minus-2^k": [n - (1 << k) for k in (1, 29, 30, 32 * wpl)],
        "random": [rng.randrange(1, n) for _ in range(RANDOM_FILL)],
    }


@functools.lru_cache(maxsize=None)
def xgcd_operands(n: int, nw: int, fill: int = RANDOM_FILL) -> tuple:
    """The invertible operands of one modulus: every candidate reduced modulo n, coprime to n, once."""
    groups = xgcd_candidates(n, nw)
    groups["random"] = groups["random"][:fill]
    out = []
    for vals in groups.values():
        for v in vals:
            v %= n
            if v and math.gcd(v, n) == 1:
                out.append(v)
    return tuple(dict.fromkeys(out))


def xgcd_rows(wpl: int):
    """(nw, shape, n) for every modulus of the instance."""
    for nw in XGCD_WORDS[wpl]:
        for shape in XGCD_SHAPES:
            yield nw, shape, xgcd_modulus(nw, shape)


def expected_modinv(n, xs):
    return [pow(x, -1, n) for x in xs]


# ---- residues without an inverse: composite moduli with a planted 64-bit factor ----------------------------------------------------
NOT_INVERTIBLE_WORDS = {1: 18, 2: 64, 4: 130, 8: MAX_WORDS}
BAD_BATCH = 9
BAD_PLACES = (0, BAD_BATCH // 2, BAD_BATCH - 1)


def planted_modulus(nw: int):
    """(n, p): n = p c of exactly nw words with p a 64-bit factor."""
    p = M.make_modulus(64, "rand")
    c = M.make_modulus(32 * nw - 64, "rand")
    while math.gcd(p, c) != 1:
        c += 2
    n = p * c
    assert (n.bit_length() + 31) // 32 == nw and n & 1
    return n, p


def not_invertible_operands(n: int, p: int) -> list:
    r = random.Random(f"kernel-edges:bad:{n & 0xffffffff}").randrange(2, n // p)
    return [p, p * r % n, n - p, 0]


def bad_batches(nw: int):
    """(n, rows, index of the first operand without an inverse): each bad operand at the first, a middle and the last place of a
    batch of 9 invertible ones, and one batch that holds two of them."""
    n, p = planted_modulus(nw)
    good = [v for v in xgcd_operands(n, nw) if v > 2][:BAD_BATCH]
    assert len(good) == BAD_BATCH
    out = []
    for k, bad in enumerate(not_invertible_operands(n, p)):
        for place in BAD_PLACES:
            rows = list(good)
            rows[place] = bad
            out.append((n, rows, place))
        rows = list(good)
        rows[2 + k], rows[BAD_BATCH - 2] = bad, p
        out.append((n, rows, 2 + k))
    return out


# ---- the guard: operands that are not reduced ----------------------------------------------------------------------------------------
GUARD_WORDS = {1: 8, 2: 64, 4: 130, 8: MAX_WORDS}
GUARD_SUBTRACTIONS = 3          # k_xgcd subtracts n at most three times


def guard_rows(nw: int):
    """(n, accepted operands x = q n + 1 with q <= 3, the refused x = 5 n + 1) on a modulus whose top word is 1, so that 5 n + 1 still
    fits nw words.  Never a larger quotient: the unbounded guard this replaces took one wave-wide subtraction per multiple of n."""
    n = xgcd_modulus(nw, "top-word-one")
    assert n >> (32 * (nw - 1)) == 1 and (5 * n + 1).bit_length() <= 32 * nw
    return n, [n + 1, 3 * n + 1], 5 * n + 1


def guard_neighbours(n: int) -> list:
    """Three small invertible residues that share a batch with the refused operand."""
    return [v for v in (2, 3, 5, 7, 11, 13, 17) if math.gcd(v, n) == 1][:3]


# ==== plain kernels ===================================================================================================================
PLAIN_WORDS = (2, 3, 8, 32, 33, 64, 96)
PLAIN_L = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 254, 255)
PLAIN_BATCHES = (1, 255, 256, 257)
STEP24B_L = (1, 64, 65, 255)


def plain_moduli(nw: int) -> dict:
    """A modulus with a small top word (two bits of it) and one with its top bit on the word's last bit.  The full one has its two top
    bits set: n > 2/3 2^(32 nw), which is what lets z + n reach word nw for a z below (n - 1) / 2."""
    rng = random.Random(f"kernel-edges:plain:{nw}")
    bits = 32 * nw
    return {"small-top": M.make_modulus(bits - 30, "rand"), "full": rng.getrandbits(bits) | (3 << (bits - 2)) | 1}


def plain_l_values(nw: int) -> list:
    """What sc_plain_alice / sc_plain_bob accept for this word count: 2^l + r must fit nw + 1 words."""
    return [l for l in PLAIN_L if l < 32 * nw]


def lw_of(l: int) -> int:
    return (l + 63) // 64


def edge_rows(n, l, rng):
    """r / z rows at the edges of the flag arithmetic: 0, N - 1, N - 2^l, all-ones low words, a borrow out of the low 64-bit word
    of r - N, both halves of (N-1)/2, and random values."""
    nlo = n & ((1 << 64) - 1)
    rows = [0, 1, n - 1, n - (1 << l), (n - 1) // 2, (n - 1) // 2 - 1, (n + 1) // 2, (1 << l) - 1, (1 << 64) - 1, (1 << 128) - 1,
            ((n >> 300) << 300) | ((1 << 256) - 1), rng.randrange(max(1, n >> 64)) << 64 | (nlo - 1 if nlo else 0), (1 << l) + nlo // 2]
    rows += [rng.randrange(n) for _ in range(19)]
    return [v % n for v in rows]


def _w64(x: int, j: int) -> int:
    return (x >> (64 * j)) & ((1 << 64) - 1)


def borrow_into_equal_word(r: int, n: int, l: int) -> bool:
    """Does the borrow chain of (r - n) mod 2^l meet, below its last flag word, a word where r equals n with a borrow arriving?"""
    borrow = 0
    for j in range(lw_of(l)):
        if borrow and _w64(r, j) == _w64(n, j):
            return True
        borrow = int(_w64(r, j) - borrow < _w64(n, j))
    return False


def equal_word_without_borrow(r: int, n: int, l: int) -> bool:
    """A flag word below the last where r equals n and no borrow arrives (a chain that took `<=` for `<` would invent one)."""
    borrow = 0
    for j in range(lw_of(l) - 1):
        if not borrow and _w64(r, j) == _w64(n, j):
            return True
        borrow = int(_w64(r, j) - borrow < _w64(n, j))
    return False


def named_plain_rows(n: int, nw: int, l: int) -> dict:
    """The rows the issue names, by name (a name is absent where the modulus does not allow the row)."""
    rng = random.Random(f"kernel-edges:plain-rows:{nw}:{l}:{n & 0xffffffff}")
    full, half = 1 << (32 * nw), (n - 1) // 2
    out = {}
    # equal to n in one whole 64-bit word with the word below it smaller; the word above (if any) differs
    for j in range(1, 4):
        if n >> (64 * j) and _w64(n, j - 1):
            v = n - (1 << (64 * (j - 1)))
            if _w64(n, j + 1):
                v -= 1 << (64 * (j + 1))
            out[f"equal-word-{j}-borrow-in"] = v
    if n >> 64:
        out["equal-word-0-no-borrow"] = n - (1 << 64)
    if full - n < half:                                # z below (n - 1) / 2 with z + n >= 2^(32 nw)
        out["sum-is-2^(32nw)"] = full - n
        out["sum-carries-into-word-nw"] = full - n + rng.randrange(1, half - (full - n))
        out["sum-carries-high-bits-set"] = half - 1
    out["half-plus-1"], out["half-minus-1"] = half + 1, half - 1
    q = rng.randrange(1, n >> l) if n >> l > 1 else n >> l
    out["only-at-and-above-l"] = (q << l) if q else 0
    low = (1 << l) - 1
    out["all-below-l"] = ((q << l) | low) if ((q << l) | low) < n else (low if low < n else n - 1)
    assert all(0 <= v < n for v in out.values()), (nw, l)
    return out


@functools.lru_cache(maxsize=None)
def plain_rows(n: int, nw: int, l: int) -> tuple:
    return tuple(edge_rows(n, l, random.Random(f"kernel-edges:edge-rows:{nw}:{l}")) + list(named_plain_rows(n, nw, l).values()))


def expected_plain_alice(n: int, l: int, rows) -> dict:
    return {"m1": [r + (1 << l) for r in rows], "alpha": [r % (1 << l) for r in rows], "alpha_tilde": [(r - n) % (1 << l) for r in rows],
            "rsmall": [int(r < (n - 1) // 2) for r in rows], "rshift": [r >> l for r in rows]}


def expected_plain_bob(n: int, l: int, rows) -> dict:
    d = [int(z < (n - 1) // 2) for z in rows]
    return {"beta": [z % (1 << l) for z in rows], "dbit": d, "zeta1": [z >> l for z in rows],
            "zeta2": [((z + n) >> l) if b else (z >> l) for z, b in zip(rows, d)],
            "bits": [d] + [[(z >> i) & 1 for z in rows] for i in range(l)]}          # the planes of steps 4a / 4b: [l + 1][count]


# ==== selection =======================================================================================================================
SEL_MAX_FIELDS = 4
SEL_BATCHES = (1, 257)
# (bits of the golden Paillier N, kappa, widths)
SEL_LAYOUTS = (
    (1024, 1, (1,)),                        # kappa = 1, one field, everything inside word 0
    (1024, 31, (30,)),                      # kappa = 31: s = 32, the field starts on a word boundary
    (2048, 32, (29, 30, 31, 32)),           # kappa = 32 (r_a fills its one word), SEL_MAX_FIELDS fields, offsets 96 and 160 on word boundaries
    (2048, 62, (1, 64)),                    # kappa = 62 (two words of r_a), a 65-bit field over three words, end = 256
    (1024, 40, (939,)),                     # end = nbits - 2: the last field ends in the top word of N
    (2048, 40, (1000, 921)),
    (3072, 62, (1400, 1479)),
    (3072, 40, (32, 5)),                    # the layout of a secure minimum with its index (a kappa the library's callers use)
)
SEL_CONDITIONS = ("offset on a word boundary", "end on a word boundary", "end in the top word of N", "field over three words",
                  "kappa = 1", "kappa = 31", "kappa = 32", "kappa = 62", "one field", "SEL_MAX_FIELDS fields", "aw = 1", "aw = 2")


def sel_layout(kappa: int, widths, nbits: int):
    """(s, offsets, field bits, end) by the protocol's definition; ValueError where select_layout refuses."""
    if not 1 <= kappa <= 62 or not 1 <= len(widths) <= SEL_MAX_FIELDS:
        raise ValueError("kappa or field count out of range")
    s = kappa + 1
    fbits = [w + kappa + 2 for w in widths]
    offs, off = [], s
    for f in fbits:
        offs.append(off)
        if s + f >= nbits - 1:
            raise ValueError("product does not fit")
        off += f
        if off >= nbits - 1:
            raise ValueError("fields do not fit")
    return s, offs, fbits, off


def sel_aw(kappa: int) -> int:
    return 1 if kappa <= 32 else 2


def sel_conditions(nbits: int, kappa: int, widths) -> set:
    s, offs, fbits, end = sel_layout(kappa, widths, nbits)
    got = set()
    if any(o % 32 == 0 for o in offs):
        got.add("offset on a word boundary")
    if end % 32 == 0:
        got.add("end on a word boundary")
    if end == nbits - 2:
        got.add("end in the top word of N")
    if any(f <= 96 and (o + f - 1) // 32 - o // 32 == 2 for o, f in zip(offs, fbits)):
        got.add("field over three words")
    if kappa in (1, 31, 32, 62):
        got.add(f"kappa = {kappa}")
    if len(widths) == 1:
        got.add("one field")
    if len(widths) == SEL_MAX_FIELDS:
        got.add("SEL_MAX_FIELDS fields")
    got.add(f"aw = {sel_aw(kappa)}")
    return got


def sel_draws(nbits: int, kappa: int, widths) -> list:
    """(r_a, [r_b_j]) rows: r_a in {0, 1, 2^kappa - 1, random} against r_b_j all in {0, 1, 2^(fbits_j - 1) - 1 (the largest draw of
    width + 1 + kappa bits), random}, then mixed random rows."""
    _, _, fbits, _ = sel_layout(kappa, widths, nbits)
    rng = random.Random(f"kernel-edges:sel-draws:{nbits}:{kappa}:{widths}")
    ras = (0, 1, (1 << kappa) - 1, rng.getrandbits(kappa))
    rows = []
    for ra in ras:
        for kind in range(4):
            rows.append((ra, [(0, 1, (1 << (f - 1)) - 1, rng.getrandbits(f - 1))[kind] for f in fbits]))
    rows += [(rng.getrandbits(kappa), [rng.getrandbits(f - 1) for f in fbits]) for _ in range(5)]
    return rows


def sel_pack_fields(kappa: int, widths, nbits: int, a: int, bs) -> int:
    s, offs, fbits, _ = sel_layout(kappa, widths, nbits)
    assert a < 1 << s and all(b < 1 << f for b, f in zip(bs, fbits))
    return a + sum(b << o for b, o in zip(bs, offs))


def sel_p_rows(nbits: int, kappa: int, widths) -> list:
    """P rows below 2^end: every field all ones (highest bit exactly end - 1), all zero, each field alone all ones, random fields."""
    s, offs, fbits, end = sel_layout(kappa, widths, nbits)
    rng = random.Random(f"kernel-edges:sel-p:{nbits}:{kappa}:{widths}")
    sizes = [s] + fbits
    ones = [(1 << f) - 1 for f in sizes]
    fields = [ones, [0] * len(sizes)]
    for i in range(len(sizes)):
        fields.append([ones[k] if k == i else 0 for k in range(len(sizes))])
        fields.append([0 if k == i else ones[k] for k in range(len(sizes))])
    fields += [[rng.getrandbits(f) for f in sizes] for _ in range(6)]
    rows = [sel_pack_fields(kappa, widths, nbits, f[0], f[1:]) for f in fields]
    assert rows[0] == (1 << end) - 1 and all(r >> end == 0 for r in rows)
    return rows


def expected_select_prep(nbits: int, kappa: int, widths, draws, nw: int) -> dict:
    _, offs, _, _ = sel_layout(kappa, widths, nbits)
    mask = (1 << (32 * nw)) - 1
    return {"R": [ra + sum(rb << o for rb, o in zip(rbs, offs)) for ra, rbs in draws],
            "e": [[rbs[j] + (1 << w) for _, rbs in draws] for j, w in enumerate(widths)],
            "rab": [[ra * rbs[j] & mask for ra, rbs in draws] for j in range(len(widths))]}


def expected_select_split(nbits: int, kappa: int, widths, ps, nw: int) -> dict:
    s, offs, fbits, end = sel_layout(kappa, widths, nbits)
    mask = (1 << (32 * nw)) - 1
    return {"prod": [[(p & ((1 << s) - 1)) * ((p >> o) & ((1 << f) - 1)) & mask for p in ps] for o, f in zip(offs, fbits)],
            "fields": [[p & ((1 << s) - 1)] + [(p >> o) & ((1 << f) - 1) for o, f in zip(offs, fbits)] for p in ps],
            "bad": int(any(p >> end for p in ps))}


# ==== coverage: every kernel launched from csrc/sc_launch_misc.hip and launch_xgcd =================================================
COVERED_HERE = {
    **{f"k_xgcd<{w}>": "XGCD_WORDS" for w in XGCD_WORDS},
    **{f"k_plain_alice<{lw}>": "PLAIN_L" for lw in sorted({lw_of(l) for l in PLAIN_L})},
    **{f"k_plain_bob<{lw}>": "PLAIN_L" for lw in sorted({lw_of(l) for l in PLAIN_L})},
    "k_select_prep": "SEL_LAYOUTS", "k_select_split": "SEL_LAYOUTS",
}
_RNG_TEST = "tests/test_gpu_round3.py::test_device_generator_equals_its_restatement"
COVERED_ELSEWHERE = {"k_rng_bits": _RNG_TEST, "k_rng_below": _RNG_TEST, "k_rng_coins": _RNG_TEST, "k_rng_perm": _RNG_TEST,
                     "k_peak_probe": "a multiply-add issue-rate probe: its output is a rate, not a value"}

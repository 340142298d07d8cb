"""The kernels outside the interpreter as data: deterministic rows at the edges of the division-step inversion kernel (k_xgcd, four
WPL instances), the plain-word kernels (k_plain_alice / k_plain_bob, four flag-word counts each), the selection kernels
(k_select_prep / k_select_split) and the plain-word kernels of the multiplication, the inner product and the one-hot encoding
(k_mul_prep / _split, k_dot_prep / _split, k_onehot_prep / _split / _rotate), with plain-integer references for every output.

Pure Python (no torch at import, nothing from the package under test): tests/test_kernel_edges_cpu.py checks the table against
the launcher sources, the inversion model and the families' models on a machine without a GPU; tests/test_gpu_kernel_edges.py and
tests/test_gpu_family_kernel_edges.py run it.  The references
use Python integers only: pow(x, -1, n), shifts, %.

The edges are the kernels' own, not the interpreter's:
* launch_xgcd picks WPL from need = nw + 2 <= 64 WPL, so the lane layout changes at nw = 62 | 63, 126 | 127 and 254 | 255, and just
  above a multiple of WPL words the top lane holds one word;
* the plain kernels read 64-bit words of an nw-word number (an odd nw ends in half a word), shift by l / 32 words and l % 32 bits,
  and carry a borrow across LW = ceil(l / 64) flag words;
* the selection kernels cut fields at arbitrary bit offsets out of nw words and multiply them by a value of up to 63 bits;
* the multiplication, inner-product and one-hot kernels (k_mul_*, k_dot_*, k_onehot_*) hold fields of up to MUL_FIELD_WORDS (one-hot:
  three) words, sum up to DOT_MAX_K products in DOT_ACC_WORDS words, append fields to a bit stream whose pending bits return to zero
  when a field ends on a word boundary, and (one-hot split, rotate) walk a row with 64 lanes, so that a row above 64 words takes a
  second pass.  Their moduli are not keys: the entry points read bits(N) and the word count alone.
"""
from __future__ import annotations

import collections
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


# ==== the three families: what their kernels share ====================================================================================
MUL_MAX_WIDTH = 255
MUL_FIELD_WORDS = 10            # a field or an exponent has at most 255 + 62 + 1 = 318 bits
DOT_MAX_K = 1024
DOT_ACC_WORDS = 2 * MUL_FIELD_WORDS + 1
ONEHOT_MAX_K = 1024
ONEHOT_FIELD_WORDS = 3
BLOCK_BATCHES = (1, 255, 256, 257)          # items per launch of a thread-per-item kernel (a block is 256 threads)
WAVE_ROWS = (1, 3, 4, 5)                    # rows per launch of a wave-per-row kernel (a block is four waves)


def words_of(bits: int) -> int:
    return (bits + 31) // 32


def family_modulus(nbits: int) -> int:
    """Not a key: an odd number of exactly nbits bits.  The entry points read its bit length and its word count."""
    return M.make_modulus(nbits, "rand")


def _ceil_log2(k: int) -> int:
    lg = 0
    while (1 << lg) < k:
        lg += 1
    return lg


def bad_bits(end: int, nw: int) -> dict:
    """Where a planted bit makes a row exceed its layout: at `end` itself, in the last word of the row, on the word boundary above end."""
    out = {"end": end, "last word": 32 * nw - 1}
    if 32 * (end // 32 + 1) < 32 * nw:
        out["word boundary above end"] = 32 * (end // 32 + 1)
    assert all(end <= b < 32 * nw for b in out.values())
    return out


def plant(rows, m: int, i: int, bit: int) -> list:
    """rows [M][count] with one more bit in message m of row i."""
    assert not rows[m][i] >> bit & 1
    out = [list(r) for r in rows]
    out[m][i] |= 1 << bit
    return out


def first_over(rows, ends):
    """(row, message, bit) of the first bit at or above its message's end in rows [M][count], or None: what a wrong verdict is reported with."""
    for i in range(len(rows[0])):
        for m, end in enumerate(ends):
            over = rows[m][i] >> end
            if over:
                return i, m, end + (over & -over).bit_length() - 1
    return None


# ==== multiplication ==================================================================================================================
# sc_launch_mul.hip: A in bits [0, s), s = wx + kappa + 1, then field j of fbits[j] = wy[j] + kappa + 1 bits at off[j], off[0] = s,
# off[j + 1] = off[j] + fbits[j]; every s + fbits[j] and the end of the last field stay below bits(N) - 1.
MulCase = collections.namedtuple("MulCase", "nbits kappa wx wy signed aw bw ew")
MUL_LAYOUTS = (
    MulCase(96, 1, 1, (1,), False, 1, 1, 1),                      # 0: the smallest, s = fbits = 3: the batches around one block
    MulCase(638, 62, 255, (255,), False, 10, 10, 10),             # 1: s = fbits = 318, one field, end = 636 = bits(N) - 2
    MulCase(3072, 62, 255, (255,) * 4, True, 10, 10, 10),         # 2: SEL_MAX_FIELDS fields of 318 bits on 96 words
    MulCase(1050, 1, 30, (29, 31, 30), False, 1, 1, 2),           # 3: s = 32, offsets 32 | 63 | 96, end = 128, 33 words
    MulCase(224, 62, 64, (32,), True, 4, 3, 4),                   # 4: end = 222 = bits(N) - 2, the offset bits 63 and 31
    MulCase(1024, 40, 100, (100, 50), False, 1, 1, 11),           # 5: one-word draws under fields of five and three words, ew = 11
)
MUL_CONDITIONS = ("s = fbits = 318, one field", "s = fbits = 318, SEL_MAX_FIELDS fields", "end in the top word of N (the largest)",
                  "s a multiple of 32", "offset on a word boundary", "end on a word boundary", "field starts at bit 31 of a word",
                  "kappa = 1", "kappa = 62", "aw = 1 under a multi-word field", "bw = 1 under a multi-word field",
                  "aw at the field's word count", "bw at the field's word count", "ew the smallest", "ew above MUL_FIELD_WORDS",
                  "signed, offset bits on the top bit of a word", "unsigned", "nw = 33", "nw = 96")


def mul_layout(kappa: int, wx: int, wys, nbits: int):
    """(s, offsets, field bits, end); ValueError where the fit rule refuses."""
    if not 1 <= kappa <= 62 or not 1 <= wx <= MUL_MAX_WIDTH or not 1 <= len(wys) <= SEL_MAX_FIELDS:
        raise ValueError("kappa, wx or the field count out of range")
    s = wx + kappa + 1
    offs, fbits, off = [], [], s
    for w in wys:
        if not 1 <= w <= MUL_MAX_WIDTH:
            raise ValueError("width out of range")
        f = w + kappa + 1
        offs.append(off)
        fbits.append(f)
        off += f
        if s + f >= nbits - 1 or off >= nbits - 1:
            raise ValueError("does not fit")
    return s, offs, fbits, off


def mul_ew_min(c) -> int:
    s, _, fbits, _ = mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    return words_of(max([s] + fbits))


def mul_conditions(c) -> set:
    s, offs, fbits, end = mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    nw, got = words_of(c.nbits), set()
    if s == 318 and all(f == 318 for f in fbits) and len(fbits) in (1, SEL_MAX_FIELDS):
        got.add("s = fbits = 318, one field" if len(fbits) == 1 else "s = fbits = 318, SEL_MAX_FIELDS fields")
    if end == c.nbits - 2:
        got.add("end in the top word of N (the largest)")
    if s % 32 == 0:
        got.add("s a multiple of 32")
    if any(o % 32 == 0 for o in offs):
        got.add("offset on a word boundary")
    if end % 32 == 0:
        got.add("end on a word boundary")
    if any(o % 32 == 31 for o in offs):
        got.add("field starts at bit 31 of a word")
    if c.kappa in (1, 62):
        got.add(f"kappa = {c.kappa}")
    if c.aw == 1 and s > 32:
        got.add("aw = 1 under a multi-word field")
    if c.bw == 1 and max(fbits) > 32:
        got.add("bw = 1 under a multi-word field")
    if c.aw == words_of(s) > 1:
        got.add("aw at the field's word count")
    if c.bw == words_of(max(fbits)) > 1:
        got.add("bw at the field's word count")
    if c.ew == mul_ew_min(c):
        got.add("ew the smallest")
    if c.ew > MUL_FIELD_WORDS:               # (row_words sets no largest ew: past MUL_FIELD_WORDS the kernel writes zero words)
        got.add("ew above MUL_FIELD_WORDS")
    if c.signed and (c.wx - 1) % 32 == 31 and any((w - 1) % 32 == 31 for w in c.wy):
        got.add("signed, offset bits on the top bit of a word")
    if not c.signed:
        got.add("unsigned")
    if nw in (33, 96):
        got.add(f"nw = {nw}")
    return got


def mul_draws(c) -> list:
    """(r_a, [r_b_j]) rows: r_a in {0, 1, all ones, random} against every r_b_j in {0, 1, all ones, random}, then mixed random rows.  All
    ones is 2^(w + kappa) - 1, or what the aw / bw words of the row hold where those are fewer."""
    abits = min(c.wx + c.kappa, 32 * c.aw)
    bbits = [min(w + c.kappa, 32 * c.bw) for w in c.wy]
    rng = random.Random(f"kernel-edges:mul-draws:{tuple(c)}")
    rows = []
    for ra in (0, 1, (1 << abits) - 1, rng.getrandbits(abits)):
        for kind in range(4):
            rows.append((ra, [(0, 1, (1 << b) - 1, rng.getrandbits(b))[kind] for b in bbits]))
    rows += [(rng.getrandbits(abits), [rng.getrandbits(b) for b in bbits]) for _ in range(5)]
    return rows


def expected_mul_prep(c, draws) -> dict:
    """e: the planes e_x_0 .. e_x_(nf-1), then e_y."""
    _, offs, _, _ = mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    mask = (1 << (32 * words_of(c.nbits))) - 1
    ox = (1 << (c.wx - 1)) if c.signed else 0
    oys = [(1 << (w - 1)) if c.signed else 0 for w in c.wy]
    ey = [ra + ox for ra, _ in draws]
    ex = [[rbs[j] + oys[j] for _, rbs in draws] for j in range(len(c.wy))]
    return {"e": ex + [ey], "R": [ey[i] + sum(ex[j][i] << offs[j] for j in range(len(offs))) for i in range(len(draws))],
            "rab": [[ex[j][i] * ey[i] & mask for i in range(len(draws))] for j in range(len(offs))]}


def mul_p_rows(c) -> list:
    """P rows below 2^end: every field all ones (highest bit exactly end - 1), all zero, each field alone all ones, each field alone zero,
    random fields."""
    s, offs, fbits, end = mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    rng = random.Random(f"kernel-edges:mul-p:{tuple(c)}")
    sizes, places = [s] + fbits, [0] + offs
    ones = [(1 << f) - 1 for f in sizes]
    fields = [ones, [0] * len(sizes)]
    for i in range(len(sizes)):
        fields.append([ones[k] if k == i else 0 for k in range(len(sizes))])
        fields.append([0 if k == i else ones[k] for k in range(len(sizes))])
    fields += [[rng.getrandbits(f) for f in sizes] for _ in range(6)]
    rows = [sum(v << o for v, o in zip(f, places)) for f in fields]
    assert rows[0] == (1 << end) - 1 and all(r >> end == 0 for r in rows)
    return rows


def expected_mul_split(c, ps) -> dict:
    s, offs, fbits, end = mul_layout(c.kappa, c.wx, c.wy, c.nbits)
    mask = (1 << (32 * words_of(c.nbits))) - 1
    return {"prod": [[(p & ((1 << s) - 1)) * ((p >> o) & ((1 << f) - 1)) & mask for p in ps] for o, f in zip(offs, fbits)],
            "bad": int(any(p >> end for p in ps))}


# ==== inner product ===================================================================================================================
# sc_launch_dot.hip: k pairs (A_j, B_j) of sa = wx + kappa + 1 and sb = wy + kappa + 1 bits, pb = sa + sb (square: the one field, sb = 0);
# g = the largest integer with g pb < bits(N) - 1, M = ceil(k / g) messages; pair j in message j mod M at position t = j div M, A in
# bits [t pb, t pb + sa), B above it; message m ends at n_m pb.  pb' + ceil(log2 k) < bits(N) - 1, pb' = sa + sb (2 sa for a square).
DotCase = collections.namedtuple("DotCase", "nbits kappa wx wy signed square k aw bw ew")
DOT_WIDE_ROWS = 3                     # rows per launch at k = DOT_MAX_K
DOT_LAYOUTS = (
    DotCase(64, 1, 1, 1, False, False, 1, 1, 1, 1),                   # 0: the smallest, k = 1: the batches around one block
    DotCase(1024, 62, 255, 255, True, False, 1024, 10, 10, 10),       # 1: k = DOT_MAX_K of 318 x 318 bits, g = 1, M = 1024
    DotCase(2048, 62, 255, 255, False, False, 1024, 10, 10, 10),      # 2: g = 3, M = 342: the last position holds 340 pairs
    DotCase(704, 1, 18, 42, False, False, 11, 1, 2, 2),               # 3: sa = 20, sb = 44, pb = 64, k = g + 1 = 11, 22 words
    DotCase(386, 31, 32, 32, True, False, 7, 2, 2, 2),                # 4: sa = sb = 64, g pb = 384 = bits(N) - 2, the offset bits 31
    DotCase(64, 1, 26, 26, False, False, 64, 1, 1, 1),                # 5: two words; 56 + 6 bits: k = 65 does not fit
    DotCase(3072, 62, 32, 0, True, True, 33, 3, 0, 3),                # 6: a square, sa = 95, 2 a fills the three exponent words
    DotCase(100, 1, 30, 0, False, True, 5, 1, 0, 2),                  # 7: a square, sa = 32: bit 31 of a is bit 0 of the second word
)
DOT_CONDITIONS = ("k = DOT_MAX_K, sa = sb = 318, g = 1", "k = DOT_MAX_K, sa = sb = 318, g = 3, partial last position", "k = 1", "k = g + 1",
                  "pb a multiple of 32, sa not", "sa and sb multiples of 32", "message end on a word boundary",
                  "message end at bits(N) - 2", "square, sa = 31 mod 32", "square, sa = 0 mod 32", "square, ew below MUL_FIELD_WORDS",
                  "nw below DOT_ACC_WORDS, the largest k that fits", "nw = 22", "nw = 96", "signed", "unsigned", "kappa = 1", "kappa = 62")


def dot_layout(kappa: int, wx: int, wy: int, square: bool, k: int, nbits: int):
    """(sa, sb, pb, g, M, exponent bits); ValueError where the fit rule refuses."""
    if not 1 <= kappa <= 62 or not 1 <= wx <= MUL_MAX_WIDTH or not 1 <= k <= DOT_MAX_K or not (square or 1 <= wy <= MUL_MAX_WIDTH):
        raise ValueError("kappa, a width or k out of range")
    sa = wx + kappa + 1
    sb = 0 if square else wy + kappa + 1
    pb = sa + sb
    g = (nbits - 2) // pb
    if g < 1:
        raise ValueError("one pair does not fit")
    if (2 * sa if square else pb) + _ceil_log2(k) >= nbits - 1:
        raise ValueError("the sum does not fit")
    return sa, sb, pb, g, -(-k // g), (sa + 1 if square else max(sa, sb))


def dot_of(c):
    return dot_layout(c.kappa, c.wx, c.wy, c.square, c.k, c.nbits)


def dot_ends(c) -> list:
    """The end n_m pb of every message."""
    _, _, pb, _, M_, _ = dot_of(c)
    return [len(range(m, c.k, M_)) * pb for m in range(M_)]


def dot_rows_per_launch(c, rows: list) -> list:
    return rows[:DOT_WIDE_ROWS] if c.k == DOT_MAX_K else rows


def dot_conditions(c) -> set:
    sa, sb, pb, g, M_, ebits = dot_of(c)
    nw, ends, got = words_of(c.nbits), dot_ends(c), set()
    if c.k == DOT_MAX_K and sa == sb == 318 and g == 1:
        got.add("k = DOT_MAX_K, sa = sb = 318, g = 1")
    if c.k == DOT_MAX_K and sa == sb == 318 and g == 3 and c.k % M_:
        got.add("k = DOT_MAX_K, sa = sb = 318, g = 3, partial last position")
    if c.k == 1:
        got.add("k = 1")
    if c.k == g + 1:
        got.add("k = g + 1")
    if not c.square and pb % 32 == 0 and sa % 32:
        got.add("pb a multiple of 32, sa not")
    if not c.square and sa % 32 == 0 and sb % 32 == 0:
        got.add("sa and sb multiples of 32")
    if any(e % 32 == 0 for e in ends):
        got.add("message end on a word boundary")
    if any(e == c.nbits - 2 for e in ends):
        got.add("message end at bits(N) - 2")
    if c.square and sa % 32 in (0, 31):
        got.add(f"square, sa = {sa % 32} mod 32")
    if c.square and c.ew < MUL_FIELD_WORDS:
        got.add("square, ew below MUL_FIELD_WORDS")
    if nw < DOT_ACC_WORDS and c.k < DOT_MAX_K and not _fits(dot_layout, c.kappa, c.wx, c.wy, c.square, c.k + 1, c.nbits):
        got.add("nw below DOT_ACC_WORDS, the largest k that fits")
    if nw in (22, 96):
        got.add(f"nw = {nw}")
    got.add("signed" if c.signed else "unsigned")
    if c.kappa in (1, 62):
        got.add(f"kappa = {c.kappa}")
    return got


def _fits(rule, *args) -> bool:
    try:
        rule(*args)
        return True
    except ValueError:
        return False


def _bit31_pattern(bits: int) -> int:
    """Bit 31 of every word that has one below `bits`."""
    return sum(1 << b for b in range(31, bits, 32))


def dot_draws(c) -> list:
    """(r_a [k], r_b [k] or None) rows: every mask all ones (with the signed offsets the sums carry through every word), random, every
    mask 0, every mask 1, bit 31 of every word of every a_j and b_j, random rows.  At k = DOT_MAX_K the first three."""
    abits, bbits = min(c.wx + c.kappa, 32 * c.aw), min(c.wy + c.kappa, 32 * c.bw)
    rng = random.Random(f"kernel-edges:dot-draws:{tuple(c)}")
    ox, oy = ((1 << (c.wx - 1)) if c.signed else 0), ((1 << (c.wy - 1)) if c.signed and not c.square else 0)
    rnd = lambda bits, off: [rng.getrandbits(bits) for _ in range(c.k)]      # noqa: E731
    kinds = [lambda b, off: [(1 << b) - 1] * c.k, rnd, lambda b, off: [0] * c.k, lambda b, off: [1] * c.k,
             lambda b, off: [_bit31_pattern(b) - (_bit31_pattern(b) & off)] * c.k, rnd, rnd]      # (the offset supplies its own bit 31)
    return dot_rows_per_launch(c, [(kind(abits, ox), None if c.square else kind(bbits, oy)) for kind in kinds])


def expected_dot_prep(c, draws) -> dict:
    """e [planes][count] (planes: the b_j then the a_j; a square: 2 a_j), R [M][count], S [count]."""
    sa, _, pb, _, M_, _ = dot_of(c)
    ox, oy = ((1 << (c.wx - 1)), (1 << (c.wy - 1)) if not c.square else 0) if c.signed else (0, 0)
    e, R, S = [[] for _ in range(c.k if c.square else 2 * c.k)], [[] for _ in range(M_)], []
    for r_as, r_bs in draws:
        a = [r + ox for r in r_as]
        b = None if c.square else [r + oy for r in r_bs]
        msgs = [0] * M_
        for j in range(c.k):
            m, t = j % M_, j // M_
            msgs[m] |= a[j] << (t * pb)
            if not c.square:
                msgs[m] |= b[j] << (t * pb + sa)
        for j in range(c.k):
            if c.square:
                e[j].append(2 * a[j])
            else:
                e[j].append(b[j])
                e[c.k + j].append(a[j])
        for m in range(M_):
            R[m].append(msgs[m])
        S.append(sum(v * v for v in a) if c.square else sum(u * v for u, v in zip(a, b)))
    return {"e": e, "R": R, "S": S}


def dot_p_rows(c) -> list:
    """P [M][count] with the fields of every row: all ones (the highest bit of message m exactly at its end - 1), random, all zero,
    alternating all ones and zero, bit 31 of every word of every field, random.  At k = DOT_MAX_K the first three."""
    sa, sb, pb, _, M_, _ = dot_of(c)
    rng = random.Random(f"kernel-edges:dot-p:{tuple(c)}")
    rnd = lambda bits: [rng.getrandbits(bits) for _ in range(c.k)]      # noqa: E731
    kinds = [lambda b: [(1 << b) - 1] * c.k, rnd, lambda b: [0] * c.k, lambda b: [((1 << b) - 1) * (j & 1) for j in range(c.k)],
             lambda b: [_bit31_pattern(b)] * c.k, rnd]
    out = [[] for _ in range(M_)]
    for kind in dot_rows_per_launch(c, kinds):
        A, B = kind(sa), kind(sb)
        msgs = [0] * M_
        for j in range(c.k):
            msgs[j % M_] |= (A[j] | (B[j] << sa)) << (j // M_ * pb)
        for m in range(M_):
            out[m].append(msgs[m])
    return out


def expected_dot_split(c, P) -> dict:
    """From P [M][count]: D [count] and the verdict, every message against its own end."""
    sa, sb, pb, _, M_, _ = dot_of(c)
    ends = dot_ends(c)
    D = []
    for i in range(len(P[0])):
        total = 0
        for m in range(M_):
            for t in range(ends[m] // pb):
                A = (P[m][i] >> (t * pb)) & ((1 << sa) - 1)
                total += A * A if c.square else A * ((P[m][i] >> (t * pb + sa)) & ((1 << sb) - 1))
        D.append(total)
    return {"D": D, "bad": int(first_over(P, ends) is not None)}


def dot_bad_messages(c) -> list:
    """The first, a middle and the last message."""
    M_ = dot_of(c)[4]
    return sorted({0, M_ // 2, M_ - 1})


# ==== one-hot =========================================================================================================================
# sc_launch_lookup.hip: m indices per row; field q of f = ib + kappa + 1 bits in message q div g at bits [(q mod g) f, (q mod g + 1) f),
# g = floor((bits(N) - 2) / f) >= 1 with f < bits(N) - 1; message mm holds n_mm = min(g, m - mm g) fields.  A mask has ib + kappa bits in
# rw >= ceil((ib + kappa) / 32) words, rw <= 3.
OnehotCase = collections.namedtuple("OnehotCase", "nbits kappa ib k m rw count")
ONEHOT_LAYOUTS = (
    OnehotCase(64, 1, 1, 1, 1, 1, 4),                # 0: the smallest, f = 3, k = m = M = 1: the batches around one block and four waves
    OnehotCase(2050, 1, 30, 3, 65, 1, 2),            # 1: f = 32, g f = 2048 = bits(N) - 2 on 65 words, one field in the last message
    OnehotCase(4096, 1, 31, 1024, 2, 1, 3),          # 2: f = 33 (a mask fills its word), k = 1024, 128 words
    OnehotCase(3072, 31, 32, 2, 94, 2, 2),           # 3: f = 64, two full messages of 47 fields ending at bit 3008, 96 words
    OnehotCase(3072, 62, 32, 1023, 2, 3, 2),         # 4: f = 95 over three words against k = 1023
)
ONEHOT_CONDITIONS = ("nw = 65", "nw = 96", "nw = 128", "message end at or above word 64", "f = 32", "f = 33", "f = 64", "f = 95",
                     "k = 1", "k = 2", "k = 3", "k = 1023", "k = 1024", "rw = 1", "rw = 2", "rw = 3", "full last message",
                     "partial last message", "g f = bits(N) - 2")


def onehot_layout(kappa: int, ib: int, k: int, m: int, nbits: int):
    """(f, g, M, words of a mask); ValueError where the fit rule refuses."""
    if not 1 <= kappa <= 62 or not 1 <= ib <= 32 or not 1 <= k <= ONEHOT_MAX_K or not 1 <= m <= 65536:
        raise ValueError("kappa, ib, k or m out of range")
    f = ib + kappa + 1
    if f >= nbits - 1:
        raise ValueError("one field does not fit")
    g = (nbits - 2) // f
    return f, g, -(-m // g), words_of(ib + kappa)


def onehot_of(c):
    return onehot_layout(c.kappa, c.ib, c.k, c.m, c.nbits)


def onehot_ends(c) -> list:
    f, g, M_, _ = onehot_of(c)
    return [min(g, c.m - mm * g) * f for mm in range(M_)]


def onehot_conditions(c) -> set:
    f, g, M_, rw = onehot_of(c)
    nw, ends, got = words_of(c.nbits), onehot_ends(c), set()
    assert rw <= c.rw <= ONEHOT_FIELD_WORDS
    if nw in (65, 96, 128):
        got.add(f"nw = {nw}")
    if any(e >> 5 >= 64 for e in ends):
        got.add("message end at or above word 64")
    if f in (32, 33, 64, 95):
        got.add(f"f = {f}")
    if c.k in (1, 2, 3, 1023, 1024):
        got.add(f"k = {c.k}")
    got.add(f"rw = {c.rw}")
    if M_ > 1:
        got.add("full last message" if c.m % g == 0 else "partial last message")
    if g * f == c.nbits - 2 and c.m >= g:
        got.add("g f = bits(N) - 2")
    return got


def _onehot_kinds(c, bits: int, rng) -> list:
    """Rows of m values of `bits` bits: all ones, random, all zero, all one, random."""
    rnd = lambda: [rng.getrandbits(bits) for _ in range(c.m)]      # noqa: E731
    return [[(1 << bits) - 1] * c.m, rnd(), [0] * c.m, [1] * c.m, rnd()]


def onehot_draws(c) -> list:
    """c.count rows of masks r [m], each below 2^(ib + kappa)."""
    return _onehot_kinds(c, c.ib + c.kappa, random.Random(f"kernel-edges:onehot-draws:{tuple(c)}"))[:c.count]


def expected_onehot_prep(c, draws) -> dict:
    """R [M][count], rot [m][count]."""
    f, g, M_, _ = onehot_of(c)
    R = [[sum(rs[q] << (q % g * f) for q in range(c.m) if q // g == mm) for rs in draws] for mm in range(M_)]
    return {"R": R, "rot": [[rs[q] % c.k for rs in draws] for q in range(c.m)]}


def onehot_p_rows(c) -> list:
    """P [M][count] from c.count rows of fields d [m], each below 2^f; the first row has every field all ones."""
    f, g, M_, _ = onehot_of(c)
    rows = _onehot_kinds(c, f, random.Random(f"kernel-edges:onehot-p:{tuple(c)}"))[:c.count]
    return [[sum(d[q] << (q % g * f) for q in range(c.m) if q // g == mm) for d in rows] for mm in range(M_)]


def expected_onehot_split(c, P) -> dict:
    """From P [M][count]: prod [m][k][count] (the value of a row of nw words: word 0 is the mark, the others 0) and the verdict."""
    f, g, _, _ = onehot_of(c)
    hot = [[((P[q // g][b] >> (q % g * f)) & ((1 << f) - 1)) % c.k for b in range(len(P[0]))] for q in range(c.m)]
    return {"prod": [[[int(t == j) for j in hot[q]] for t in range(c.k)] for q in range(c.m)],
            "bad": int(first_over(P, onehot_ends(c)) is not None)}


def onehot_bad_bits(c, mm: int) -> dict:
    """Bits above the end of message mm: the end itself, word 63, word 64 and the last word (where the row has them above the end)."""
    end, nw = onehot_ends(c)[mm], words_of(c.nbits)
    out = {"end": end, "last word": 32 * nw - 1}
    for name, bit in (("word 63", 32 * 63 + 31), ("word 64", 32 * 64)):
        if end <= bit < 32 * nw:
            out[name] = bit
    return out


# ---- the rotation: (words, k, m, count); m k count rows, one wave each -----------------------------------------------------------------
ROTATE_CASES = ((1, 1, 1, 1), (63, 3, 1, 1), (64, 2, 2, 1), (65, 5, 1, 1), (192, 7, 3, 3), (1, 5, 2, 4), (65, 1024, 1, 8), (63, 3, 1, 8))
ROTATE_WORDS = (1, 63, 64, 65, 192)


def rotate_values(k: int) -> tuple:
    return (0, 1, k - 1, k, 2 * k + 1, (1 << 31) - 1, -1, -k - 1)


def rotate_rot(k: int, m: int, count: int) -> list:
    """rot [m][count]: the values above in turn, starting one further for every q."""
    vals = rotate_values(k)
    return [[vals[(q + q * count + b) % len(vals)] for b in range(count)] for q in range(m)]


def rotate_source(rot: int, k: int, t: int) -> int:
    """The row of e that out[q][t][b] copies.  rot is an int32 that sc_onehot_rotate reads as an UNSIGNED 32-bit number (include/
    sc_amd_dev.h): for 0 <= rot < 2^31 the residue rot mod k, for a negative rot (2^32 + rot) mod k, which is the mathematical residue
    only where k divides 2^32."""
    return (t + (rot % (1 << 32)) % k) % k


def rotate_input(words: int, k: int, m: int, count: int) -> list:
    """e [m][k][count], every row another value of `words` words with its top word non-zero."""
    rng = random.Random(f"kernel-edges:rotate:{words}:{k}:{m}:{count}")
    return [[[rng.getrandbits(32 * words) | 1 << (32 * words - 1) for _ in range(count)] for _ in range(k)] for _ in range(m)]


def expected_rotate(k: int, m: int, count: int, e, rot) -> list:
    return [[[e[q][rotate_source(rot[q][b], k, t)][b] for b in range(count)] for t in range(k)] for q in range(m)]


# ==== coverage ======================================================================================================================
# every kernel launched from csrc/sc_launch_misc.hip, launch_xgcd and the three families' units sc_launch_mul / _dot / _lookup.hip
COVERED_HERE = {
    **{f"k_xgcd<{w}>": "XGCD_WORDS" for w in XGCD_WORDS},
    **{f"k_plain_alice<{lw}>": "PLAIN_L" for lw in sorted({lw_of(l) for l in PLAIN_L})},
    **{f"k_plain_bob<{lw}>": "PLAIN_L" for lw in sorted({lw_of(l) for l in PLAIN_L})},
    "k_select_prep": "SEL_LAYOUTS", "k_select_split": "SEL_LAYOUTS",
    "k_mul_prep": "MUL_LAYOUTS", "k_mul_split": "MUL_LAYOUTS", "k_dot_prep": "DOT_LAYOUTS", "k_dot_split": "DOT_LAYOUTS",
    "k_onehot_prep": "ONEHOT_LAYOUTS", "k_onehot_split": "ONEHOT_LAYOUTS", "k_onehot_rotate": "ROTATE_CASES",
}
_RNG_TEST = "tests/test_gpu_round3.py::test_device_generator_equals_its_restatement"
COVERED_ELSEWHERE = {"k_rng_bits": _RNG_TEST, "k_rng_below": _RNG_TEST, "k_rng_coins": _RNG_TEST, "k_rng_perm": _RNG_TEST,
                     "k_peak_probe": "a multiply-add issue-rate probe: its output is a rate, not a value"}
# the kernels defined in the units whose launches the ledger above does not parse: the interpreter and the axis kernels, by the test
# that runs every compiled instance of each
DEFINED_ELSEWHERE = {"k_vm": "tests/test_gpu_instance_matrix.py::test_instance", "k_pvm": "tests/test_gpu_instance_matrix.py::test_instance",
                     "k_prod_axis": "tests/test_gpu_aggregate.py::test_instance", "k_scan_axis": "tests/test_gpu_scan.py::test_instance",
                     "k_lin_lift": "tests/test_gpu_linear.py::test_instance", "k_lin_axis": "tests/test_gpu_linear.py::test_instance"}

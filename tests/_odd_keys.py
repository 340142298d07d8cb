"""Paillier keys that do not fill their words (tests/golden/keys_odd.json), what the host policy does with them, and the widths the
family tests run on them.

Pure Python (no torch at import): tests/test_odd_keys_cpu.py checks this module on a machine without a GPU;
tests/test_gpu_odd_keys.py runs it.  Nothing here is a literal: the conditions, the kernel configurations and the instances a call
must launch come from the policy restated in tests/_instance_matrix.py (first_fit, pair_capable, has_neg1_multiple, nwords_of), and
the widths from the package's own layout classes, imported only when a width is asked for.

How sc_paillier_key_create lays a key out (csrc/sc_schemes.hip): N in nw = nwords(N) words; N^2 in 2 nw words, whatever its own
length; both primes in hw = nwords(max(bits(p), bits(q))) words, so the shorter prime is padded; p^2 and q^2 in 2 hw words each.
"""
from __future__ import annotations

import functools
import json
import os
from dataclasses import dataclass

import _instance_matrix as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (521, 1025, 1040, 1041, 1100, 1540)

CONDITIONS = ("partial_top_word", "n2_top_word_zero", "n2_moved_by_whole_words", "n_on_L27_with_L14_pair_twin", "n_on_own_pair_config",
              "unequal_prime_bits", "unequal_prime_words", "prime_squares_on_different_configs", "n2_on_L14")
# what the padding of the shorter prime does (found while these tests were written): a condition of its own
EXTRA_CONDITIONS = ("shorter_prime_moved_by_padding", "prime_squares_joined_by_padding")


@dataclass(frozen=True)
class OddKey:
    bits: int
    seed: int
    p: int
    q: int

    @property
    def n(self) -> int:
        return self.p * self.q

    @property
    def n2(self) -> int:
        return self.n * self.n

    @property
    def nw(self) -> int:
        return M.nwords_of(self.n.bit_length())

    @property
    def hw(self) -> int:
        return M.nwords_of(max(self.p.bit_length(), self.q.bit_length()))

    def oracle(self):
        from oracle import sc_oracle as o

        return o.PaillierKey(self.n, self.p, self.q)


@functools.lru_cache(maxsize=None)
def load() -> dict:
    """{bits: OddKey} of tests/golden/keys_odd.json."""
    raw = json.load(open(os.path.join(GOLDEN, "keys_odd.json")))
    return {v["bits"]: OddKey(v["bits"], v["seed"], int(v["p"], 16), int(v["q"], 16)) for v in raw.values()}


# ---- the host policy on a key's moduli ---------------------------------------------------------------------------------------------
def config(n: int, words: int | None = None):
    """The configuration sc_mod_create gives `n` stored in `words` words (default: its own)."""
    return M.first_fit(n.bit_length(), words)


def pair_config(n: int, words: int | None = None):
    """Where a pair call (sc_modexp_shared_sq) modulo n^2 runs: n's own configuration when it has a pair kernel, else the first
    pair-capable one that holds n in `words` words (pair_twin)."""
    own = config(n, words)
    return own if own and M.pair_capable(*own) else M.first_fit(n.bit_length(), words, for_pairs=True)


def vm(cfg) -> tuple:
    return ("vm", cfg[0], cfg[1], M.W, False, False, False)


def pvm(n: int, words: int | None = None) -> tuple:
    """The pair instance of a chip-filling or small pair call modulo n^2 with the small-batch policy off: the NEG1 one when n = -1
    (mod 2^29) or its multiple M = c n fits the pair configuration."""
    cfg = pair_config(n, words)
    neg1_kernel = cfg in ((4, 18), (4, 14), (8, 14))
    return ("pvm", cfg[0], cfg[1], M.W, (neg1_kernel and M.is_neg1(n)) or M.has_neg1_multiple(n, cfg), False, False)


def moduli(key: OddKey) -> dict:
    """{name: (modulus, words it is stored in)} as sc_paillier_key_create makes them."""
    return {"n": (key.n, key.nw), "n2": (key.n2, 2 * key.nw), "p": (key.p, key.hw), "q": (key.q, key.hw),
            "p2": (key.p * key.p, 2 * key.hw), "q2": (key.q * key.q, 2 * key.hw)}


def configs(key: OddKey) -> dict:
    return {name: config(*mw) for name, mw in moduli(key).items()}


def conditions(key: OddKey) -> dict:
    """{condition name: bool} for CONDITIONS + EXTRA_CONDITIONS, computed from the key."""
    n, p, q = key.n, key.p, key.q
    nbits, n2bits = n.bit_length(), key.n2.bit_length()
    cfg = configs(key)
    own_p2, own_q2 = config(p * p), config(q * q)                  # each square in its own words: what no padding would give
    return {
        "partial_top_word": nbits % 32 != 0,
        "n2_top_word_zero": M.nwords_of(n2bits) < 2 * key.nw,
        "n2_moved_by_whole_words": cfg["n2"] != config(key.n2),
        "n_on_L27_with_L14_pair_twin": cfg["n"][1] == 27 and pair_config(n, key.nw)[1] == 14,
        "n_on_own_pair_config": pair_config(n, key.nw) == cfg["n"],
        "unequal_prime_bits": p.bit_length() != q.bit_length(),
        "unequal_prime_words": M.nwords_of(p.bit_length()) != M.nwords_of(q.bit_length()),
        # the issue's reading: each square where its own length would put it.  The library pads both to 2 hw words, see below
        "prime_squares_on_different_configs": own_p2 != own_q2,
        "n2_on_L14": cfg["n2"][1] == 14,
        "shorter_prime_moved_by_padding": cfg["p"] != config(p) or cfg["q"] != config(q),
        "prime_squares_joined_by_padding": own_p2 != own_q2 and cfg["p2"] == cfg["q2"],
    }


def padded_squares_can_differ() -> list:
    """Every (hw, bits(p^2), bits(q^2)) for which two squares stored in 2 hw words, the longer prime filling hw words, would get
    different configurations.  Empty: the whole-words rule decides before the lengths do, so the CRT halves of one key always run
    on one instance."""
    out = []
    for hw in range(1, M.MAX_BITS // 64 + 1):
        top = 64 * hw                                            # bits(q^2) is 2 bits(q) or one less; bits(q) in (32 (hw - 1), 32 hw]
        seen = {M.first_fit(b, 2 * hw) for b in range(2, top + 1)}
        if len(seen - {None}) > 1:
            out.append((hw, sorted(seen - {None})))
    return out


def has_axis_instance(key: OddKey) -> bool:
    """Does the configuration of the key's N^2 have k_prod_axis / k_scan_axis / k_lin_axis instances?"""
    import _reduce_model as R

    return configs(key)["n2"] in set(R.INSTANCES)


# ---- the launch_counts() keys a call must add to ---------------------------------------------------------------------------------------
def instances(key: OddKey) -> dict:
    """{call: set of launch_counts() keys that must grow}, with the small-batch and the one-lane policies off (latency mode 0,
    one-lane mode 0).  `allowed` holds every instance any of the key's moduli can run on: nothing else may grow."""
    mods, cfg = moduli(key), configs(key)
    halves = {vm(cfg["p"]), vm(cfg["q"]), vm(cfg["p2"]), vm(cfg["q2"])}
    pair_halves = {pvm(*mods["p"]), pvm(*mods["q"])}
    out = {
        "randomizer_public": {pvm(*mods["n"]), vm(cfg["n2"])},
        "randomizer_public_no_pairs": {vm(cfg["n2"])},
        "randomizer_crt": halves | pair_halves | {vm(cfg["n2"])},
        "decrypt_crt": halves | pair_halves | {vm(cfg["n"])},
        "decrypt_crt_no_pairs": set(halves) | {vm(cfg["n"])},
        "decrypt_no_crt": {pvm(*mods["n"]), vm(cfg["n2"]), vm(cfg["n"])},
        "decrypt_no_crt_no_pairs": {vm(cfg["n2"]), vm(cfg["n"])},
    }
    out["allowed"] = {vm(c) for c in cfg.values()} | pair_halves | {pvm(*mods["n"])}
    return out


def batch_sizes(key: OddKey) -> list:
    """1 and NG + 1 items of the instance N^2 runs on (at most 24)."""
    return [1, min(24, 64 // configs(key)["n2"][0] + 1)]


# ---- widths ------------------------------------------------------------------------------------------------------------------------
def _three_words(off: int, f: int) -> bool:
    return (off + f - 1) // 32 - off // 32 >= 2


def mul_widths(key: OddKey, columns: int = 4) -> dict:
    """kappa, wx and `columns` widths whose last field ends exactly at nbits - 2 (MulLayout.end): the seed widths 32 | 17, 5, 64, 1 of
    the existing unaligned case, grown from the last column down, kappa = 40 where five fields of at most 255 bits reach the end, else
    62.  `refused`: the same with the last column one bit wider."""
    from protocols.secure_comparison_amd.multiplication import MAX_WIDTH, MulLayout

    nbits = key.n.bit_length()
    seed = [32, 17, 5, 64, 1][:columns + 1]
    for kappa in (40, 62):
        rest = nbits - 2 - (columns + 1) * (kappa + 1) - sum(seed)
        if 0 <= rest <= (columns + 1) * (MAX_WIDTH - 1) - sum(seed):
            break
    else:
        raise ValueError(f"no {columns}-column layout ends at {nbits - 2}")
    w = list(seed)
    for j in range(columns, -1, -1):
        add = min(rest, MAX_WIDTH - 1 - w[j])
        w[j] += add
        rest -= add
    lay = MulLayout(kappa, w[0], tuple(w[1:]), True, nbits)
    assert lay.end == nbits - 2
    fields = [(0, lay.s)] + list(zip(lay.offsets, lay.fbits))
    return {"kappa": kappa, "wx": w[0], "wy": w[1:], "layout": lay, "refused": (kappa, w[0], tuple(w[1:-1]) + (w[-1] + 1,)),
            "ends_at_nbits_minus_2": lay.end == nbits - 2, "three_word_field": any(_three_words(o, f) for o, f in fields),
            "unaligned_offsets": [o % 32 for o in lay.offsets]}


def dot_widths(key: OddKey, square: bool = False) -> dict:
    """kappa, wx, wy with g pairs of pb bits per message, g pb = nbits - 2 where nbits - 2 has a divisor in reach (g from 2 to 16),
    else the g = 2 layout that comes closest.  k = g gives one message, k = g + 1 two."""
    from protocols.secure_comparison_amd.dotproduct import MAX_WIDTH, DotLayout

    nbits = key.n.bit_length()
    sides = 1 if square else 2
    best = None
    for kappa in (40, 62, 20):
        for g in range(2, 17):
            pb = (nbits - 2) // g
            total = pb - sides * (kappa + 1)
            if not sides <= total <= sides * MAX_WIDTH:
                continue
            exact = g * pb == nbits - 2
            if best is None or (exact and not best[0]):
                best = (exact, kappa, g, total)
        if best and best[0]:
            break
    exact, kappa, g, total = best
    wx = total if square else (total + 1) // 2
    wy = 0 if square else total - wx
    lay = DotLayout(kappa, wx, wy, g + 1, True, square, nbits)
    assert lay.g == g and lay.M == 2
    # the fit rule on one pair: the widest wy beside wx = 255 with k = 1, and one bit more, where 255 + wy can reach the end at all
    refused = None
    room = nbits - 2 - 2 * (kappa + 1) - MAX_WIDTH
    if not square and 1 <= room < MAX_WIDTH:
        refused = {"admitted": (kappa, MAX_WIDTH, room, 1), "refused": (kappa, MAX_WIDTH, room + 1, 1)}
    return {"kappa": kappa, "wx": wx, "wy": wy, "g": g, "layout": lay, "ends_at_nbits_minus_2": exact, "fit": refused,
            "three_word_field": any(_three_words(t * lay.pb, lay.sa) or (not square and _three_words(t * lay.pb + lay.sa, lay.sb)) for t in range(g))}


def onehot_widths(key: OddKey) -> dict:
    """kappa, index_bits with g fields of f bits per message, g f = nbits - 2 where a divisor gives at most 24 fields, else the widest field,
    kappa = 62 and index_bits = 32 (95 bits: three or four words).  m = g + 1 indices leave a last message with one field; k = 3."""
    from protocols.secure_comparison_amd.lookup import OnehotLayout

    nbits = key.n.bit_length()
    pick = None
    for kappa in range(62, 19, -1):
        for ib in range(32, 0, -1):
            f = ib + kappa + 1
            g = (nbits - 2) // f
            if g * f == nbits - 2 and 2 <= g <= 24 and pick is None:
                pick = (kappa, ib)
    kappa, ib = pick or (62, 32)
    g = (nbits - 2) // (ib + kappa + 1)
    lay = OnehotLayout(kappa, ib, 3, g + 1, nbits)
    assert lay.g == g and lay.M == 2
    return {"kappa": kappa, "index_bits": ib, "k": 3, "m": g + 1, "g": g, "layout": lay, "ends_at_nbits_minus_2": g * lay.f == nbits - 2,
            "three_word_field": any(_three_words(t * lay.f, lay.f) for t in range(g))}


def select_widths(key: OddKey, nf: int, kappa: int = 40) -> dict:
    """nf column widths whose last field ends exactly at nbits - 2 (SelectLayout.end), each column 3 bits wider than the one before so
    that no two offsets share a residue modulo 32 by design.  `refused`: the last column one bit wider."""
    from protocols.secure_comparison_amd.selection import SelectLayout

    nbits = key.n.bit_length()
    total = nbits - 2 - (kappa + 1) - nf * (kappa + 2)
    base = (total - 3 * nf * (nf - 1) // 2) // nf
    w = [base + 3 * j for j in range(nf)]
    w[-1] += total - sum(w)
    lay = SelectLayout(w[0], kappa, tuple(w[1:]), nbits)
    assert lay.end == nbits - 2
    return {"kappa": kappa, "widths": w, "layout": lay, "refused": w[:-1] + [w[-1] + 1], "ends_at_nbits_minus_2": True,
            "three_word_field": any(_three_words(o, f) for o, f in zip(lay.offsets, lay.fbits))}


def linear_x_bits(key: OddKey, rows: list) -> int:
    """The largest x_bits check_fit admits for these weight rows under this key: bits(sum |w|) + x_bits + 1 < nbits - 1."""
    return key.n.bit_length() - 3 - max(sum(abs(v) for v in row).bit_length() for row in rows)

"""The compiled interpreter instances as data: which moduli, policy switches, operands and exponents land a call on each of the 37
k_vm / k_pvm template instances, and plain-integer references for every primitive the matrix runs on them.

Pure Python (no torch at import): tests/test_instance_matrix_cpu.py checks this table against the launcher sources and the first-fit
rule on a machine without a GPU; tests/test_gpu_instance_matrix.py runs it.  The routes restate csrc/sc_route.h, the header that holds the policy (sc_lib.hip applies
it); the restatement stays independent of it, and tests/test_route_cpu.py compares the two rule by rule without a GPU:

* sc_mod_create takes the first kConfigs entry with capacity W G L >= bits + 8 that also holds whole words (32 nwords <= W G L).  The
  whole-words condition moves the largest modulus of a configuration below 29 G L - 8 wherever that size needs another word:
  (2,18) ends at 1024 bits, not 1036.  `size_range` scans the rule instead of trusting a formula.
* latency mode 2 runs an L = 18 modulus of G <= 8 on k_vm<2G, 9>; one-lane mode 2 runs shared exponents of more than 64 bits on
  k_vm<1, 37, 28> when the modulus has at most 32 words -- so 1024 bits is the widest modulus that reaches it, although 28 * 37 - 8 =
  1028 bits is the capacity DESIGN.md quotes (ONE_LANE_UNREACHABLE_BITS records the finding).
* k_vm<4, 18, NEG1> runs (4,18) moduli = -1 (mod 2^29), and sc_modexp_var of any (4,18) modulus of at most 2051 bits through the
  multiple M = c n.
* pair calls (sc_modexp_shared_sq) run on the modulus's own configuration when it has a pair kernel, else on the first pair-capable
  one that fits: (4,14) for (2,27) moduli, (8,14) for (4,27) ones, and (16,18) for the 4161 .. 4172-bit moduli whose square still
  fits the library -- the only road to k_pvm<16, 18>.  Chip-filling pair calls of (4,18) / (4,14) / (8,14) moduli run modulo
  M = c n on the NEG1 instances when M fits (bits + 37 <= 29 G L, and M in whole words below R), else on the plain ones; latency mode 2 takes the (4G, 5) twins of
  (G,18) moduli, G <= 4.  k_pvm<2G, 9> is reached only with latency mode 1, a chip share of 64 and a batch between the two
  thresholds (the (4G, 5) twin declined, the small-batch configuration still chosen): see `pair9_counts`.
* the DIG instances run sc_modexp_var_sq; the STAMP twin runs inside sc_clock_probe, which discards its residues (only its launch
  can be observed).
"""
from __future__ import annotations

import functools
import math
import random
from dataclasses import dataclass, field

W = 29
K_CONFIGS = [(1, 18), (2, 18), (2, 27), (4, 14), (4, 18), (4, 27), (8, 14), (8, 18), (8, 27), (16, 14), (16, 18)]
ONE_LANE = (1, 37, 28)
MAX_BITS = 29 * 16 * 18 - 8
MIN_BITS = 64                             # (1,18) has no configuration below it: the matrix starts at three limbs
ONE_LANE_UNREACHABLE_BITS = 1028          # fits 28 * 37 - 8 but has 33 words: onelane_for declines it

# (kind, G, L, W, neg1, stamp, dig) -- the key of Engine.launch_counts()
VM = [("vm", g, l, 29, False, False, False) for g, l in
      [(4, 18), (2, 18), (1, 18), (2, 9), (4, 9), (8, 18), (16, 18), (8, 9), (16, 9), (2, 27), (4, 27), (8, 27), (4, 14), (8, 14), (16, 14)]] + \
     [("vm", 4, 18, 29, True, False, False), ("vm", 1, 37, 28, False, False, False)]
PVM = [("pvm", g, l, 29, False, False, False) for g, l in
       [(4, 18), (2, 18), (1, 18), (8, 18), (16, 18), (2, 9), (4, 9), (8, 9), (4, 5), (8, 5), (16, 5), (4, 14), (8, 14)]] + \
      [("pvm", 4, 18, 29, True, False, False), ("pvm", 4, 14, 29, True, False, False), ("pvm", 8, 14, 29, True, False, False),
       ("pvm", 4, 18, 29, True, True, False),
       ("pvm", 2, 18, 29, False, False, True), ("pvm", 4, 18, 29, False, False, True), ("pvm", 8, 14, 29, False, False, True)]
INSTANCES = VM + PVM


def instance_id(inst) -> str:
    kind, g, l, w, neg1, stamp, dig = inst
    return f"{kind}-{g}x{l}" + ("" if w == 29 else f"w{w}") + ("-neg1" if neg1 else "") + ("-stamp" if stamp else "") + ("-dig" if dig else "")


# ---- the host policy, restated ---------------------------------------------------------------------------------------------------
def nwords_of(bits: int) -> int:
    return (bits + 31) // 32


def pair_capable(g: int, l: int) -> bool:
    return l == 18 or (l == 14 and g in (4, 8)) or (l == 5 and g in (4, 8, 16))


def first_fit(bits: int, nwords: int | None = None, for_pairs: bool = False):
    """The configuration sc_mod_create (for_pairs: the pair twin) gives a modulus of `bits` bits in `nwords` words, or None."""
    nwords = nwords or nwords_of(bits)
    for need_words in (True, False):
        for g, l in K_CONFIGS:
            if for_pairs and not pair_capable(g, l):
                continue
            cap = W * g * l
            if cap >= bits + 8 and (not need_words or cap >= 32 * nwords):
                return (g, l)
    return None


@functools.lru_cache(maxsize=None)
def size_range(cfg) -> tuple[int, int]:
    """Smallest and largest bit length whose first-fit configuration is `cfg`."""
    hits = [b for b in range(MIN_BITS, MAX_BITS + 1) if first_fit(b) == cfg]
    return hits[0], hits[-1]


def pair_config(bits: int):
    own = first_fit(bits)
    return own if own and pair_capable(*own) else first_fit(bits, for_pairs=True)


def neg1_multiple(n: int):
    """M = c n with c = -n^-1 mod 2^29, so that M = -1 (mod 2^29)."""
    return n * ((-pow(n, -1, 1 << 29)) % (1 << 29))


def has_neg1_multiple(n: int, cfg) -> bool:
    """Does neg1_twin build M = c n for this modulus in this configuration?  n itself not = -1 (mod 2^29), the 8 guard bits left
    whatever c is, and M in whole words below R (a wide operand is read in raw chunks of M's words)."""
    g, l = cfg
    cap = W * g * l
    return ((l == 18 and g == 4) or (l == 14 and g in (4, 8))) and not is_neg1(n) and n.bit_length() + 29 + 8 <= cap and \
        32 * nwords_of(neg1_multiple(n).bit_length()) <= cap


def onelane_fits(bits: int) -> bool:
    return bits + 8 <= 28 * 37 and 32 * nwords_of(bits) <= 28 * 37


# ---- moduli ------------------------------------------------------------------------------------------------------------------------
SHAPES = ("neg1", "one", "rand", "allones", "square")


def make_modulus(bits: int, shape: str) -> int:
    """A deterministic odd modulus of exactly `bits` bits: low limb all ones (n = -1 mod 2^29), low limb 1, seeded random, every bit
    set, or the square of a seeded odd number (a Paillier N^2: what the exact-limb ops of the encryption are defined on)."""
    rng = random.Random(f"instance-matrix:{bits}:{shape}")
    top = 1 << (bits - 1)
    if shape == "allones":
        return (1 << bits) - 1
    if shape == "square":
        lo, hi = math.isqrt(top - 1) + 1, math.isqrt((1 << bits) - 1)
        r = rng.randrange(lo, hi) | 1
        r = r if r <= hi else r - 2
        assert (r * r).bit_length() == bits
        return r * r
    n = rng.getrandbits(bits) | top | 1
    if shape == "neg1":
        n |= (1 << 29) - 1
    elif shape == "one":
        n = (n >> 29 << 29) | 1
    assert n.bit_length() == bits and shape in SHAPES
    return n


def is_neg1(n: int) -> bool:
    return n % (1 << 29) == (1 << 29) - 1


@dataclass(frozen=True)
class Case:
    """One modulus and the switches under which its calls land on the instance."""
    label: str
    n: int
    latency: int = 0
    onelane: int = 0
    chip_share: int = 1
    pair: bool = False            # the instance is reached by pair calls (sc_modexp_shared_sq / sc_modexp_var_sq), not single-modulus ones
    pair9: bool = False           # counts from pair9_counts (the k_pvm<2G, 9> window)
    primary: tuple = field(default=(0, 0))    # the configuration sc_mod_create gives n

    @property
    def bits(self) -> int:
        return self.n.bit_length()


def _family(cfg, shapes, sizes=None, **kw) -> list[Case]:
    lo, hi = size_range(cfg)
    out = []
    for bits in (sizes or (lo, hi)):
        for shape in shapes:
            if shape in ("allones", "square") and bits != (sizes or (lo, hi))[-1]:
                continue
            n = make_modulus(bits, shape)
            out.append(Case(f"{bits}-{shape}", n, primary=cfg, **kw))
    return out


ALL = ("neg1", "one", "rand", "allones", "square")
NOT_NEG1 = ("one", "rand", "square")
ONLY_NEG1 = ("neg1", "allones")


def cases_for(inst) -> list[Case]:
    seen, out = set(), []
    for c in _cases_for(inst):
        if c.n not in seen:
            seen.add(c.n)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _cases_for(inst) -> list[Case]:
    """The deterministic moduli (with their switches) that must land on `inst`.  Empty for the STAMP twin (sc_clock_probe)."""
    kind, g, l, w, neg1, stamp, dig = inst
    if kind == "vm":
        if (g, l, w) == ONE_LANE:
            # shared exponents of more than 64 bits only; any modulus of at most 32 words
            return [Case(f"{b}-{s}", make_modulus(b, s), onelane=2, primary=first_fit(b)) for b, s in
                    ((64, "rand"), (523, "rand"), (1024, "neg1"), (1024, "one"), (1024, "allones"), (1024, "rand"))]
        if l == 9:
            base = (g // 2, 18)
            return _family(base, ("neg1", "one", "rand", "allones"), latency=2)
        if neg1:            # native n = -1 (every primitive), and the multiple M = c n of other moduli (sc_modexp_var only)
            return _family((4, 18), ONLY_NEG1) + [Case("2048-rand-multiple", make_modulus(2048, "rand"), primary=(4, 18)),
                                                  Case("2051-one-multiple", make_modulus(2051, "one"), primary=(4, 18))]
        if (g, l) == (4, 18):   # n = -1 would run the NEG1 instance; 2052 / 2080 bits: too long for M = c n, so sc_modexp_var stays here
            return _family((4, 18), NOT_NEG1) + _family((4, 18), ("one", "rand"), sizes=(2052, 2080))
        return _family((g, l), ALL)
    # ---- pair instances
    if stamp:
        return []
    if dig:
        if (g, l) == (8, 14):
            return [Case(f"{b}-{s}", make_modulus(b, s), pair=True, primary=first_fit(b)) for b, s in
                    ((3072, "rand"), (3072, "neg1"), (2081, "one"), (3232, "rand"), (3232, "allones"))]
        return _family((g, l), ("neg1", "one", "rand", "allones"), pair=True)
    if l == 5:
        return _family((g // 4, 18), ("neg1", "one", "rand", "allones"), latency=2, pair=True)
    if l == 9:
        return _family((g // 2, 18), ("neg1", "one", "rand", "allones"), latency=1, chip_share=64, pair=True, pair9=True)
    if l == 18 and g == 16:     # pair twin of (8,27) moduli whose square still fits: 4161 .. 4172 bits
        return [Case(f"{b}-{s}", make_modulus(b, s), pair=True, primary=first_fit(b)) for b, s in
                ((4161, "neg1"), (4161, "one"), (4161, "rand"), (4172, "neg1"), (4172, "one"), (4172, "rand"), (4172, "allones"))]
    if l == 18 and g != 4:
        return _family((g, 18), ("neg1", "one", "rand", "allones"), pair=True)
    # (4,18), (4,14), (8,14): NEG1 for n = -1 and for every modulus whose multiple M = c n fits, the plain instance for the others.
    # One family of candidates for both instances, each placed where the restated policy sends it: the ends of the configuration's
    # own range and of the L = 27 range below it (pair twin), the longest size whose M holds whole words for every c, and
    # cap - 37, the longest size with the guard bits left -- where M needs one word more than the limbs hold and a 4-chunk operand
    # came out wrong while such moduli still got a twin (1587 bits on (4,14), 3211 on (8,14)): they must run on the plain instance.
    cap = W * g * l
    own_lo, own_hi = size_range((g, l))
    whole = max(b for b in range(own_lo, cap - 36) if 32 * nwords_of(b + 29) <= cap)
    sizes = [own_lo, whole, cap - 37, cap - 36, own_hi]
    if l == 14:
        sizes = list(size_range({(4, 14): (2, 27), (8, 14): (4, 27)}[(g, l)])) + sizes
    out = []
    for b in dict.fromkeys(sizes):
        for s in ("neg1", "one", "rand") + (("allones",) if b == own_hi else ()):
            c = Case(f"{b}-{s}", make_modulus(b, s), pair=True, primary=first_fit(b))
            if expected_instance(c, "pvm") == inst[:5]:
                out.append(c)
    return out


def moduli_for(inst) -> list[int]:
    return [c.n for c in cases_for(inst)]


def expected_instance(case: Case, inst_kind: str, shared_exp_bits: int = 65):
    """Where the restated policy sends a call of `case` (a cross-check of cases_for, used by the CPU tier): the (kind, G, L, W, neg1)
    of a single-modulus shared exponentiation (kind "vm") or of a pair call (kind "pvm") with these switches."""
    bits, n = case.bits, case.n
    g, l = first_fit(bits)
    if inst_kind == "vm":
        if case.onelane == 2 and shared_exp_bits > 64 and onelane_fits(bits):
            return ("vm",) + ONE_LANE + (False,)
        if case.latency == 2 and l == 18 and g <= 8:
            return ("vm", 2 * g, 9, 29, False)
        return ("vm", g, l, 29, (g, l) == (4, 18) and is_neg1(n))
    if case.latency == 2 and l == 18 and g <= 4:
        return ("pvm", 4 * g, 5, 29, False)
    pg, pl = pair_config(bits)
    if case.pair9:
        return ("pvm", 2 * pg, 9, 29, False)
    native = is_neg1(n) and ((pg, pl) == (4, 18) or (pl == 14 and pg in (4, 8)))
    return ("pvm", pg, pl, 29, native or has_neg1_multiple(n, (pg, pl)))


# ---- counts ------------------------------------------------------------------------------------------------------------------------
def items_per_wave(inst) -> int:
    return 64 // inst[1]


def counts_for(inst) -> list[int]:
    ng = items_per_wave(inst)
    return [1, ng - 1, ng, ng + 1, 2 * ng + 3]


def pair9_counts(inst, num_cu: int) -> list[int]:
    """Batches that take k_pvm<2G, 9> under latency mode 1 and chip share 64: above the (4G, 5) twin's threshold of num_cu * 2 / 64
    waves of 64 / 2G items, and far below the small-batch threshold of 2 num_cu waves of the (G,18) form."""
    ng = items_per_wave(inst)
    base = (num_cu * 2 // 64) * ng
    assert base + 2 * ng + 3 <= 2 * num_cu * 2 * ng
    return [base + 1, base + ng - 1, base + ng, base + ng + 1, base + 2 * ng + 3]


def over_one_round(inst, num_cu: int) -> int:
    """More items than every resident wave of a full chip holds (the launchers clamp occupancy to 16): the grid-stride loop runs."""
    ng = items_per_wave(inst)
    return num_cu * 16 * ng + ng + 1


TILE = 257                                   # distinct operands of the large batch; coprime to every NG


# ---- operands and exponents ------------------------------------------------------------------------------------------------------
def edge_operands(n: int, inst) -> list[int]:
    _, g, l, w = inst[:4]
    bits, r = n.bit_length(), 1 << (w * g * l)
    limbs_all_ones = (1 << (w * g * l)) - 1
    vals = [0, 1, 2, n - 1, n - 2, (n + 1) // 2, (n - 1) // 2, (1 << (bits - 1)) - 1, r % n, r * r % n, limbs_all_ones % n]
    return [v % n for v in vals]


def operands(n: int, inst, count: int, salt: int = 0) -> list[int]:
    """`count` residues: the edge operands (rotated by `salt`, so that short batches take different ones) and seeded random fill."""
    edge = edge_operands(n, inst)
    rng = random.Random(f"ops:{n & 0xffffffff}:{count}:{salt}")
    rot = [edge[(i + salt) % len(edge)] for i in range(len(edge))]
    return (rot + [rng.randrange(n) for _ in range(max(0, count - len(rot)))])[:count]


def coprime_operands(n: int, inst, count: int, salt: int = 0) -> list[int]:
    """What sc_modinv is given: the edge operands coprime to n first, then seeded random coprime residues."""
    edge = [v for v in edge_operands(n, inst) if v and math.gcd(v, n) == 1]
    rng = random.Random(f"inv:{n & 0xffffffff}:{count}:{salt}")
    out = list(dict.fromkeys(edge))
    while len(out) < count:
        v = rng.randrange(1, n)
        if math.gcd(v, n) == 1:
            out.append(v)
    return out[:count]


def shared_exponents(n: int) -> list[int]:
    bits = n.bit_length()
    alt = 0
    for k in range(0, 400, 32):               # alternating 16-bit runs: zero runs longer than any sliding window
        alt |= 0xffff << (k + 16)
    alt &= (1 << 400) - 1
    full = random.Random(f"exp:{n & 0xffffffff}").getrandbits(bits) | (1 << (bits - 1))
    return [0, 1, 2, 3, 1 << 64, (1 << 65) - 1, (1 << 160) + 1, alt, full]


VAR_EBITS = (1, 5, 35, 67)


def row_exponents(ebits: int, count: int, salt: int = 0) -> list[int]:
    rng = random.Random(f"rowexp:{ebits}:{count}:{salt}")
    special = [0, 1, (1 << ebits) - 1]
    rot = [special[(i + salt) % 3] for i in range(3)]
    return (rot + [rng.getrandbits(ebits) for _ in range(max(0, count - 3))])[:count]


# ---- references: Python integers only ------------------------------------------------------------------------------------------------
def expected_modmul(n, a, b):
    count = max(len(a), len(b))
    a, b = (a * count if len(a) == 1 else a), (b * count if len(b) == 1 else b)
    return [x * y % n for x, y in zip(a, b)]


def expected_modmul_const(n, a, c):
    return [x * c % n for x in a]


def expected_modmul_const_sel(n, a, c0, c1, flags):
    k0, k1 = (1 if c0 is None else c0), (1 if c1 is None else c1)
    return [x * (k1 if f else k0) % n for x, f in zip(a, flags)]


def expected_modexp_shared(n, xs, e, mul_into=None):
    r = [pow(x, e, n) for x in xs]
    return r if mul_into is None else [a * b % n for a, b in zip(r, mul_into)]


def expected_isone(n, xs, e):
    return [int(pow(x, e, n) == 1) for x in xs]


def expected_isone_any(n, xs, e, inner):
    flags = expected_isone(n, xs, e)
    return [int(any(flags[b::inner])) for b in range(inner)]


def expected_modexp_var(n, xs, es, base=None, e2=None, dest=None):
    r = [pow(x, e, n) for x, e in zip(xs, es)]
    if base is not None:
        r = [a * pow(base, k, n) % n for a, k in zip(r, e2)]
    if dest is not None:
        placed = [None] * len(r)
        for i, d in enumerate(dest):
            placed[d] = r[i]
        r = placed
    return r


def expected_fixedbase_pow(n, base, es, mul_into=None):
    r = [pow(base, e, n) for e in es]
    return r if mul_into is None else [a * b % n for a, b in zip(r, mul_into)]


def expected_modinv(n, xs):
    return [pow(x, -1, n) for x in xs]


def expected_paillier_encrypt_raw(big_n, ms, negate=False):
    n2 = big_n * big_n
    return [(1 - (m % big_n) * big_n) % n2 if negate else (1 + (m % big_n) * big_n) % n2 for m in ms]


def expected_paillier_l_mul(n, k, xs):
    return [((x % (n * n)) - 1) // n * k % n for x in xs]


def expected_crt_combine(mp, mq, a_p, a_q):
    k = pow(mq, -1, mp)
    return [(y + mq * ((x - y) * k % mp)) % (mp * mq) for x, y in zip(a_p, a_q)]


def expected_select_finish_cx(n, t, ab, u_inv, f, g):
    hi = [x * b % n * b % n * u % n for x, b, u in zip(f, ab, u_inv)]
    lo = [y * a % n * a % n * u % n for y, a, u in zip(g, t, u_inv)]
    return lo, hi


def expected_modexp_var_sq(n2, xs, es, mul_into=None):
    """xs, es: [nbases][count]."""
    out = []
    for i in range(len(xs[0])):
        v = 1 if mul_into is None else mul_into[i]
        for j in range(len(xs)):
            v = v * pow(xs[j][i], es[j][i], n2) % n2
        out.append(v)
    return out


def expected_dgk_step4(n, g, l, beta, d, alpha, alpha_tilde, rsmall, delta_a):
    """[l + 1][count] by the oracle's step arithmetic (steps 4c .. 4h on unrandomized values); beta: [l][count]."""
    from oracle import sc_oracle as o

    dgk = o.DGKKey(n, g, 1, 0, 0)
    count = len(d)
    out = [[None] * count for _ in range(l + 1)]
    for c in range(count):
        a_bits, at_bits = o.to_bits(alpha[c] % (1 << l), l), o.to_bits(alpha_tilde[c] % (1 << l), l)
        d2 = dgk.enc_raw(0) if rsmall[c] else d[c]
        b_enc = [beta[i][c] for i in range(l)]
        xor = o.step_4d(a_bits, b_enc, dgk)
        w = [x if a == at else dgk.add(x, dgk.neg(d2)) for a, at, x in zip(a_bits, at_bits, xor)]
        w = o.step_4f(w, dgk)
        res = o.step_4h(1 - 2 * delta_a[c], a_bits, at_bits, d2, b_enc, w, delta_a[c], dgk)
        for i in range(l + 1):
            out[i][c] = res[i]
    return out


# ---- sc_modinv across SC_INV_TOP -----------------------------------------------------------------------------------------------------
INV_TOP = 2048
INV_COUNTS = (INV_TOP - 1, INV_TOP, INV_TOP + 1, 2 * INV_TOP + 1)
# (factor, cofactor): the modulus is their product -- composite with a known factor, so that the factor itself is a residue without an
# inverse; one small configuration ((2,18)) and one large ((8,27))
NOT_INVERTIBLE = ((make_modulus(64, "rand"), make_modulus(512, "rand")), (make_modulus(64, "rand"), make_modulus(4160, "rand")))

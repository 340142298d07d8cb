"""Batched secure inner product of Paillier ciphertexts, and what follows from it: sums of squares and squared Euclidean distances.

One round trip (semi-honest like the multiplication's §8e), for k pairs ([[x_j]], [[y_j]]) per row:

1. Alice draws an independent mask per field, r_a_j < 2^(wx + kappa) and r_b_j < 2^(wy + kappa), and rho_p_m in [1, N) per message.
   With a_j = r_a_j + ox, b_j = r_b_j + oy (the offsets are 2^(w - 1) for signed operands, else 0) the blinded pair is A_j = x_j + a_j
   (sa bits), B_j = y_j + b_j (sb bits).  g pairs fit one Paillier message; a row takes M = ceil(k / g) messages, pair j in message
   j mod M at position j div M.
2. Bob decrypts the M messages of a row, adds the products under the blinding, D = sum_j A_j B_j, and returns ONE fresh [[D]] per row.
3. Alice unblinds: [[sum_j x_j y_j]] = [[D]] T^-1, T = prod_j [[x_j]]^(b_j) [[y_j]]^(a_j) (1 + S N), S = sum_j a_j b_j.

Square mode computes [[sum_j x_j^2]] with one field per value: D = sum_j A_j^2, T = prod_j [[x_j]]^(2 a_j) (1 + S N), S = sum_j a_j^2.

Everything stays on the device; each step is one scheme-level library call (include/sc_amd.h: sc_initiator_dot_pack, sc_keyholder_dot,
sc_initiator_dot_finish), the same calls a C host makes.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .exchange import announce, answer, no_chunks, receive_announced
from .multiplication import MAX_WIDTH
from .schemes import Paillier

MAX_K = 1024        # pairs per row (csrc/sc_vm.h DOT_MAX_K)


@dataclass(frozen=True)
class DotLayout:
    """Layout of the packed plaintexts of an inner product of k pairs of widths (wx, wy) under a key of nbits bits: a pair takes
    pb = sa + sb bits (sa = wx + kappa + 1, sb = wy + kappa + 1; square mode: the one field, sb = 0 and wy = 0), g pairs fit a message
    and a row takes M messages.  Raises ValueError when a quantity is out of range, when not even one pair fits (g < 1) or when the sum
    of k products would not stay below N (dot_layout in csrc/sc_families.hip is the library's copy of the rule)."""

    kappa: int
    wx: int
    wy: int
    k: int
    signed: bool = False
    square: bool = False
    nbits: int = 2048

    def __post_init__(self) -> None:
        object.__setattr__(self, "signed", bool(self.signed))
        object.__setattr__(self, "square", bool(self.square))
        for name in ("kappa", "wx", "wy", "k", "nbits"):
            object.__setattr__(self, name, int(getattr(self, name)))
        if self.square:
            object.__setattr__(self, "wy", 0)
        if not 1 <= self.kappa <= 62:
            raise ValueError(f"kappa = {self.kappa}: expected 1 <= kappa <= 62")
        if not 1 <= self.wx <= MAX_WIDTH:
            raise ValueError(f"wx = {self.wx}: expected 1 .. {MAX_WIDTH}")
        if not self.square and not 1 <= self.wy <= MAX_WIDTH:
            raise ValueError(f"wy = {self.wy}: expected 1 .. {MAX_WIDTH}")
        if not 1 <= self.k <= MAX_K:
            raise ValueError(f"k = {self.k}: expected 1 .. {MAX_K} pairs per row")
        if self.g < 1:
            raise ValueError(f"pb = {self.pb}: one pair does not fit below a {self.nbits}-bit N (kappa = {self.kappa})")
        prod, lg = (2 * self.sa if self.square else self.pb), (self.k - 1).bit_length()
        if prod + lg >= self.nbits - 1:
            raise ValueError(f"the sum of k = {self.k} products ({prod} + {lg} bits) does not fit below a {self.nbits}-bit N")

    @property
    def sa(self) -> int:
        return self.wx + self.kappa + 1

    @property
    def sb(self) -> int:
        return 0 if self.square else self.wy + self.kappa + 1

    @property
    def pb(self) -> int:
        return self.sa + self.sb

    @property
    def g(self) -> int:
        """Pairs per message: the largest integer with g pb < bits(N) - 1."""
        return max(0, self.nbits - 2) // self.pb

    @property
    def M(self) -> int:
        """Messages per row."""
        return -(-self.k // self.g)

    def position(self, j: int) -> tuple[int, int]:
        """(message, position) of pair j: A_j sits at bits [t pb, t pb + sa) of message m, B_j above it."""
        if not 0 <= j < self.k:
            raise ValueError(f"pair {j}: expected 0 .. {self.k - 1}")
        return j % self.M, j // self.M

    @property
    def ebits(self) -> int:
        """Bits of the exponents of T: b_j < 2^sb and a_j < 2^sa; 2 a_j < 2^(sa + 1) for a square."""
        return self.sa + 1 if self.square else max(self.sa, self.sb)

    @property
    def header(self) -> list[int]:
        """What `dot_1_batch_{tag}` announces: kappa, wx, wy, signed, square, k."""
        return [self.kappa, self.wx, self.wy, int(self.signed), int(self.square), self.k]


@dataclass
class DotDraws:
    """The random inputs of one inner-product batch: Alice's r_a [k][B][aw] (< 2^(wx + kappa)), r_b [k][B][bw] (< 2^(wy + kappa); None
    for a square) and rho_p [M][B][nw] (the messages' randomizers); Bob's rho_d [B][nw].  Either side None."""

    r_a: torch.Tensor | None
    r_b: torch.Tensor | None
    rho_p: torch.Tensor | None
    rho_d: torch.Tensor | None


def draw_dot(count: int, layout: DotLayout, paillier: Paillier, source: str = "device", generator=None, alice: bool = True,
             bob: bool = True) -> DotDraws:
    """Both players' (or one player's) draws for `count` rows.  Alice, three generator calls: r_a as k count items of wx + kappa bits,
    element-major (pair j of row b is item j count + b); r_b likewise (no such call for a square); rho_p as M count items in [1, N),
    message-major.  Bob, one call: count bases in [1, N).  No two fields share a mask."""
    from .randomness import random_bits, uniform_below

    e, n = paillier.engine, paillier.public_key.n
    k, M = layout.k, layout.M
    r_a = r_b = rho_p = rho_d = None
    if alice:
        r_a = random_bits(layout.wx + layout.kappa, (k * count,), e, source, generator).reshape(k, count, -1)
        if not layout.square:
            r_b = random_bits(layout.wy + layout.kappa, (k * count,), e, source, generator).reshape(k, count, -1)
        rho_p = uniform_below(n, M * count, e, source, generator, nonzero=True).reshape(M, count, -1)
    if bob:
        rho_d = uniform_below(n, count, e, source, generator, nonzero=True)
    return DotDraws(r_a=r_a, r_b=r_b, rho_p=rho_p, rho_d=rho_d)


# ---- the three steps --------------------------------------------------------------------------------------------------------------
def _planes(layout: DotLayout, x_enc: torch.Tensor, y_enc: torch.Tensor | None):
    if x_enc.dim() != 3 or x_enc.shape[0] != layout.k:
        raise ValueError(f"x_enc: expected [{layout.k}][B][words]")
    if layout.square:
        return x_enc.contiguous(), None
    if y_enc is None or y_enc.shape != x_enc.shape:
        raise ValueError(f"y_enc: expected the shape of x_enc, [{layout.k}][{x_enc.shape[1]}][words]")
    return x_enc.contiguous(), y_enc.contiguous()


def dot_pack(layout: DotLayout, x_enc: torch.Tensor, y_enc: torch.Tensor | None, draws: DotDraws, paillier: Paillier):
    """Alice, step 1: P [M][B][2nw] from [[x_j]], [[y_j]] [k][B][2nw]; returns (P, (e, S)) -- the latter is what dot_finish needs
    (sc_initiator_dot_pack)."""
    x, y = _planes(layout, x_enc, y_enc)
    ew = (layout.ebits + 31) // 32
    P, e, S = paillier.engine.initiator_dot_pack(paillier.key, layout.kappa, layout.wx, layout.wy, layout.signed, layout.square, layout.k,
                                                 layout.M, x, y, draws.r_a, draws.r_b, draws.rho_p, ew)
    return P, (e, S)


def dot_sum(layout: DotLayout, P: torch.Tensor, paillier: Paillier, rho_d: torch.Tensor) -> torch.Tensor:
    """Bob, step 2: the CRT decryption of the M B messages, D = sum_j A_j B_j per row, encrypted and freshly randomized: [B][2nw]
    (sc_keyholder_dot).  ValueError when a decrypted message does not fit the announced layout."""
    return paillier.engine.keyholder_dot(paillier.key, layout.kappa, layout.wx, layout.wy, layout.square, layout.k, layout.M, P.contiguous(),
                                         rho_d.contiguous())


def dot_finish(layout: DotLayout, x_enc: torch.Tensor, y_enc: torch.Tensor | None, d_enc: torch.Tensor, plain, paillier: Paillier,
               base: torch.Tensor | None = None, coef: int = 1) -> torch.Tensor:
    """Alice, step 3: base [[sum_j x_j y_j]]^coef [B][2nw] from Bob's [[D]] (sc_initiator_dot_finish): one inversion, one launch."""
    x, y = _planes(layout, x_enc, y_enc)
    e, S = plain
    return paillier.engine.initiator_dot_finish(paillier.key, layout.kappa, layout.wx, layout.wy, layout.square, layout.k, x, y,
                                                d_enc.contiguous(), e, S, None if base is None else base.contiguous(), coef)


def dot_batch(layout: DotLayout, x_enc: torch.Tensor, y_enc: torch.Tensor | None, alice_paillier: Paillier, bob_paillier: Paillier,
              draws: DotDraws, base: torch.Tensor | None = None, coef: int = 1) -> torch.Tensor:
    """Both players' halves of one inner-product batch in one process: base [[sum_j x_j y_j]]^coef [B][2nw]."""
    P, plain = dot_pack(layout, x_enc, y_enc, draws, alice_paillier)
    d_enc = dot_sum(layout, P, bob_paillier, draws.rho_d)
    return dot_finish(layout, x_enc, y_enc, d_enc, plain, alice_paillier, base, coef)


# ---- inner product, sum of squares, squared distance ----------------------------------------------------------------------------------
def _layout(x_enc, x_bits, y_bits, signed, square, kappa, paillier: Paillier) -> DotLayout:
    if not isinstance(x_enc, torch.Tensor) or x_enc.dim() != 3:
        raise ValueError("x_enc: expected [k][B][words]")
    return DotLayout(kappa, int(x_bits), int(y_bits), x_enc.shape[0], signed, square, paillier.public_key.n.bit_length())


def secure_dot_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, x_bits: int, y_bits: int, alice_paillier: Paillier, bob_paillier: Paillier,
                     signed: bool = False, kappa: int = 40, draws: DotDraws | None = None) -> torch.Tensor:
    """[[sum_j x_j y_j]] for B rows of k pairs of Paillier ciphertexts under Bob's key: x_enc, y_enc [k][B][2nw] -> [B][2nw],
    1 <= k <= 1024.  Unsigned: 0 <= x_j < 2^x_bits; signed: -2^(x_bits - 1) <= x_j < 2^(x_bits - 1) as residues modulo N; likewise y."""
    layout = _layout(x_enc, x_bits, y_bits, signed, False, kappa, alice_paillier)          # the fit rule, before any launch
    draws = draws if draws is not None else draw_dot(x_enc.shape[1], layout, alice_paillier)
    return dot_batch(layout, x_enc, y_enc, alice_paillier, bob_paillier, draws)


def secure_sum_squares_batch(x_enc: torch.Tensor, x_bits: int, alice_paillier: Paillier, bob_paillier: Paillier, signed: bool = False,
                             kappa: int = 40, draws: DotDraws | None = None) -> torch.Tensor:
    """[[sum_j x_j^2]] for B rows of k ciphertexts: x_enc [k][B][2nw] -> [B][2nw].  Square mode: one field per value, so a message
    holds twice as many values as it holds pairs of a dot product."""
    layout = _layout(x_enc, x_bits, 0, signed, True, kappa, alice_paillier)
    draws = draws if draws is not None else draw_dot(x_enc.shape[1], layout, alice_paillier)
    return dot_batch(layout, x_enc, None, alice_paillier, bob_paillier, draws)


def _differences(x_enc: torch.Tensor, y_enc: torch.Tensor, paillier: Paillier) -> torch.Tensor:
    """[[x_j - y_j]] [k][B][2nw]: one inversion pass and one product over the k B flat items."""
    if x_enc.dim() != 3 or y_enc.shape != x_enc.shape:
        raise ValueError("x_enc, y_enc: expected two [k][B][words] arrays of one shape")
    flat = (x_enc.shape[0] * x_enc.shape[1], x_enc.shape[2])
    d = paillier.add_batch(x_enc.contiguous().reshape(flat), paillier.neg_batch(y_enc.contiguous().reshape(flat)))
    return d.reshape(x_enc.shape)


def secure_squared_distance_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, bits: int, alice_paillier: Paillier, bob_paillier: Paillier,
                                  kappa: int = 40, draws: DotDraws | None = None) -> torch.Tensor:
    """[[sum_j (x_j - y_j)^2]] for B rows, 0 <= x_j, y_j < 2^bits: the differences [[x_j - y_j]] are signed values of bits + 1 bits,
    then square mode.  x_enc, y_enc [k][B][2nw] -> [B][2nw]."""
    layout = _layout(x_enc, int(bits) + 1, 0, True, True, kappa, alice_paillier)
    d = _differences(x_enc, y_enc, alice_paillier)
    draws = draws if draws is not None else draw_dot(x_enc.shape[1], layout, alice_paillier)
    return dot_batch(layout, d, None, alice_paillier, bob_paillier, draws)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_dot_batch) -------------------------------------------
# the announced exchange of exchange.py under the name `dot`: the header is DotLayout.header, exactly 6 entries, P is [M][B][2nw] and the
# answer the key holder's one [[D]] per row.
async def alice_dot(ini, x_enc, y_enc, x_bits, y_bits, signed, square, kappa, draws, source, engine, generator, chunks):
    no_chunks(chunks)
    if not isinstance(x_enc, torch.Tensor) or x_enc.dim() != 3:
        raise ValueError("x_enc: expected [k][B][words]")
    sid = await ini._open_batch_session(x_enc[0], x_enc[0] if square else y_enc[0], engine)
    pai, count = ini.scheme_paillier, x_enc.shape[1]
    layout = _layout(x_enc, x_bits, 0 if square else y_bits, signed, square, kappa, pai)
    draws = draws if draws is not None else draw_dot(count, layout, pai, source, generator, bob=False)
    P, plain = dot_pack(layout, x_enc, None if square else y_enc, draws, pai)
    d_enc = await announce(ini, "dot", f"session_{sid}", layout.header, P, (count,), "[[D]]")
    return dot_finish(layout, x_enc, None if square else y_enc, d_enc, plain, pai)


async def bob_dot(kh, k, x_bits, y_bits, signed, square, kappa, draws, source, generator, count=None):
    sid = await kh._open_batch_session()
    pai, tag = kh.scheme_paillier, f"session_{sid}"
    layout = DotLayout(kappa, int(x_bits), 0 if square else int(y_bits), int(k), signed, square, pai.public_key.n.bit_length())
    P, count = await receive_announced(kh, "dot", tag, layout.header, "(kappa, wx, wy, signed, square, k)", range(6, 7), (layout.M,), count)
    rho = draws.rho_d if draws is not None else draw_dot(count, layout, pai, source, generator, alice=False).rho_d
    await answer(kh, "dot", tag, dot_sum(layout, P, pai, rho))

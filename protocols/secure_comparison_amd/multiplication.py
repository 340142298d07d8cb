"""Batched secure multiplication of Paillier ciphertexts, and what follows from it: AND / OR / XOR of encrypted bits, equality and
interval membership on top of the comparison.

One round trip (semi-honest like the selection's §8b), for [[x]] and up to four columns [[y_j]] per row:

1. Alice draws r_a < 2^(wx + kappa), r_b_j < 2^(wy_j + kappa), rho_p in [1, N); with e_y = r_a + ox and e_x_j = r_b_j + oy_j (the
   offsets are 2^(w - 1) for signed operands, else 0) she packs P = [[x]] prod_j [[y_j]]^(2^off_j) (1 + R N) rho_p^N,
   R = e_y + sum_j 2^off_j e_x_j: plaintext A + sum_j 2^off_j B_j, A = x + e_y < 2^s, B_j = y_j + e_x_j < 2^fbits_j.
2. Bob decrypts P once, splits the fields and returns fresh encryptions [[A B_j]].
3. Alice unblinds: [[x y_j]] = [[A B_j]] T_j^-1 with T_j = [[x]]^(e_x_j) [[y_j]]^(e_y) (1 + e_x_j e_y N).

Everything stays on the device; each step is one scheme-level library call (include/sc_amd.h: sc_initiator_mul_pack,
sc_keyholder_mul, sc_initiator_mul_finish), the same calls a C host makes.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .batch import secure_comparison_batch
from .exchange import announce, answer, no_chunks, receive_announced
from .flags import check_l
from .schemes import DGK, Paillier
from .selection import MAX_FIELDS, _comparison_draws

MAX_WIDTH = 255     # bits of one operand (csrc/sc_vm.h MUL_MAX_WIDTH)


@dataclass(frozen=True)
class MulLayout:
    """Field layout of the packed plaintext of P for x of wx bits and columns y_j of wy[j] bits under a key of nbits bits:
    A = x + e_y in [0, s), s = wx + kappa + 1, then B_j = y_j + e_x_j in fbits_j = wy[j] + kappa + 1 bits.  Raises ValueError when
    s + sum_j fbits_j or one s + fbits_j reaches bits(N) - 1 (mul_layout in csrc/sc_families.hip is the library's copy of the rule)."""

    kappa: int
    wx: int
    wy: tuple
    signed: bool = False
    nbits: int = 2048

    def __post_init__(self) -> None:
        wy = (self.wy,) if isinstance(self.wy, int) else self.wy
        object.__setattr__(self, "wy", tuple(int(w) for w in wy))
        object.__setattr__(self, "signed", bool(self.signed))
        if not 1 <= self.kappa <= 62:
            raise ValueError(f"kappa = {self.kappa}: expected 1 <= kappa <= 62")
        if not 1 <= self.wx <= MAX_WIDTH:
            raise ValueError(f"wx = {self.wx}: expected 1 .. {MAX_WIDTH}")
        if not 1 <= len(self.wy) <= MAX_FIELDS:
            raise ValueError(f"{len(self.wy)} columns: expected 1 .. {MAX_FIELDS}")
        off = self.s
        for j, w in enumerate(self.wy):
            if not 1 <= w <= MAX_WIDTH:
                raise ValueError(f"column {j}: width {w}: expected 1 .. {MAX_WIDTH}")
            f = w + self.kappa + 1
            if self.s + f >= self.nbits - 1:
                raise ValueError(f"column {j}: the product A * B ({self.s + f} bits) does not fit below a {self.nbits}-bit N")
            off += f
            if off >= self.nbits - 1:
                raise ValueError(f"column {j}: the packed fields ({off} bits) do not fit below a {self.nbits}-bit N (kappa = {self.kappa})")

    @property
    def s(self) -> int:
        return self.wx + self.kappa + 1

    @property
    def fbits(self) -> list[int]:
        return [w + self.kappa + 1 for w in self.wy]

    @property
    def offsets(self) -> list[int]:
        off, out = self.s, []
        for f in self.fbits:
            out.append(off)
            off += f
        return out

    @property
    def end(self) -> int:
        return self.s + sum(self.fbits)

    @property
    def ebits(self) -> int:
        """Bits of the exponents of T: e_y < 2^s, e_x_j < 2^fbits_j."""
        return max(self.s, *self.fbits)

    @property
    def header(self) -> list[int]:
        """What `mul_1_batch_{tag}` announces: kappa, wx, signed, the number of columns, their widths."""
        return [self.kappa, self.wx, int(self.signed), len(self.wy), *self.wy]


@dataclass
class MulDraws:
    """The random inputs of one multiplication batch: Alice's r_a [B][aw] (< 2^(wx + kappa)), r_b [nf][B][bw] (column j
    < 2^(wy_j + kappa)) and rho_p [B][nw] (P's randomizer); Bob's rho_products [nf][B][nw].  Either side None."""

    r_a: torch.Tensor | None
    r_b: torch.Tensor | None
    rho_p: torch.Tensor | None
    rho_products: torch.Tensor | None


def draw_mul(count: int, layout: MulLayout, paillier: Paillier, source: str = "device", generator=None, alice: bool = True,
             bob: bool = True) -> MulDraws:
    """Both players' (or one player's) multiplication draws for `count` rows, on the device or from a seeded torch generator."""
    from .randomness import random_bits, random_columns, uniform_below

    e, n = paillier.engine, paillier.public_key.n
    nf = len(layout.wy)
    r_a = r_b = rho_p = rho_q = None
    if alice:
        r_a = random_bits(layout.wx + layout.kappa, (count,), e, source, generator)
        r_b = random_columns([w + layout.kappa for w in layout.wy], (max(layout.wy) + layout.kappa + 31) // 32, count, e, source, generator)
        rho_p = uniform_below(n, count, e, source, generator, nonzero=True)
    if bob:
        rho_q = uniform_below(n, nf * count, e, source, generator, nonzero=True).reshape(nf, count, -1)
    return MulDraws(r_a=r_a, r_b=r_b, rho_p=rho_p, rho_products=rho_q)


# ---- the three steps --------------------------------------------------------------------------------------------------------------
def _columns(layout: MulLayout, x_enc: torch.Tensor, y_enc: torch.Tensor) -> torch.Tensor:
    """y_enc as [nf][B][2nw]: a [B][2nw] array (x_enc itself for a square) is one column."""
    y = y_enc.unsqueeze(0) if y_enc.dim() == 2 else y_enc
    nf, count = len(layout.wy), x_enc.shape[0]
    if y.dim() != 3 or y.shape[0] != nf or y.shape[1] != count:
        raise ValueError(f"y_enc: expected [{nf}][{count}][words]")
    return y.contiguous()


def mul_pack(layout: MulLayout, x_enc: torch.Tensor, y_enc: torch.Tensor, draws: MulDraws, paillier: Paillier):
    """Alice, step 1: P [B][2nw] from [[x]] [B][2nw] and [[y_j]] [nf][B][2nw]; returns (P, (e, rab)) -- the latter is what mul_finish
    needs (sc_initiator_mul_pack)."""
    ew = (layout.ebits + 31) // 32
    P, e, rab = paillier.engine.initiator_mul_pack(paillier.key, layout.kappa, layout.wx, layout.wy, layout.signed, x_enc,
                                                   _columns(layout, x_enc, y_enc), draws.r_a, draws.r_b, draws.rho_p, ew)
    return P, (e, rab)


def mul_mult(layout: MulLayout, P: torch.Tensor, paillier: Paillier, rho_products: torch.Tensor) -> torch.Tensor:
    """Bob, step 2: one CRT decryption of P, the field products A * B_j, encrypted and freshly randomized: [nf][B][2nw]
    (sc_keyholder_mul).  ValueError when a decrypted row does not fit the announced layout."""
    return paillier.engine.keyholder_mul(paillier.key, layout.kappa, layout.wx, layout.wy, P, rho_products.contiguous())


def mul_finish(layout: MulLayout, x_enc: torch.Tensor, y_enc: torch.Tensor, products: torch.Tensor, plain, paillier: Paillier,
               base: torch.Tensor | None = None, coef: int = 1) -> torch.Tensor:
    """Alice, step 3: base_j [[x y_j]]^coef [nf][B][2nw] from Bob's products (sc_initiator_mul_finish): one inversion, one launch."""
    e, rab = plain
    return paillier.engine.initiator_mul_finish(paillier.key, layout.kappa, layout.wx, layout.wy, x_enc, _columns(layout, x_enc, y_enc),
                                                products.contiguous(), e, rab, None if base is None else base.contiguous(), coef)


def mul_batch(layout: MulLayout, x_enc: torch.Tensor, y_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier,
              draws: MulDraws, base: torch.Tensor | None = None, coef: int = 1) -> torch.Tensor:
    """Both players' halves of one multiplication batch in one process: base_j [[x y_j]]^coef [nf][B][2nw]."""
    P, plain = mul_pack(layout, x_enc, y_enc, draws, alice_paillier)
    products = mul_mult(layout, P, bob_paillier, draws.rho_products)
    return mul_finish(layout, x_enc, y_enc, products, plain, alice_paillier, base, coef)


# ---- products, Boolean operations ---------------------------------------------------------------------------------------------------
def _layout(x_bits, y_bits, signed, kappa, paillier: Paillier) -> MulLayout:
    return MulLayout(kappa, int(x_bits), y_bits, signed, paillier.public_key.n.bit_length())


def secure_multiply_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, x_bits: int, y_bits, alice_paillier: Paillier,
                          bob_paillier: Paillier, signed: bool = False, kappa: int = 40, draws: MulDraws | None = None) -> torch.Tensor:
    """[[x y_j]] for B rows of Paillier ciphertexts under Bob's key: x_enc [B][2nw], y_enc [nf][B][2nw] with y_bits a sequence of nf
    widths -> [nf][B][2nw]; or y_enc [B][2nw] with y_bits one width -> [B][2nw] (y_enc may be x_enc itself: a square).  Unsigned:
    0 <= x < 2^x_bits; signed: -2^(x_bits - 1) <= x < 2^(x_bits - 1) as residues modulo N; likewise every column."""
    layout = _layout(x_bits, y_bits, signed, kappa, alice_paillier)          # the fit rule, before any launch
    draws = draws if draws is not None else draw_mul(x_enc.shape[0], layout, alice_paillier)
    out = mul_batch(layout, x_enc, y_enc, alice_paillier, bob_paillier, draws)
    return out[0] if y_enc.dim() == 2 else out


def _bit_op(a_enc, b_enc, ap, bp, kappa, draws, coef):
    layout = _layout(1, (1,), False, kappa, ap)
    draws = draws if draws is not None else draw_mul(a_enc.shape[0], layout, ap)
    base = None if coef == 1 else ap.add_batch(a_enc, b_enc).unsqueeze(0)                # [[a + b]]
    return mul_batch(layout, a_enc, b_enc, ap, bp, draws, base, coef)[0]


def secure_and_batch(a_enc: torch.Tensor, b_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier, kappa: int = 40,
                     draws: MulDraws | None = None) -> torch.Tensor:
    """[[a AND b]] = [[a b]] for encrypted bits a, b in {0, 1}: [B][2nw]."""
    return _bit_op(a_enc, b_enc, alice_paillier, bob_paillier, kappa, draws, 1)


def secure_or_batch(a_enc: torch.Tensor, b_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier, kappa: int = 40,
                    draws: MulDraws | None = None) -> torch.Tensor:
    """[[a OR b]] = [[a + b - a b]]: the finish multiplies [[a]] [[b]] by [[a b]]^-1 in its one launch (no second inversion)."""
    return _bit_op(a_enc, b_enc, alice_paillier, bob_paillier, kappa, draws, -1)


def secure_xor_batch(a_enc: torch.Tensor, b_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier, kappa: int = 40,
                     draws: MulDraws | None = None) -> torch.Tensor:
    """[[a XOR b]] = [[a + b - 2 a b]]."""
    return _bit_op(a_enc, b_enc, alice_paillier, bob_paillier, kappa, draws, -2)


# ---- equality and interval membership: two comparisons in ONE batch of 2B rows, then one AND ------------------------------------------
def _two_comparisons(lo_enc, hi_enc, l, ap, ad, bp, bd, draws):
    """[[lo_i <= hi_i]] for the 2B stacked rows, with independent draws per row."""
    check_l(l)
    draws = draws if draws is not None else _comparison_draws(lo_enc.shape[0], l, ap, ad, bp, bd)
    return secure_comparison_batch(lo_enc, hi_enc, l, ap, ad, bp, bd, draws)


def secure_equal_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK,
                       bob_paillier: Paillier, bob_dgk: DGK, draws=None, mul_draws: MulDraws | None = None, kappa: int = 40):
    """([[x == y]], [[x <= y]], [[y <= x]]) for B pairs [B][2nw], 0 <= x, y < 2^l: one comparison batch of 2B rows -- (x, y) stacked
    on (y, x); `draws` is a batch.BatchDraws for 2B rows -- then [[x == y]] = [[x <= y]] AND [[y <= x]]."""
    B = x_enc.shape[0]
    _layout(1, (1,), False, kappa, alice_paillier)
    d = _two_comparisons(torch.cat([x_enc, y_enc]), torch.cat([y_enc, x_enc]), l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, draws)
    le, ge = d[:B].contiguous(), d[B:].contiguous()
    return secure_and_batch(le, ge, alice_paillier, bob_paillier, kappa, mul_draws), le, ge


def secure_in_range_batch(x_enc: torch.Tensor, lo_enc: torch.Tensor, hi_enc: torch.Tensor, l: int, alice_paillier: Paillier,
                          alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK, draws=None, mul_draws: MulDraws | None = None,
                          kappa: int = 40) -> torch.Tensor:
    """[[lo <= x <= hi]] for B rows, all values in [0, 2^l): one comparison batch of 2B rows -- (lo, x) stacked on (x, hi) -- then
    one AND."""
    B = x_enc.shape[0]
    _layout(1, (1,), False, kappa, alice_paillier)
    d = _two_comparisons(torch.cat([lo_enc, x_enc]), torch.cat([x_enc, hi_enc]), l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, draws)
    return secure_and_batch(d[:B].contiguous(), d[B:].contiguous(), alice_paillier, bob_paillier, kappa, mul_draws)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{multiply,equal}_batch) -------------------------------
# the announced exchange of exchange.py under the name `mul`: the header is MulLayout.header (more than 4 + MAX_FIELDS entries are
# malformed), the answer the key holder's products.
async def _alice_mul(ini, tag, layout, x_enc, y_enc, draws, source, generator):
    pai, count = ini.scheme_paillier, x_enc.shape[0]
    draws = draws if draws is not None else draw_mul(count, layout, pai, source, generator, bob=False)
    P, plain = mul_pack(layout, x_enc, y_enc, draws, pai)
    prods = await announce(ini, "mul", tag, layout.header, P, (len(layout.wy), count), "[[A B_j]]")
    return mul_finish(layout, x_enc, y_enc, prods, plain, pai)


async def _bob_mul(kh, tag, layout, count, draws, source, generator):
    """The key holder's half of one multiplication exchange: the layout check, then his products.  count None: P's own."""
    pai = kh.scheme_paillier
    P, count = await receive_announced(kh, "mul", tag, layout.header, "(kappa, wx, signed, columns, widths)", range(5 + MAX_FIELDS), (), count)
    rho = draws.rho_products if draws is not None else draw_mul(count, layout, pai, source, generator, alice=False).rho_products
    await answer(kh, "mul", tag, mul_mult(layout, P, pai, rho))


async def alice_multiply(ini, x_enc, y_enc, x_bits, y_bits, signed, kappa, draws, source, engine, generator, chunks):
    no_chunks(chunks)
    y = y_enc if y_enc.dim() == 2 else y_enc[0]
    sid = await ini._open_batch_session(x_enc, y, engine)
    layout = _layout(x_bits, y_bits, signed, kappa, ini.scheme_paillier)
    out = await _alice_mul(ini, f"session_{sid}", layout, x_enc, y_enc, draws, source, generator)
    return out[0] if y_enc.dim() == 2 else out


async def bob_multiply(kh, x_bits, y_bits, signed, kappa, draws, source, generator, count=None):
    sid = await kh._open_batch_session()
    await _bob_mul(kh, f"session_{sid}", _layout(x_bits, y_bits, signed, kappa, kh.scheme_paillier), count, draws, source, generator)


async def alice_equal(ini, x_enc, y_enc, draws, mul_draws, kappa, source, engine, generator, chunks):
    no_chunks(chunks)
    sid = await ini._open_batch_session(x_enc, y_enc, engine)
    pai, B, tag = ini.scheme_paillier, x_enc.shape[0], f"session_{sid}"
    layout = _layout(1, (1,), False, kappa, pai)
    d = await ini._batch_session(tag, torch.cat([x_enc, y_enc]), torch.cat([y_enc, x_enc]), draws, source, generator, None)
    le, ge = d[:B].contiguous(), d[B:].contiguous()
    eq = await _alice_mul(ini, tag, layout, le, ge, mul_draws, source, generator)
    return eq[0], le, ge


async def bob_equal(kh, draws, mul_draws, kappa, source, generator):
    sid = await kh._open_batch_session()
    tag = f"session_{sid}"
    layout = _layout(1, (1,), False, kappa, kh.scheme_paillier)
    count = await kh._batch_session(tag, None, draws, source, generator)
    if count % 2:
        raise ValueError(f"equal: the comparison session has {count} rows, expected the 2B rows of (x, y) stacked on (y, x)")
    await _bob_mul(kh, tag, layout, count // 2, mul_draws, source, generator)

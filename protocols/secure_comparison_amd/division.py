"""Batched secure division and modulo of Paillier ciphertexts by PUBLIC divisors: exact floor division, no +-1 error.

The comparison [[x <= y]] = (z div 2^l) - (r div 2^l) - [[z mod 2^l < r mod 2^l]] is a division by 2^l; this is the same identity for an
arbitrary public divisor d per row, 1 <= d < 2^64 (semi-honest like the rest).  For [[x]], 0 <= x < 2^x_bits:

1. Alice draws r < 2^(x_bits + kappa), sends [[z]] = [[x + r]] rho^N and keeps rq = r div d, rm = r mod d.
2. Bob decrypts z and computes zq = z div d, zm = z mod d.
3. Both run the comparison's DGK sub-comparison (steps 4a-4j, 5, 6, 7) on planted plaintexts -- beta = zm, alpha = alpha~ = rm, the bit d = 1,
   r_small = 1, zeta_1 = zeta_2 = zq, r_shift = rq -- at l = max(1, bits(max d - 1)); step 7 then yields
   [[x div d]] = [[zq]] ([[rq]] [[zm < rm]])^-1.

Signed input (-2^x_bits <= x < 2^x_bits) is offset by c d, c = ceil(2^x_bits / d), and c is taken from the quotient again: Python's //, which
floors toward minus infinity.  The modulo is [[x]] ([[x div d]]^d)^-1, in [0, d) for signed input too.  The long divisions of r and z run on
the device (k_divmod_words behind sc_initiator_div_blind / sc_keyholder_div_open, include/sc_amd.h), the rest are the calls the comparison
makes.  Out of scope: encrypted divisors, divisors of 2^64 and above, rounding modes other than floor.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .exchange import announce, answer, no_chunks, receive_announced
from .initiator import AlicePlain, Initiator
from .keyholder import BobPlain, KeyHolder
from .limbs import ints_to_words
from .schemes import DGK, Paillier

MAX_DIVISOR = (1 << 64) - 1


def div_width(x_bits: int, signed: bool) -> int:
    """Bits of the dividend that is blinded: x itself, or for signed input x + c d, which is below 2^(x_bits + 2) where d <= 2^x_bits and
    below 2 d < 2^65 elsewhere."""
    return max(x_bits + 2, 65) if signed else x_bits


def div_fits(nbits: int, kappa: int, x_bits: int, signed: bool = False) -> bool:
    """The fit rule (sc_div_fits in csrc/sc_schemes.hip is the library's copy): width + kappa + 2 < bits(N) - 1, so that z = x + r never
    wraps around N and stays below (N - 1) / 2 -- which is why the planted bit d = 1 and r_small = 1 are honest."""
    if not (1 <= kappa <= 62 and x_bits >= 1):
        return False
    return div_width(x_bits, signed) + kappa + 2 < nbits - 1


def divisors_of(divisor, count: int) -> tuple:
    """`divisor` -- a Python int, or a CPU int64 / uint64 tensor or a list of [count] -- as a tuple of `count` Python ints in [1, 2^64)."""
    if isinstance(divisor, torch.Tensor):
        if divisor.device.type != "cpu" or divisor.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
            raise ValueError("divisor: expected a Python int, a list, or a CPU int64 / uint64 tensor (divisors are public)")
        divisor = [int(v) for v in divisor.reshape(-1).tolist()]
    if isinstance(divisor, int) and not isinstance(divisor, bool):
        ds = (divisor,) * count
    else:
        ds = tuple(int(v) for v in divisor)
        if len(ds) != count:
            raise ValueError(f"divisor: {len(ds)} divisors for {count} rows")
    for i, d in enumerate(ds):
        if not 1 <= d <= MAX_DIVISOR:
            raise ValueError(f"divisor: row {i}: {d}: expected 1 <= d < 2^64")
    return ds


@dataclass(frozen=True)
class DivLayout:
    """What both players derive from the public arguments of one division batch.  Raises ValueError where the fit rule or the DGK rule
    u > 2^(l + 2) refuses, before anything is drawn or sent."""

    kappa: int
    x_bits: int
    signed: bool
    nbits: int
    divisors: tuple
    u: int

    def __post_init__(self) -> None:
        object.__setattr__(self, "signed", bool(self.signed))
        if not 1 <= self.kappa <= 62:
            raise ValueError(f"kappa = {self.kappa}: expected 1 <= kappa <= 62")
        if self.x_bits < 1:
            raise ValueError(f"x_bits = {self.x_bits}: expected at least 1")
        if not div_fits(self.nbits, self.kappa, self.x_bits, self.signed):
            raise ValueError(f"division: x_bits = {self.x_bits} ({'signed' if self.signed else 'unsigned'}), kappa = {self.kappa}: the blinded "
                             f"dividend ({self.width + self.kappa + 2} bits) does not fit below a {self.nbits}-bit N")
        if self.u <= 1 << (self.l + 2):
            raise ValueError(f"division: divisors of up to {self.l} bits need a DGK key with u > 2^{self.l + 2}")

    @property
    def width(self) -> int:
        return div_width(self.x_bits, self.signed)

    @property
    def l(self) -> int:
        """Bits of the sub-comparison: the remainders are below max d."""
        return max(1, (max(self.divisors) - 1).bit_length())

    @property
    def rbits(self) -> int:
        return self.width + self.kappa

    @property
    def c(self) -> tuple:
        """Per row, the offset quotient c = ceil(2^x_bits / d) of signed input (0 for unsigned)."""
        return tuple(-(-(1 << self.x_bits) // d) if self.signed else 0 for d in self.divisors)

    @property
    def header(self) -> list[int]:
        """What `div_1_batch_{tag}` announces: kappa, x_bits, signed, l, the number of rows and a 31-bit digest of the divisors."""
        digest = 0
        for d in self.divisors:
            digest = (digest * 1000003 + d) % 0x7fffffff
        return [self.kappa, self.x_bits, int(self.signed), self.l, len(self.divisors), digest]


def _layout(count, divisor, x_bits, signed, kappa, paillier: Paillier, dgk: DGK) -> DivLayout:
    return DivLayout(int(kappa), int(x_bits), signed, paillier.public_key.n.bit_length(), divisors_of(divisor, count), dgk.public_key.u)


@dataclass
class DivDraws:
    """The random inputs of one division batch.  Alice's: r [B][nw] (< 2^(width + kappa), zero-extended to the words of N), rho_z [B][nw]
    ([[z]]'s randomizer) and her sub-comparison draws delta_a [B], rhos [l+1][B][ew], permutation [B][l+1], r_alice_dgk [l+1][B][er]; Bob's:
    r_bob_dgk [l+1][B][er] and rho3 [3B][nw] (the bases for [[zq]] twice and [[delta_B]]).  Either side None."""

    r: torch.Tensor | None = None
    rho_z: torch.Tensor | None = None
    delta_a: torch.Tensor | None = None
    rhos: torch.Tensor | None = None
    permutation: torch.Tensor | None = None
    r_alice_dgk: torch.Tensor | None = None
    r_bob_dgk: torch.Tensor | None = None
    rho3: torch.Tensor | None = None


def draw_div(count: int, layout: DivLayout, paillier: Paillier, dgk: DGK, source: str = "device", generator=None, alice: bool = True,
             bob: bool = True) -> DivDraws:
    """Both players' (or one player's) division draws for `count` rows, on the device or from a seeded torch generator."""
    from .randomness import random_bits, random_coins, random_permutations, uniform_below

    e, n, u, l = paillier.engine, paillier.public_key.n, dgk.public_key.u, layout.l
    d = DivDraws()
    if alice:
        r = random_bits(layout.rbits, (count,), e, source, generator)
        d.r = torch.nn.functional.pad(r, (0, paillier.mod_n.nwords - r.shape[-1])).contiguous()
        d.rho_z = uniform_below(n, count, e, source, generator, nonzero=True)
        d.delta_a = random_coins(count, e, source, generator)
        d.rhos = uniform_below(u, (l + 1) * count, e, source, generator, nonzero=True).reshape(l + 1, count, -1)
        d.permutation = random_permutations(count, l + 1, e, source, generator)
        d.r_alice_dgk = random_bits(dgk.randomizer_bits, (l + 1, count), e, source, generator)
    if bob:
        d.r_bob_dgk = random_bits(dgk.randomizer_bits, (l + 1, count), e, source, generator)
        d.rho3 = uniform_below(n, 3 * count, e, source, generator, nonzero=True)
    return d


# ---- the steps -------------------------------------------------------------------------------------------------------------------------
def _u64(values, engine) -> torch.Tensor:
    return engine.upload_u64(values)


def _words(values, nwords: int, engine) -> torch.Tensor:
    return engine.upload_words(ints_to_words(values, nwords))


def div_blind(layout: DivLayout, x_enc: torch.Tensor, draws: DivDraws, paillier: Paillier):
    """Alice, step 1: ([[z]] [B][2nw], her planted plaintext side of the sub-comparison) -- sc_initiator_div_blind, after the offset c d
    of signed input."""
    e, nw = paillier.engine, paillier.mod_n.nwords
    if layout.signed:
        x_enc = paillier.add_batch(x_enc, paillier.encrypt_raw_batch(_words([c * d for c, d in zip(layout.c, layout.divisors)], nw, e)))
    z_enc, rq, rm = e.initiator_div_blind(paillier.key, layout.kappa, layout.x_bits, layout.signed, x_enc, draws.r, draws.rho_z,
                                          _u64(layout.divisors, e))
    one = torch.ones_like(rm)
    return z_enc, AlicePlain(draws.r, rm, rm, one, rq)


def div_open(layout: DivLayout, z_enc: torch.Tensor, paillier: Paillier) -> BobPlain:
    """Bob, step 2: his planted plaintext side from z = Dec([[z]]) -- sc_keyholder_div_open."""
    e = paillier.engine
    zq, zm = e.keyholder_div_open(paillier.key, z_enc, _u64(layout.divisors, e))
    return BobPlain(None, zm, torch.ones_like(zm), zq, zq)


def div_finish(layout: DivLayout, q_enc: torch.Tensor, paillier: Paillier) -> torch.Tensor:
    """Alice, last: the offset quotient c of signed input taken from [[(x + c d) div d]] again."""
    if not layout.signed:
        return q_enc
    e, nw = paillier.engine, paillier.mod_n.nwords
    return paillier.add_batch(q_enc, paillier.encrypt_raw_neg_batch(_words(layout.c, nw, e)))


def mod_from_quotient(layout: DivLayout, x_enc: torch.Tensor, q_enc: torch.Tensor, paillier: Paillier) -> torch.Tensor:
    """[[x mod d]] = [[x]] ([[x div d]]^d)^-1: the per-row scalar multiplication and one inversion pass."""
    e = paillier.engine
    dq = paillier.scalar_mul_batch(q_enc, _words(layout.divisors, 2, e), 64)
    return paillier.add_batch(x_enc, paillier.neg_batch(dq))


def div_batch(layout: DivLayout, x_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier, alice_dgk: DGK, bob_dgk: DGK,
              draws: DivDraws) -> torch.Tensor:
    """Both players' halves of one division batch in one process: [[x div d]] [B][2nw]."""
    l = layout.l
    z_enc, a_plain = div_blind(layout, x_enc, draws, alice_paillier)
    b_plain = div_open(layout, z_enc, bob_paillier)
    d_enc, beta_enc = KeyHolder.step_4a_4b_batch(b_plain, l, bob_dgk, bob_paillier, draws.r_bob_dgk)
    c_sent, _ = Initiator.step_4_batch(d_enc, beta_enc, a_plain, draws.delta_a, alice_dgk, draws.rhos, draws.permutation, draws.r_alice_dgk)
    _, zeta_1, zeta_2, delta_b = KeyHolder.step_4j_5_batch(c_sent, b_plain, bob_paillier, bob_dgk, draws.rho3)
    q_enc = Initiator.step_6_7_batch(draws.delta_a, delta_b, zeta_1, zeta_2, a_plain, l, alice_paillier)
    return div_finish(layout, q_enc, alice_paillier)


def _prepare(x_enc, divisor, x_bits, ap, ad, signed, kappa, draws):
    layout = _layout(x_enc.shape[0], divisor, x_bits, signed, kappa, ap, ad)              # every refusal, before any launch
    return layout, (draws if draws is not None else draw_div(x_enc.shape[0], layout, ap, ad))


def secure_divide_batch(x_enc: torch.Tensor, divisor, x_bits: int, alice_paillier: Paillier, bob_paillier: Paillier, alice_dgk: DGK,
                        bob_dgk: DGK, signed: bool = False, kappa: int = 40, draws: DivDraws | None = None) -> torch.Tensor:
    """[[x // d]] for B rows of Paillier ciphertexts under Bob's key: x_enc [B][2nw]; divisor a Python int, or a CPU int64 / uint64 tensor
    or list of [B], 1 <= d < 2^64, public.  Unsigned: 0 <= x < 2^x_bits; signed: -2^x_bits <= x < 2^x_bits as residues modulo N, and the
    quotient floors toward minus infinity like Python's //."""
    layout, draws = _prepare(x_enc, divisor, x_bits, alice_paillier, alice_dgk, signed, kappa, draws)
    return div_batch(layout, x_enc, alice_paillier, bob_paillier, alice_dgk, bob_dgk, draws)


def secure_divmod_batch(x_enc: torch.Tensor, divisor, x_bits: int, alice_paillier: Paillier, bob_paillier: Paillier, alice_dgk: DGK,
                        bob_dgk: DGK, signed: bool = False, kappa: int = 40, draws: DivDraws | None = None):
    """([[x // d]], [[x % d]]) from ONE protocol run; the remainder is in [0, d) for signed input too."""
    layout, draws = _prepare(x_enc, divisor, x_bits, alice_paillier, alice_dgk, signed, kappa, draws)
    q_enc = div_batch(layout, x_enc, alice_paillier, bob_paillier, alice_dgk, bob_dgk, draws)
    return q_enc, mod_from_quotient(layout, x_enc, q_enc, alice_paillier)


def secure_modulo_batch(x_enc: torch.Tensor, divisor, x_bits: int, alice_paillier: Paillier, bob_paillier: Paillier, alice_dgk: DGK,
                        bob_dgk: DGK, signed: bool = False, kappa: int = 40, draws: DivDraws | None = None) -> torch.Tensor:
    """[[x % d]], in [0, d)."""
    return secure_divmod_batch(x_enc, divisor, x_bits, alice_paillier, bob_paillier, alice_dgk, bob_dgk, signed, kappa, draws)[1]


def secure_shift_right_batch(x_enc: torch.Tensor, t: int, x_bits: int, alice_paillier: Paillier, bob_paillier: Paillier, alice_dgk: DGK,
                             bob_dgk: DGK, signed: bool = False, kappa: int = 40, draws: DivDraws | None = None) -> torch.Tensor:
    """[[x >> t]] = [[x // 2^t]] for a public 0 <= t <= 63 (an arithmetic shift for signed input)."""
    if not 0 <= int(t) <= 63:
        raise ValueError(f"t = {t}: expected 0 <= t <= 63")
    return secure_divide_batch(x_enc, 1 << int(t), x_bits, alice_paillier, bob_paillier, alice_dgk, bob_dgk, signed, kappa, draws)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{divide,modulo}_batch) ---------------------------------------
# The announced exchange of exchange.py under the name `div`: the header is DivLayout.header, P is [[z]], the answer the key holder's [d] and
# [beta_i] as one array [l+1][B][nd]; then the sub-comparison's second round trip, `div_3_batch_{tag}` ([c_i]) and `div_4_batch_{tag}`
# ([[zq]] | [[zq]] | [[delta_B]]).
async def _alice_div(ini, tag, layout, x_enc, draws, source, generator):
    from . import wire

    pai, dgk, comm, count, l = ini.scheme_paillier, ini.scheme_dgk, ini.communicator, x_enc.shape[0], layout.l
    draws = draws if draws is not None else draw_div(count, layout, pai, dgk, source, generator, bob=False)
    z_enc, plain = div_blind(layout, x_enc, draws, pai)
    planes = await announce(ini, "div", tag, layout.header, z_enc, (l + 1, count), "[d], [beta_i]", reply_words=dgk.mod_n.nwords)
    if draws.permutation is not None and not bool(Initiator.permutation_is_valid(draws.permutation)):
        raise ValueError("permutation: a row is not a permutation of the l + 1 positions")
    c, _ = Initiator.step_4_batch(planes[0], planes[1:], plain, draws.delta_a, dgk, draws.rhos, draws.permutation, draws.r_alice_dgk)
    await comm.send(ini.other_party, wire.outgoing(comm, c), msg_id=f"div_3_batch_{tag}")
    (three,) = wire.incoming(await comm.recv(ini.other_party, msg_id=f"div_4_batch_{tag}"), x_enc.device, expect=1)
    three = wire.expect_array(three, (3, count, pai.mod_n2.nwords), "[[zq]], [[zq]], [[delta_B]]")
    return div_finish(layout, Initiator.step_6_7_batch(draws.delta_a, three[2], three[0], three[1], plain, l, pai), pai)


async def _bob_div(kh, tag, layout, draws, source, generator):
    from . import wire

    pai, dgk, comm, count, l = kh.scheme_paillier, kh.scheme_dgk, kh.communicator, len(layout.divisors), layout.l
    z_enc, _ = await receive_announced(kh, "div", tag, layout.header, "(kappa, x_bits, signed, l, rows, divisor digest)", range(6, 7), (), count)
    draws = draws if draws is not None else draw_div(count, layout, pai, dgk, source, generator, alice=False)
    plain = div_open(layout, z_enc, pai)
    d_enc, beta_enc = KeyHolder.step_4a_4b_batch(plain, l, dgk, pai, draws.r_bob_dgk)
    await answer(kh, "div", tag, torch.cat([d_enc.unsqueeze(0), beta_enc]))
    (c_enc,) = wire.incoming(await comm.recv(kh.other_party, msg_id=f"div_3_batch_{tag}"), pai.engine.device, expect=1)
    c_enc = wire.expect_array(c_enc, (l + 1, count, dgk.mod_n.nwords), "[c_i]")
    _, z1, z2, db = KeyHolder.step_4j_5_batch(c_enc, plain, pai, dgk, draws.rho3)
    await comm.send(kh.other_party, wire.outgoing(comm, torch.stack([z1, z2, db])), msg_id=f"div_4_batch_{tag}")


async def alice_divide(ini, x_enc, divisor, x_bits, signed, kappa, draws, source, engine, generator, chunks, want: str):
    """want: "div", "mod" or "divmod"."""
    no_chunks(chunks)
    sid = await ini._open_batch_session(x_enc, x_enc, engine)
    pai = ini.scheme_paillier
    layout = _layout(x_enc.shape[0], divisor, x_bits, signed, kappa, pai, ini.scheme_dgk)
    q_enc = await _alice_div(ini, f"session_{sid}", layout, x_enc, draws, source, generator)
    if want == "div":
        return q_enc
    m_enc = mod_from_quotient(layout, x_enc, q_enc, pai)
    return m_enc if want == "mod" else (q_enc, m_enc)


async def bob_divide(kh, count, divisor, x_bits, signed, kappa, draws, source, generator):
    sid = await kh._open_batch_session()
    layout = _layout(count, divisor, x_bits, signed, kappa, kh.scheme_paillier, kh.scheme_dgk)
    await _bob_div(kh, f"session_{sid}", layout, draws, source, generator)

"""Batched secure one-hot encoding of an encrypted index, and the table lookup that follows from it.

One round trip, "blind, decrypt, rotate" (semi-honest like the multiplication's §8e), for m indices [[i_q]] per row and a
public table length k:

1. Alice draws a mask r_q < 2^(ib + kappa) per index and rho_p in [1, N) per message.  The blinded index is the field d_q = i_q + r_q of
   f = ib + kappa + 1 bits; g fields fit one Paillier message at the bit offsets 0, f, 2f, .., a row takes M = ceil(m / g) messages, index
   q in message q div g at position q mod g (only the last message may hold fewer than g fields).
2. Bob decrypts the M messages of a row, takes j_q = d_q mod k and returns the k fresh encryptions E[q][t] = [[ [t == j_q] ]], t < k.
3. Alice rotates: j_q = (i_q + r_q) mod k, so [t == i_q mod k] = [(t + r_q) mod k == j_q] and out[q][t] = E[q][(t + r_q mod k) mod k] -- a
   gather of ciphertext rows, no arithmetic modulo N^2.

Precondition 0 <= i_q < 2^ib.  The result marks position i_q mod k: an index at or above k is reduced, not refused.

secure_gather_batch turns the one-hot planes into [[table[i_q]]] with one inner product (dotproduct.py) in a second round trip, whatever
m and k are.  Everything stays on the device; each step is one scheme-level library call (include/sc_amd.h: sc_initiator_onehot_pack,
sc_keyholder_onehot, sc_initiator_onehot_finish), the same calls a C host makes.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .dotproduct import DotLayout, dot_batch, draw_dot
from .exchange import announce, answer, no_chunks, receive_announced
from .schemes import Paillier

MAX_K = 1024        # table length (csrc/sc_vm.h ONEHOT_MAX_K)
MAX_M = 65536       # indices per row (csrc/sc_vm.h ONEHOT_MAX_M)


def default_index_bits(k: int) -> int:
    """The narrowest index width that reaches every position of a table of k entries: max(1, bits(k - 1))."""
    return max(1, (int(k) - 1).bit_length())


@dataclass(frozen=True)
class OnehotLayout:
    """Layout of the packed plaintexts of a one-hot encoding of m indices of ib bits against a table of k entries under a key of nbits
    bits: a field takes f = ib + kappa + 1 bits, g fields fit a message and a row takes M messages.  Raises ValueError when a quantity
    is out of range or when not even one field fits, f >= nbits - 1 (onehot_layout in csrc/sc_families.hip is the library's copy of the
    rule)."""

    kappa: int
    ib: int
    k: int
    m: int = 1
    nbits: int = 2048

    def __post_init__(self) -> None:
        for name in ("kappa", "ib", "k", "m", "nbits"):
            object.__setattr__(self, name, int(getattr(self, name)))
        if not 1 <= self.kappa <= 62:
            raise ValueError(f"kappa = {self.kappa}: expected 1 <= kappa <= 62")
        if not 1 <= self.ib <= 32:
            raise ValueError(f"ib = {self.ib}: expected an index width of 1 .. 32 bits")
        if not 1 <= self.k <= MAX_K:
            raise ValueError(f"k = {self.k}: expected a table length of 1 .. {MAX_K}")
        if not 1 <= self.m <= MAX_M:
            raise ValueError(f"m = {self.m}: expected 1 .. {MAX_M} indices per row")
        if self.f >= self.nbits - 1:
            raise ValueError(f"f = {self.f}: one field does not fit below a {self.nbits}-bit N (kappa = {self.kappa})")

    @property
    def f(self) -> int:
        return self.ib + self.kappa + 1

    @property
    def g(self) -> int:
        """Fields per message: the largest integer with g f < bits(N) - 1."""
        return max(1, (self.nbits - 2) // self.f)

    @property
    def M(self) -> int:
        """Messages per row."""
        return -(-self.m // self.g)

    @property
    def rw(self) -> int:
        """Words of a mask of ib + kappa bits."""
        return (self.ib + self.kappa + 31) // 32

    def position(self, q: int) -> tuple[int, int]:
        """(message, position) of index q: its field sits at bits [t f, (t + 1) f) of message mm."""
        if not 0 <= q < self.m:
            raise ValueError(f"index {q}: expected 0 .. {self.m - 1}")
        return q // self.g, q % self.g

    @property
    def header(self) -> list[int]:
        """What `onehot_1_batch_{tag}` announces: kappa, ib, k, m."""
        return [self.kappa, self.ib, self.k, self.m]


@dataclass
class OnehotDraws:
    """The random inputs of one one-hot batch: Alice's r [m][B][rw] (< 2^(ib + kappa)) and rho_p [M][B][nw] (the messages' randomizers);
    Bob's rho_e [m][k][B][nw] (the randomizers of his m k B answers).  Either side None."""

    r: torch.Tensor | None
    rho_p: torch.Tensor | None
    rho_e: torch.Tensor | None


def draw_onehot(count: int, layout: OnehotLayout, paillier: Paillier, source: str = "device", generator=None, alice: bool = True,
                bob: bool = True) -> OnehotDraws:
    """Both players' (or one player's) draws for `count` rows.  Alice, two generator calls: r as m count items of ib + kappa bits,
    index-major (index q of row b is item q count + b); rho_p as M count items in [1, N), message-major.  Bob, one call: m k count bases
    in [1, N), in [q][t][b] order.  No two indices share a mask."""
    from .randomness import random_bits, uniform_below

    e, n = paillier.engine, paillier.public_key.n
    m, k, M = layout.m, layout.k, layout.M
    r = rho_p = rho_e = None
    if alice:
        r = random_bits(layout.ib + layout.kappa, (m * count,), e, source, generator).reshape(m, count, -1)
        rho_p = uniform_below(n, M * count, e, source, generator, nonzero=True).reshape(M, count, -1)
    if bob:
        rho_e = uniform_below(n, m * k * count, e, source, generator, nonzero=True).reshape(m, k, count, -1)
    return OnehotDraws(r=r, rho_p=rho_p, rho_e=rho_e)


# ---- the three steps --------------------------------------------------------------------------------------------------------------
def _indices(layout: OnehotLayout, index_enc: torch.Tensor) -> torch.Tensor:
    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() != 3 or index_enc.shape[0] != layout.m:
        raise ValueError(f"index_enc: expected [{layout.m}][B][words]")
    return index_enc.contiguous()


def onehot_pack(layout: OnehotLayout, index_enc: torch.Tensor, draws: OnehotDraws, paillier: Paillier):
    """Alice, step 1: (P [M][B][2nw], rot [m][B]) from [[i_q]] [m][B][2nw]; rot = r mod k is what onehot_finish needs
    (sc_initiator_onehot_pack)."""
    return paillier.engine.initiator_onehot_pack(paillier.key, layout.kappa, layout.ib, layout.k, layout.m, layout.M, _indices(layout, index_enc),
                                                 draws.r, draws.rho_p)


def onehot_answer(layout: OnehotLayout, P: torch.Tensor, paillier: Paillier, rho_e: torch.Tensor) -> torch.Tensor:
    """Bob, step 2: the CRT decryption of the M B messages, [t == d_q mod k] per index and position, encrypted and freshly randomized:
    E [m][k][B][2nw] (sc_keyholder_onehot).  ValueError when a decrypted message does not fit the announced layout."""
    return paillier.engine.keyholder_onehot(paillier.key, layout.kappa, layout.ib, layout.k, layout.m, layout.M, P.contiguous(), rho_e.contiguous())


def onehot_finish(layout: OnehotLayout, E: torch.Tensor, rot: torch.Tensor, paillier: Paillier, out: torch.Tensor | None = None) -> torch.Tensor:
    """Alice, step 3: out[q][t] = E[q][(t + rot_q) mod k], [m][k][B][2nw] (sc_initiator_onehot_finish): one launch."""
    return paillier.engine.initiator_onehot_finish(paillier.key, layout.kappa, layout.ib, layout.k, layout.m, E.contiguous(), rot.contiguous(), out)


def onehot_batch(layout: OnehotLayout, index_enc: torch.Tensor, alice_paillier: Paillier, bob_paillier: Paillier,
                 draws: OnehotDraws) -> torch.Tensor:
    """Both players' halves of one one-hot batch in one process: [m][k][B][2nw]."""
    P, rot = onehot_pack(layout, index_enc, draws, alice_paillier)
    E = onehot_answer(layout, P, bob_paillier, draws.rho_e)
    return onehot_finish(layout, E, rot, alice_paillier)


# ---- one-hot, gather, lookup ------------------------------------------------------------------------------------------------------------
def _as_planes(index_enc) -> tuple[torch.Tensor, bool]:
    """([m][B][2nw], whether the caller gave the single-index form [B][2nw])."""
    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() not in (2, 3):
        raise ValueError("index_enc: expected [B][words] or [m][B][words]")
    return (index_enc.unsqueeze(0), True) if index_enc.dim() == 2 else (index_enc, False)


def _layout(index_enc: torch.Tensor, k: int, index_bits, kappa: int, paillier: Paillier) -> OnehotLayout:
    k = int(k)
    ib = default_index_bits(max(k, 1)) if index_bits is None else int(index_bits)
    return OnehotLayout(kappa, ib, k, index_enc.shape[0], paillier.public_key.n.bit_length())


def secure_onehot_batch(index_enc: torch.Tensor, k: int, alice_paillier: Paillier, bob_paillier: Paillier, index_bits: int | None = None,
                        kappa: int = 40, draws: OnehotDraws | None = None) -> torch.Tensor:
    """[[ [t == i mod k] ]], t < k, for B rows of Paillier-encrypted indices under Bob's key: index_enc [B][2nw] -> [k][B][2nw], or m
    indices per row, [m][B][2nw] -> [m][k][B][2nw]; 1 <= k <= 1024.  0 <= i < 2^index_bits (default max(1, bits(k - 1))); an index at or
    above k marks position i mod k."""
    planes, single = _as_planes(index_enc)
    layout = _layout(planes, k, index_bits, kappa, alice_paillier)                       # the fit rule, before any launch
    draws = draws if draws is not None else draw_onehot(planes.shape[1], layout, alice_paillier)
    out = onehot_batch(layout, planes, alice_paillier, bob_paillier, draws)
    return out[0] if single else out


def _gather_operands(table_enc: torch.Tensor, onehot: torch.Tensor):
    """The inner product's operands over m B rows: x = the table's planes repeated for every index, y = the one-hot planes, both
    [k][m B][2nw] (row q B + b is index q of row b)."""
    m, k, B, w = onehot.shape
    x = table_enc.unsqueeze(1).expand(k, m, B, w).reshape(k, m * B, w)
    y = onehot.permute(1, 0, 2, 3).reshape(k, m * B, w)
    return x.contiguous(), y.contiguous()


def _gather_layout(k: int, bits: int, signed: bool, kappa: int, paillier: Paillier) -> DotLayout:
    """x = the table (width `bits`), y = a one-hot plane: width 1, or 2 for a signed table (the signed range of one bit is {-1, 0}, of two
    bits {-2 .. 1}, which holds 0 and 1)."""
    return DotLayout(kappa, int(bits), 2 if signed else 1, k, signed, False, paillier.public_key.n.bit_length())


def _table(table_enc) -> torch.Tensor:
    if not isinstance(table_enc, torch.Tensor) or table_enc.dim() != 3:
        raise ValueError("table_enc: expected [k][B][words]")
    return table_enc


def secure_gather_batch(table_enc: torch.Tensor, index_enc: torch.Tensor, bits: int, alice_paillier: Paillier, bob_paillier: Paillier,
                        signed: bool = False, kappa: int = 40, index_bits: int | None = None) -> torch.Tensor:
    """[[table[i_q]]] for B rows of an encrypted table of k entries and m encrypted indices each: table_enc [k][B][2nw], index_enc
    [m][B][2nw] -> [m][B][2nw].  Table entries: 0 <= v < 2^bits, or -2^(bits - 1) <= v < 2^(bits - 1) as residues modulo N when signed.
    Two round trips whatever m and k are: the one-hot, then one inner product over m B rows."""
    table_enc = _table(table_enc)
    planes, _ = _as_planes(index_enc)
    k, B = table_enc.shape[0], table_enc.shape[1]
    if planes.dim() != 3 or planes.shape[1] != B or planes.shape[2] != table_enc.shape[2]:
        raise ValueError(f"index_enc: expected [m][{B}][{table_enc.shape[2]}] beside table_enc [{k}][{B}][{table_enc.shape[2]}]")
    layout = _layout(planes, k, index_bits, kappa, alice_paillier)
    dot = _gather_layout(k, bits, signed, kappa, alice_paillier)                          # both fit rules, before any launch
    onehot = onehot_batch(layout, planes, alice_paillier, bob_paillier, draw_onehot(B, layout, alice_paillier))
    x, y = _gather_operands(table_enc, onehot)
    m = planes.shape[0]
    return dot_batch(dot, x, y, alice_paillier, bob_paillier, draw_dot(m * B, dot, alice_paillier)).reshape(m, B, -1)


def secure_lookup_batch(table_enc: torch.Tensor, index_enc: torch.Tensor, bits: int, alice_paillier: Paillier, bob_paillier: Paillier,
                        signed: bool = False, kappa: int = 40, index_bits: int | None = None) -> torch.Tensor:
    """The m = 1 form of secure_gather_batch: index_enc [B][2nw] -> [[table[i]]] [B][2nw]."""
    if not isinstance(index_enc, torch.Tensor) or index_enc.dim() != 2:
        raise ValueError("index_enc: expected [B][words]")
    return secure_gather_batch(table_enc, index_enc.unsqueeze(0), bits, alice_paillier, bob_paillier, signed, kappa, index_bits)[0]


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_onehot_batch, .perform_secure_gather_batch) --------------
# the announced exchange of exchange.py under the name `onehot`: the header is OnehotLayout.header, exactly 4 entries, P is [M][B][2nw] and
# the answer the key holder's E.
async def alice_onehot(ini, index_enc, k, index_bits, kappa, draws, source, engine, generator, chunks):
    no_chunks(chunks)
    planes, single = _as_planes(index_enc)
    sid = await ini._open_batch_session(planes[0], planes[0], engine)
    pai, count = ini.scheme_paillier, planes.shape[1]
    layout = _layout(planes, k, index_bits, kappa, pai)
    draws = draws if draws is not None else draw_onehot(count, layout, pai, source, generator, bob=False)
    P, rot = onehot_pack(layout, planes, draws, pai)
    E = await announce(ini, "onehot", f"session_{sid}", layout.header, P, (layout.m, layout.k, count), "E")
    out = onehot_finish(layout, E, rot, pai)
    return out[0] if single else out


async def bob_onehot(kh, k, m, index_bits, kappa, draws, source, generator, count=None):
    sid = await kh._open_batch_session()
    pai, tag = kh.scheme_paillier, f"session_{sid}"
    ib = default_index_bits(max(int(k), 1)) if index_bits is None else int(index_bits)
    layout = OnehotLayout(kappa, ib, int(k), int(m), pai.public_key.n.bit_length())
    P, count = await receive_announced(kh, "onehot", tag, layout.header, "(kappa, ib, k, m)", range(4, 5), (layout.M,), count)
    rho = draws.rho_e if draws is not None else draw_onehot(count, layout, pai, source, generator, alice=False).rho_e
    await answer(kh, "onehot", tag, onehot_answer(layout, P, pai, rho))
    return count


async def alice_gather(ini, table_enc, index_enc, bits, signed, kappa, index_bits, source, engine, generator, chunks):
    from .dotproduct import alice_dot

    no_chunks(chunks)
    table_enc = _table(table_enc)
    planes, _ = _as_planes(index_enc)
    k, B = table_enc.shape[0], table_enc.shape[1]
    if planes.shape[1] != B or planes.shape[2] != table_enc.shape[2]:
        raise ValueError(f"index_enc: expected [m][{B}][{table_enc.shape[2]}] beside table_enc [{k}][{B}][{table_enc.shape[2]}]")
    onehot = await alice_onehot(ini, planes, k, index_bits, kappa, None, source, engine, generator, 1)
    dot = _gather_layout(k, bits, signed, kappa, ini.scheme_paillier)
    x, y = _gather_operands(table_enc, onehot)
    out = await alice_dot(ini, x, y, dot.wx, dot.wy, signed, False, kappa, None, source, engine, generator, 1)
    return out.reshape(planes.shape[0], B, -1)


async def bob_gather(kh, k, m, bits, signed, kappa, index_bits, source, generator, count=None):
    from .dotproduct import bob_dot

    count = await bob_onehot(kh, k, m, index_bits, kappa, None, source, generator, count)
    dot = _gather_layout(int(k), bits, signed, kappa, kh.scheme_paillier)
    await bob_dot(kh, int(k), dot.wx, dot.wy, signed, False, kappa, None, source, generator, int(m) * count)

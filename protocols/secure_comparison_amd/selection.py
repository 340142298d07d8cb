"""Batched secure selection on top of the comparison: [[min(x, y)]], [[max(x, y)]], and argmin / argmax over k values per row.

One extra round trip after the comparison turns [[delta]] = [[x <= y]] into the selected ciphertext ("Secure
selection").  For a selector sigma in {0, 1} and columns j with [[b_j]] and [[d_j]], d_j = a_j - b_j + 2^w_j:

1. Alice packs P = [[sigma]] * prod_j [[d_j]]^(2^off_j) * (1 + R N) * rho^N, plaintext (sigma + r_a) + sum_j 2^off_j (d_j + r_b_j).
2. Bob decrypts P once, splits the fields a = sigma + r_a and b_j = d_j + r_b_j and returns the fresh encryptions [[a b_j]].
3. Alice unblinds: [[b_j + sigma (a_j - b_j)]] = [[b_j]] [[a b_j]] T_j^-1 with T_j = [[sigma]]^(r_b_j + 2^w_j) [[d_j]]^r_a (1 + r_a r_b_j N).

Everything stays on the device.  Each step is one scheme-level library call (include/sc_amd.h: sc_initiator_select_d,
sc_paillier_one_minus, sc_initiator_select_pack, sc_keyholder_select_mult, sc_initiator_select_finish), the same calls a C host makes;
the exponentiations with per-row exponents run on the pair interpreter (sc_modexp_var_sq) where the modulus has such an instance.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .batch import BatchDraws, BatchTrace, draw_alice, draw_bob, secure_comparison_batch
from .exchange import announce, answer, no_chunks, receive_announced
from .flags import check_l
from .schemes import DGK, Paillier

MAX_FIELDS = 4      # columns of one selection (csrc/sc_vm.h SEL_MAX_FIELDS)


@dataclass(frozen=True)
class SelectLayout:
    """Field layout of the packed plaintext of P for a value of l bits and payload columns of payload_bits[i] bits, under a key of
    nbits bits: a = sigma + r_a in [0, s), s = kappa + 1, then column j (width w_j: d_j < 2^(w_j + 1)) in w_j + kappa + 2 bits.
    Raises ValueError when the fields, or one product a * b_j, would not fit below N."""

    l: int
    kappa: int
    payload_bits: tuple = ()
    nbits: int = 2048

    def __post_init__(self) -> None:
        object.__setattr__(self, "payload_bits", tuple(int(b) for b in self.payload_bits))
        if not 1 <= self.kappa <= 62:
            raise ValueError(f"kappa = {self.kappa}: expected 1 <= kappa <= 62")
        if self.l < 1 or any(b < 1 for b in self.payload_bits):
            raise ValueError("column widths must be >= 1")
        if len(self.widths) > MAX_FIELDS:
            raise ValueError(f"{len(self.widths)} columns: at most {MAX_FIELDS}")
        for j, f in enumerate(self.fbits):
            if self.s + f >= self.nbits - 1:
                raise ValueError(f"column {j}: the product a * b ({self.s + f} bits) does not fit below a {self.nbits}-bit N")
        if self.end >= self.nbits - 1:
            raise ValueError(f"the packed fields ({self.end} bits) do not fit below a {self.nbits}-bit N (kappa = {self.kappa})")

    @property
    def widths(self) -> list[int]:
        return [self.l, *self.payload_bits]

    @property
    def s(self) -> int:
        return self.kappa + 1

    @property
    def fbits(self) -> list[int]:
        return [w + self.kappa + 2 for w in self.widths]

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
    def t_bits(self) -> int:
        """Bits of the exponents of T: r_b_j + 2^w_j < 2^(w_j + kappa + 2), r_a < 2^kappa."""
        return max(self.fbits)

    @property
    def header(self) -> list[int]:
        """What `select_1_batch_{tag}` announces: kappa, the column widths."""
        return [self.kappa, *self.widths]


@dataclass
class SelectDraws:
    """The random inputs of one selection batch: Alice's r_a [B][aw] (< 2^kappa), r_b [nf][B][bw] (column j < 2^(w_j + 1 + kappa)) and
    rho_p [B][nw] (P's randomizer); Bob's rho_products [nf][B][nw] (the randomizers of his returned products).  Either side None."""

    r_a: torch.Tensor | None
    r_b: torch.Tensor | None
    rho_p: torch.Tensor | None
    rho_products: torch.Tensor | None


def draw_select(count: int, layout: SelectLayout, paillier: Paillier, source: str = "device", generator=None,
                alice: bool = True, bob: bool = True) -> SelectDraws:
    """Both players' (or one player's) selection draws for `count` rows, on the device or from a seeded torch generator."""
    from .randomness import random_bits, random_columns, uniform_below

    e, n = paillier.engine, paillier.public_key.n
    nf = len(layout.widths)
    r_a = r_b = rho_p = rho_q = None
    if alice:
        r_a = random_bits(layout.kappa, (count,), e, source, generator)
        r_b = random_columns([w + 1 + layout.kappa for w in layout.widths], (max(layout.fbits) + 31) // 32, count, e, source, generator)
        rho_p = uniform_below(n, count, e, source, generator, nonzero=True)
    if bob:
        rho_q = uniform_below(n, nf * count, e, source, generator, nonzero=True).reshape(nf, count, -1)
    return SelectDraws(r_a=r_a, r_b=r_b, rho_p=rho_p, rho_products=rho_q)


# ---- the three steps --------------------------------------------------------------------------------------------------------------
def select_pack(layout: SelectLayout, sigma_enc: torch.Tensor, d_enc: torch.Tensor, draws: SelectDraws, paillier: Paillier):
    """Alice, step 1: P [B][2nw] from [[sigma]] [B][2nw] and [[d_j]] [nf][B][2nw]; returns (P, (e, rab)) -- the latter is what
    select_finish needs (sc_initiator_select_pack)."""
    nf, count = len(layout.widths), sigma_enc.shape[0]
    if d_enc.dim() != 3 or d_enc.shape[0] != nf or d_enc.shape[1] != count:
        raise ValueError(f"d_enc: expected [{nf}][{count}][words]")
    ew = (layout.t_bits + 31) // 32
    P, et, rab = paillier.engine.initiator_select_pack(paillier.key, layout.kappa, layout.widths, sigma_enc, d_enc.contiguous(), draws.r_a,
                                                       draws.r_b, draws.rho_p, ew)
    return P, (et, rab)


def select_mult(layout: SelectLayout, P: torch.Tensor, paillier: Paillier, rho_products: torch.Tensor) -> torch.Tensor:
    """Bob, step 2: one CRT decryption of P, the field products a * b_j, encrypted and freshly randomized: [nf][B][2nw]
    (sc_keyholder_select_mult).  ValueError when a decrypted row does not fit the announced layout (the players disagree on kappa
    or the widths)."""
    return paillier.engine.keyholder_select_mult(paillier.key, layout.kappa, layout.widths, P, rho_products.contiguous())


def select_finish(layout: SelectLayout, sigma_enc: torch.Tensor, d_enc: torch.Tensor, b_enc: torch.Tensor, products: torch.Tensor,
                  plain, draws: SelectDraws, paillier: Paillier) -> torch.Tensor:
    """Alice, step 3: [[b_j + sigma (a_j - b_j)]] [nf][B][2nw] from Bob's products (sc_initiator_select_finish): T_j =
    [[sigma]]^(r_b_j + 2^w_j) [[d_j]]^r_a (1 + r_a r_b_j N), one inversion, one launch."""
    et, rab = plain
    return paillier.engine.initiator_select_finish(paillier.key, layout.kappa, layout.widths, sigma_enc, d_enc.contiguous(), b_enc.contiguous(),
                                                   products.contiguous(), draws.r_a, et, rab)


def select_batch(layout: SelectLayout, sigma_enc: torch.Tensor, d_enc: torch.Tensor, b_enc: torch.Tensor, alice_paillier: Paillier,
                 bob_paillier: Paillier, draws: SelectDraws) -> torch.Tensor:
    """Both players' halves of one selection batch in one process: [[b_j + sigma (a_j - b_j)]] [nf][B][2nw]."""
    P, plain = select_pack(layout, sigma_enc, d_enc, draws, alice_paillier)
    products = select_mult(layout, P, bob_paillier, draws.rho_products)
    return select_finish(layout, sigma_enc, d_enc, b_enc, products, plain, draws, alice_paillier)


# ---- min / max ---------------------------------------------------------------------------------------------------------------------
def _comparison_draws(count: int, l: int, ap: Paillier, ad: DGK, bp: Paillier, bd: DGK) -> BatchDraws:
    a, b = draw_alice(count, l, ap, ad), draw_bob(count, l, bp, bd)
    return BatchDraws(r=a.r, delta_a=a.delta_a, rhos=a.rhos, permutation=a.permutation, rho_z=a.rho_z, r_bob_dgk=b.r_bob_dgk,
                      r_alice_dgk=a.r_alice_dgk, rho_zeta_1=b.rho_zeta_1, rho_zeta_2=b.rho_zeta_2, rho_delta_b=b.rho_delta_b)


def _compare(x_enc, y_enc, l, ap, ad, bp, bd, draws):
    """[[x <= y]] and Alice's [[d]] = [[y - x + 2^l]] = [[z + r]] (1 - r N) from step 1 (z = y - x + 2^l): no inversion."""
    draws = draws if draws is not None else _comparison_draws(x_enc.shape[0], l, ap, ad, bp, bd)
    trace = BatchTrace()
    delta = secure_comparison_batch(x_enc, y_enc, l, ap, ad, bp, bd, draws, trace=trace)
    return delta, ap.engine.initiator_select_d(ap.key, trace.z_enc, draws.r)


def _one_minus(paillier: Paillier, c: torch.Tensor) -> torch.Tensor:
    """[[1 - c]] = g [[c]]^-1 (one batched inversion; sc_paillier_one_minus)."""
    return paillier.engine.paillier_one_minus(paillier.key, c)


def _minmax(x_enc, y_enc, l, ap, ad, bp, bd, draws, select_draws, kappa, want_max):
    check_l(l)
    layout = SelectLayout(l, kappa, (), ap.public_key.n.bit_length())
    delta, d = _compare(x_enc, y_enc, l, ap, ad, bp, bd, draws)
    sigma = delta if want_max else _one_minus(ap, delta)            # max = x + delta (y - x), min = x + (1 - delta)(y - x)
    sd = select_draws if select_draws is not None else draw_select(x_enc.shape[0], layout, ap)
    out = select_batch(layout, sigma, d.unsqueeze(0), x_enc.unsqueeze(0), ap, bp, sd)
    return out[0], delta


def secure_minimum_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK,
                         bob_paillier: Paillier, bob_dgk: DGK, draws: BatchDraws | None = None,
                         select_draws: SelectDraws | None = None, kappa: int = 40):
    """([[min(x, y)]], [[x <= y]]) for B pairs of Paillier ciphertexts [B][2nw] under Bob's key, 0 <= x, y < 2^l."""
    return _minmax(x_enc, y_enc, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, draws, select_draws, kappa, False)


def secure_maximum_batch(x_enc: torch.Tensor, y_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK,
                         bob_paillier: Paillier, bob_dgk: DGK, draws: BatchDraws | None = None,
                         select_draws: SelectDraws | None = None, kappa: int = 40):
    """([[max(x, y)]], [[x <= y]]): the same comparison and selection; the minimum selects with [[1 - delta]] instead (one
    extra batched inversion)."""
    return _minmax(x_enc, y_enc, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, draws, select_draws, kappa, True)


# ---- argmin / argmax -----------------------------------------------------------------------------------------------------------------
def index_bits(k: int) -> int:
    """Width of the index column: indices 0 .. k - 1 are below 2^index_bits(k)."""
    return max(1, (k - 1).bit_length())


def tournament_rounds(k: int) -> int:
    """Rounds of the argmin / argmax tournament over k values: ceil(log2 k)."""
    return (k - 1).bit_length()


def _arg_inputs(ap, lv, li, rv, ri, delta, d_v, k, want_max):
    """The selection inputs of one tournament round from its comparison.  min compared (L, R): delta = [L <= R], d = R - L + 2^l,
    winner = L + (1 - delta)(R - L).  max compared (R, L): delta' = [R <= L], d = L - R + 2^l, winner = R + delta' (L - R).  Both
    keep the left operand on ties.  Returns (sigma, [[d]] [2][P][2nw], [[b]] [2][P][2nw])."""
    n, count, wi = ap.public_key.n, lv.shape[0], index_bits(k)
    if not want_max:            # [[1 - delta]] and the index column's [[L.i]]^-1 share one batched inversion
        inv = ap.neg_batch(torch.cat([delta, li]))
        sigma = ap.engine.modmul_const(ap.mod_n2, inv[:count], n + 1)
        d_i = ap.engine.modmul_const(ap.mod_n2, ap.add_batch(ri, inv[count:]), 1 + (1 << wi) * n)
        return sigma, torch.stack([d_v, d_i]), torch.stack([lv, li])
    d_i = ap.engine.modmul_const(ap.mod_n2, ap.add_batch(li, ap.neg_batch(ri)), 1 + (1 << wi) * n)
    return delta, torch.stack([d_v, d_i]), torch.stack([rv, ri])


def _arg_start(v_enc, l, ap, kappa):
    check_l(l)
    if v_enc.dim() != 3:
        raise ValueError("v_enc: expected [B][k][2nw]")
    B, k, _ = v_enc.shape
    if k < 1:
        raise ValueError("k must be >= 1")
    layout = SelectLayout(l, kappa, (index_bits(k),), ap.public_key.n.bit_length())    # the layout check before any launch
    vals = [v_enc[:, i].contiguous() for i in range(k)]
    idx = [ap.encrypt_raw_batch(ap.engine.upload([i] * B, 1)) for i in range(k)]         # trivial encryptions 1 + i N
    return layout, B, k, vals, idx


def _pairs(vals, idx):
    """The round's pairs (2t, 2t + 1) of every row as [h B][2nw] arrays: (h, left values, left indices, right values, right indices)."""
    h = len(vals) // 2
    cat = lambda xs: torch.cat(xs).contiguous()  # noqa: E731
    return h, cat(vals[0:2 * h:2]), cat(idx[0:2 * h:2]), cat(vals[1:2 * h:2]), cat(idx[1:2 * h:2])


def _unpair(wv, wi, vals, idx, h, B):
    nv = [wv[t * B:(t + 1) * B] for t in range(h)]
    ni = [wi[t * B:(t + 1) * B] for t in range(h)]
    if len(vals) % 2:                       # the odd element carries over to the next round
        nv.append(vals[-1])
        ni.append(idx[-1])
    return nv, ni


def _argext(v_enc, l, ap, ad, bp, bd, kappa, want_max):
    layout, B, k, vals, idx = _arg_start(v_enc, l, ap, kappa)
    while len(vals) > 1:
        h, lv, li, rv, ri = _pairs(vals, idx)
        delta, d_v = _compare(rv, lv, l, ap, ad, bp, bd, None) if want_max else _compare(lv, rv, l, ap, ad, bp, bd, None)
        sigma, d, b = _arg_inputs(ap, lv, li, rv, ri, delta, d_v, k, want_max)
        out = select_batch(layout, sigma, d, b, ap, bp, draw_select(lv.shape[0], layout, ap))
        vals, idx = _unpair(out[0], out[1], vals, idx, h, B)
    return vals[0].contiguous(), idx[0].contiguous()


def secure_argmin_batch(v_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                        kappa: int = 40):
    """([[min_i v_i]], [[argmin_i v_i]]) over k values per row, v_enc [B][k][2nw]; ties go to the lowest index.  A tournament of
    ceil(log2 k) rounds, each one comparison batch and one two-column selection batch over the row's pairs."""
    return _argext(v_enc, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, kappa, False)


def secure_argmax_batch(v_enc: torch.Tensor, l: int, alice_paillier: Paillier, alice_dgk: DGK, bob_paillier: Paillier, bob_dgk: DGK,
                        kappa: int = 40):
    """([[max_i v_i]], [[argmax_i v_i]]); ties go to the lowest index."""
    return _argext(v_enc, l, alice_paillier, alice_dgk, bob_paillier, bob_dgk, kappa, True)


# ---- the two players over a Communicator (Initiator / KeyHolder.perform_secure_{minimum,maximum,argmin,argmax}_batch) -----------------
# Each round is one batched comparison session (Initiator._batch_session, its messages unchanged) followed by one selection exchange:
# the announced exchange of exchange.py under the name `select`: the header is kappa and the column widths, the answer the key holder's
# products.
async def _alice_compare(ini, tag, x_enc, y_enc, draws, source, generator):
    keep = {}
    delta = await ini._batch_session(tag, x_enc, y_enc, draws, source, generator, None, keep=keep)
    pai = ini.scheme_paillier
    return delta, pai.engine.initiator_select_d(pai.key, keep["z_enc"], keep["r"])


async def _alice_exchange(ini, tag, layout, sigma, d, sd, source, generator):
    """Alice's selection exchange up to Bob's products: (products [nf][B][2nw], plain, draws) for select_finish or the sort's
    compare-exchange finish."""
    pai, count = ini.scheme_paillier, sigma.shape[0]
    sd = sd if sd is not None else draw_select(count, layout, pai, source, generator, bob=False)
    P, plain = select_pack(layout, sigma, d, sd, pai)
    prods = await announce(ini, "select", tag, layout.header, P, (len(layout.widths), count), "[[a b_j]]")
    return prods, plain, sd


async def _alice_select(ini, tag, layout, sigma, d, b, sd, source, generator):
    prods, plain, sd = await _alice_exchange(ini, tag, layout, sigma, d, sd, source, generator)
    return select_finish(layout, sigma, d, b, prods, plain, sd, ini.scheme_paillier)


async def alice_minmax(ini, x_enc, y_enc, draws, select_draws, kappa, source, engine, generator, chunks, want_max):
    from .batch import draw_alice

    no_chunks(chunks)
    sid = await ini._open_batch_session(x_enc, y_enc, engine)
    pai, dgk, l = ini.scheme_paillier, ini.scheme_dgk, ini.l_maximum_bit_length
    layout = SelectLayout(l, kappa, (), pai.public_key.n.bit_length())
    if draws is None:
        draws = draw_alice(x_enc.shape[0], l, pai, dgk, source, generator)
    tag = f"session_{sid}"
    delta, d = await _alice_compare(ini, tag, x_enc, y_enc, draws, source, generator)
    sigma = delta if want_max else _one_minus(pai, delta)
    out = await _alice_select(ini, tag, layout, sigma, d.unsqueeze(0), x_enc.unsqueeze(0), select_draws, source, generator)
    return out[0], delta


async def alice_argext(ini, v_enc, kappa, source, engine, generator, chunks, want_max):
    no_chunks(chunks)
    if v_enc.dim() != 3:
        raise ValueError("v_enc: expected [B][k][2nw]")
    sid = await ini._open_batch_session(v_enc[:, 0], v_enc[:, 0], engine)
    pai, l = ini.scheme_paillier, ini.l_maximum_bit_length
    layout, B, k, vals, idx = _arg_start(v_enc, l, pai, kappa)
    rnd = 0
    while len(vals) > 1:
        tag = f"session_{sid}_round_{rnd}"
        h, lv, li, rv, ri = _pairs(vals, idx)
        x, y = (rv, lv) if want_max else (lv, rv)
        delta, d_v = await _alice_compare(ini, tag, x, y, None, source, generator)
        sigma, d, b = _arg_inputs(pai, lv, li, rv, ri, delta, d_v, k, want_max)
        out = await _alice_select(ini, tag, layout, sigma, d, b, None, source, generator)
        vals, idx = _unpair(out[0], out[1], vals, idx, h, B)
        rnd += 1
    return vals[0].contiguous(), idx[0].contiguous()


async def _bob_select(kh, tag, layout, count, select_draws, source, generator):
    """The key holder's selection exchange after a comparison session of `count` rows: the layout check, then his products."""
    pai = kh.scheme_paillier
    P, _ = await receive_announced(kh, "select", tag, layout.header, "kappa and widths", range(2 + MAX_FIELDS), (), count)
    rho = (select_draws.rho_products if select_draws is not None
           else draw_select(count, layout, pai, source, generator, alice=False).rho_products)
    await answer(kh, "select", tag, select_mult(layout, P, pai, rho))


async def bob_rounds(kh, rounds, draws, select_draws, kappa, source, generator, payload_bits):
    """The key holder's side: `rounds` times (comparison session, selection exchange); he expects the layout (kappa, l, payload_bits)."""
    sid = await kh._open_batch_session()
    pai, l = kh.scheme_paillier, kh.l_maximum_bit_length
    layout = SelectLayout(l, kappa, tuple(payload_bits), pai.public_key.n.bit_length())
    for rnd in range(rounds):
        tag = f"session_{sid}" if not payload_bits else f"session_{sid}_round_{rnd}"
        count = await kh._batch_session(tag, None, draws, source, generator)
        await _bob_select(kh, tag, layout, count, select_draws, source, generator)

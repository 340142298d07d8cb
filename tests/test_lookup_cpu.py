"""Secure one-hot encoding and lookup without a GPU: the pure-Python model (tests/_onehot_model.py) decrypts to [t == i mod k] on a
512-bit oracle key; the package's OnehotLayout, the library's sc_onehot_layout (host code, no context) and the model agree on
(f, g, M, rw) and on every refusal; g is maximal; no two fields of a message overlap and no two indices share a mask; draw_onehot's
generator calls -- order, item layout, widths -- are held to tests/_draw_replay.py's Replay; a key holder refuses a header that is not
his own before he decrypts, and chunked sessions raise."""
import asyncio
import os
import random
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _draw_replay as dr  # noqa: E402
import _onehot_model as model  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402

KEY = bytes((11 * i + 5) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def sk():
    from oracle import sc_oracle as o

    return o.PaillierKey.generate(512, random.Random(20262))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ib,kappa", [(1, 1, 40), (2, 1, 40), (3, 2, 40), (7, 3, 40), (8, 4, 40), (5, 32, 62), (3, 2, 1), (1000, 10, 40)])
def test_model_onehot_decrypts_to_the_indicator(sk, k, ib, kappa):
    """512-bit key.  Indices at 0, k - 1 and 2^ib - 1 (at or above k where ib allows: reduced, not refused); masks at 0, at their maximum,
    with only their top word set, and random.  k = 1000 runs one index under one mask only: 1000 encryptions per row."""
    rng = random.Random(k * 100 + ib + kappa)
    n = sk.n
    top = (1 << (ib + kappa)) - 1
    high = top & ~((1 << (32 * ((ib + kappa - 1) // 32))) - 1)            # only the bits of the top word
    idx = [0, (k - 1) % (1 << ib), (1 << ib) - 1] if k < 1000 else [(1 << ib) - 1]
    fills = (0, top, high, None) if k < 1000 else (high,)
    for fill in fills:
        m = len(idx)
        draws = model.draw(rng, kappa, ib, k, m, n)
        if fill is not None:
            draws = ([fill] * m, draws[1], draws[2])
        got = model.onehot(sk, idx, k, ib, rng, kappa, draws)
        assert got == [[1 if t == i % k else 0 for t in range(k)] for i in idx], (fill, idx)


def test_model_rotation_undoes_the_mask(sk):
    """The identity the protocol rests on, on plain integers: with j = (i + r) mod k and rot = r mod k, position t of the output reads
    the key holder's row (t + rot) mod k, which is hot exactly when t = i mod k."""
    rng = random.Random(3)
    for k in (1, 2, 3, 7, 8, 1000, 1024):
        for _ in range(50):
            i, r = rng.getrandbits(32), rng.getrandbits(94)
            j, rot = (i + r) % k, r % k
            E = [[1 if t == j else 0 for t in range(k)]]
            assert model.rotate(E, [rot], k, 1)[0] == [1 if t == i % k else 0 for t in range(k)]


def test_model_flags_a_message_past_its_own_end(sk):
    """ib = 10, kappa = 40 on 512 bits: f = 51, g = 10.  m = 11: message 0 holds ten fields, message 1 one.  A bit at 51 of message 1 is
    past its end and inside message 0's."""
    f, g, M, _ = model.layout(40, 10, 7, 11, 512)
    assert (f, g, M) == (51, 10, 2)
    assert model.split(40, 10, 7, 11, 512, [(1 << 510) - 1, (1 << 51) - 1])[2] is False
    assert model.split(40, 10, 7, 11, 512, [0, 1 << 51])[2] is True
    assert model.split(40, 10, 7, 11, 512, [1 << 510, 0])[2] is True
    d, j, _ = model.split(40, 10, 7, 11, 512, [sum((q + 1) << (51 * q) for q in range(10)), 12345])
    assert d == list(range(1, 11)) + [12345] and j == [v % 7 for v in d]


# ---- the three copies of the fit rule ---------------------------------------------------------------------------------------------------
def _three(nbits, kappa, ib, k, m):
    """(f, g, M, rw) from OnehotLayout, sc_onehot_layout and the model, or None from each on a refusal; they must agree."""
    from protocols.secure_comparison_amd import OnehotLayout, _lib
    from protocols.secure_comparison_amd.engine import onehot_layout

    def attempt(fn):
        try:
            return tuple(fn())
        except ValueError:
            return None

    def py():
        lay = OnehotLayout(kappa, ib, k, m, nbits)
        return lay.f, lay.g, lay.M, lay.rw

    got = [attempt(py), attempt(lambda: onehot_layout(_lib.load(), nbits, kappa, ib, k, m)), attempt(lambda: model.layout(kappa, ib, k, m, nbits))]
    assert got[0] == got[1] == got[2], (nbits, kappa, ib, k, m, got)
    return got[0]


@pytest.mark.parametrize("nbits", [512, 1024, 2048, 3072])
def test_layouts_agree_over_the_sweep(nbits):
    fits = 0
    for kappa in (1, 40, 62):
        for ib in (1, 10, 32):
            f, g, M, rw = _three(nbits, kappa, ib, 1, 1)
            assert f == ib + kappa + 1 and M == 1 and rw == -(-(ib + kappa) // 32)
            assert g * f < nbits - 1 <= (g + 1) * f                 # g is maximal
            for k in (1, 2, 3, 1000, 1024):
                for m in sorted({1, g - 1, g, g + 1, 2 * g + 1} - {0}):
                    got = _three(nbits, kappa, ib, k, m)
                    assert got == (f, g, -(-m // g), rw), (kappa, ib, k, m)
                    fits += 1
    assert fits >= 3 * 3 * 5 * 4


def test_refusals_agree_and_name_the_quantity():
    from protocols.secure_comparison_amd import OnehotLayout

    for nbits, kappa, ib, k, m in ((2048, 0, 8, 4, 1), (2048, 63, 8, 4, 1), (2048, 40, 0, 4, 1), (2048, 40, 33, 4, 1), (2048, 40, 8, 0, 1),
                                   (2048, 40, 8, 1025, 1), (2048, 40, 8, 4, 0), (2048, 40, 8, 4, 65537), (96, 62, 32, 4, 1), (52, 40, 10, 4, 1)):
        assert _three(nbits, kappa, ib, k, m) is None, (nbits, kappa, ib, k, m)
    # the fit rule one bit either side: f = 95 needs f < nbits - 1
    assert _three(96, 62, 32, 4, 1) is None and _three(97, 62, 32, 4, 3) == (95, 1, 3, 3)
    assert _three(52, 40, 10, 4, 1) is None and _three(53, 40, 10, 4, 1) == (51, 1, 1, 2)
    assert _three(128, 62, 32, 1024, 1) == (95, 1, 1, 3)            # every key of 128 bits and up takes the widest field
    for kw, what in ((dict(kappa=63), "kappa"), (dict(ib=33), "ib = 33"), (dict(k=0), "k = 0"), (dict(k=1025), "k = 1025"), (dict(m=0), "m = 0"),
                     (dict(kappa=62, ib=32, nbits=96), "f = 95")):
        args = dict(kappa=40, ib=8, k=4, m=1, nbits=2048)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            OnehotLayout(**args)


@pytest.mark.parametrize("nbits,kappa,ib", [(512, 40, 10), (1024, 62, 32), (2048, 40, 3), (3072, 1, 1), (97, 62, 32)])
def test_no_two_fields_of_a_message_overlap(nbits, kappa, ib):
    from protocols.secure_comparison_amd import OnehotLayout

    g = OnehotLayout(kappa, ib, 5, 1, nbits).g
    for m in sorted({1, 2, g - 1, g, g + 1, 2 * g, 2 * g + 1} - {0}):
        lay = OnehotLayout(kappa, ib, 5, m, nbits)
        where = [lay.position(q) for q in range(m)]
        assert where == [model.position(q, g) for q in range(m)]
        assert len(set(where)) == m
        for mm in range(lay.M):
            held = sorted(t for msg, t in where if msg == mm)
            assert held == list(range(len(held))) and 1 <= len(held) <= g           # positions 0 .. n_mm - 1, no holes
            assert len(held) == g or mm == lay.M - 1                                # only the last message may be partial
            spans = [(t * lay.f, (t + 1) * lay.f) for t in held]
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] < nbits - 1
            assert model.members(mm, m, g) == [mm * g + t for t in held]
        # a field holds i + r with no carry into the next one: 2^ib - 1 + 2^(ib + kappa) - 1 < 2^f
        assert (1 << ib) - 1 + (1 << (ib + kappa)) - 1 < 1 << lay.f
    with pytest.raises(ValueError):
        OnehotLayout(kappa, ib, 5, 3, nbits).position(3)


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------
class RecordingEngine(OracleEngine):
    """The CPU stand-in engine, keeping (kind, bits or n, count, nonzero) of every generator call."""

    def __init__(self, key=KEY):
        super().__init__()
        self.calls = []
        self.rng_seed(key)

    def rng_bits(self, bits, count):
        self.calls.append(("bits", bits, count, False))
        return super().rng_bits(bits, count)

    def rng_below(self, n, count, nonzero=False):
        self.calls.append(("below", n, count, bool(nonzero)))
        return super().rng_below(n, count, nonzero)


def _ints(eng, t):
    return eng.download(t.reshape(-1, t.shape[-1]))


@pytest.mark.parametrize("kappa,ib,k,m", [(40, 10, 7, 1), (40, 10, 3, 11), (62, 32, 5, 6), (1, 1, 2, 3), (40, 24, 1000, 1)])
def test_draw_onehot_against_the_replay(sk, kappa, ib, k, m):
    """Alice: r as m count items of ib + kappa bits, index q of row b at item q count + b; rho_p as M count items in [1, N), message mm
    of row b at item mm count + b.  Bob: m k count bases, (q, t, b) at item (q k + t) count + b.  Rows of exactly ceil(bits / 32) words."""
    from protocols.secure_comparison_amd import OnehotLayout, Paillier, draw_onehot

    count, n = 3, sk.n
    eng = RecordingEngine()
    pai = Paillier(sk.n, engine=eng)
    lay = OnehotLayout(kappa, ib, k, m, n.bit_length())
    M, nw = lay.M, (n.bit_length() + 31) // 32
    rp = dr.Replay(KEY)
    for alice, bob in ((True, True), (True, False), (False, True)):
        got = draw_onehot(count, lay, pai, alice=alice, bob=bob)
        if alice:
            r = rp.bits(ib + kappa, m * count, range(m * count))
            rho_p = rp.below(n, M * count, True, range(M * count))
        if bob:
            rho_e = rp.below(n, m * k * count, True, range(m * k * count))
        assert eng.calls == rp.log and eng._rng_call == rp.call
        if alice:
            assert tuple(got.r.shape) == (m, count, (ib + kappa + 31) // 32) and _ints(eng, got.r) == r
            assert eng.download(got.r[m - 1])[count - 1] == r[(m - 1) * count + count - 1]              # index-major
            assert tuple(got.rho_p.shape) == (M, count, nw) and _ints(eng, got.rho_p) == rho_p and all(1 <= v < n for v in rho_p)
        else:
            assert got.r is None and got.rho_p is None
        if bob:
            assert tuple(got.rho_e.shape) == (m, k, count, nw) and _ints(eng, got.rho_e) == rho_e
            assert eng.download(got.rho_e[m - 1][k - 1])[count - 1] == rho_e[((m - 1) * k + k - 1) * count + count - 1]     # [q][t][b]
        else:
            assert got.rho_e is None
    assert [c[0] for c in eng.calls] == ["bits", "below", "below", "bits", "below", "below"]      # both players, Alice alone, Bob alone


def test_no_two_indices_share_a_mask(sk):
    """4096 rows of m = 5 indices: the masks of a row are pairwise different, fill their range, and differ from row to row and from call
    to call (a mask shared by two indices of a row would hand the key holder i_p - i_q)."""
    from protocols.secure_comparison_amd import OnehotLayout, Paillier, draw_onehot

    rows, m, kappa, ib = 4096, 5, 40, 16
    eng = RecordingEngine()
    pai = Paillier(sk.n, engine=eng)
    lay = OnehotLayout(kappa, ib, 2, m, sk.n.bit_length())
    first, second = draw_onehot(rows, lay, pai, bob=False), draw_onehot(64, lay, pai)
    r = _ints(eng, first.r)
    top = 1 << (ib + kappa)
    assert len(r) == m * rows and all(0 <= x < top for x in r) and max(r) > 3 * top // 4
    assert len(set(r)) == len(r)                                    # 56-bit values: a repeat among 20480 is a shared mask, not chance
    for b in range(rows):
        assert len({r[q * rows + b] for q in range(m)}) == m, b
    rho = _ints(eng, first.rho_p)
    assert len(rho) == lay.M * rows and len(set(rho)) == len(rho) and min(rho) >= 1 and max(rho) < sk.n
    assert not set(_ints(eng, second.r)) & set(r) and not set(_ints(eng, second.rho_p)) & set(rho)
    rho_e = _ints(eng, second.rho_e)
    assert len(rho_e) == m * 2 * 64 and len(set(rho_e)) == len(rho_e) and not set(rho_e) & set(rho)


# ---- the header and chunked sessions ---------------------------------------------------------------------------------------------------------
class _OneMessage:
    """A communicator that hands over one prepared message and records what is sent."""

    def __init__(self, message):
        self.message, self.sent, self.device_tensors = message, [], True

    async def recv(self, other, msg_id=None):
        return self.message

    async def send(self, other, message, msg_id=None):
        self.sent.append(msg_id)


class _NoDecryption(OracleEngine):
    def keyholder_onehot(self, *a, **kw):
        raise AssertionError("the key holder decrypted before he compared the header")


def _stub_key_holder(sk, head, P):
    from protocols.secure_comparison_amd import Paillier, wire

    pai = Paillier(sk.n, engine=_NoDecryption())
    comm = _OneMessage(wire.DeviceArrays((head, P), None))

    async def open_session():
        return 1

    return types.SimpleNamespace(communicator=comm, scheme_paillier=pai, other_party="initiator", _open_batch_session=open_session), comm


@pytest.mark.parametrize("theirs", [dict(kappa=50), dict(index_bits=4), dict(k=8), dict(m=3)])
def test_key_holder_refuses_a_different_header(sk, theirs):
    from protocols.secure_comparison_amd import OnehotLayout
    from protocols.secure_comparison_amd.lookup import bob_onehot

    hers = OnehotLayout(40, 3, 7, 2, sk.n.bit_length())
    nw2 = 2 * ((sk.n.bit_length() + 31) // 32)
    head = torch.tensor(hers.header, dtype=torch.int32)
    kh, comm = _stub_key_holder(sk, head, torch.zeros((hers.M, 4, nw2), dtype=torch.int32))
    his = dict(k=7, m=2, index_bits=3, kappa=40)
    his.update(theirs)
    with pytest.raises(ValueError, match="announces"):
        asyncio.run(bob_onehot(kh, his["k"], his["m"], his["index_bits"], his["kappa"], None, "device", None))
    assert comm.sent == []
    # his own header passes the comparison and reaches the decryption
    kh, _ = _stub_key_holder(sk, head, torch.zeros((hers.M, 4, nw2), dtype=torch.int32))
    with pytest.raises(AssertionError, match="decrypted"):
        asyncio.run(bob_onehot(kh, 7, 2, 3, 40, types.SimpleNamespace(rho_e=torch.zeros((2, 7, 4, nw2 // 2), dtype=torch.int32)), "device", None))
    # a malformed announcement
    kh, _ = _stub_key_holder(sk, torch.tensor([40, 3, 7], dtype=torch.int32), torch.zeros((hers.M, 4, nw2), dtype=torch.int32))
    with pytest.raises(ValueError, match="malformed"):
        asyncio.run(bob_onehot(kh, 7, 2, 3, 40, None, "device", None))


def test_chunked_sessions_raise():
    from protocols.secure_comparison_amd import Initiator

    alice = Initiator(16)
    idx = torch.zeros((4, 32), dtype=torch.int32)
    with pytest.raises(ValueError, match="chunks"):
        asyncio.run(alice.perform_secure_onehot_batch(idx, 5, chunks=2))
    with pytest.raises(ValueError, match="chunks"):
        asyncio.run(alice.perform_secure_gather_batch(torch.zeros((5, 4, 32), dtype=torch.int32), idx.unsqueeze(0), 8, chunks=2))


def test_exports_and_bindings():
    import protocols.secure_comparison_amd as pkg
    from protocols.secure_comparison_amd import _lib, lookup

    for name in ("OnehotLayout", "OnehotDraws", "draw_onehot", "secure_onehot_batch", "secure_gather_batch", "secure_lookup_batch"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("onehot_pack", "onehot_answer", "onehot_finish", "onehot_batch"):
        assert hasattr(lookup, name)
    for name in ("sc_onehot_prep", "sc_onehot_split", "sc_onehot_rotate", "sc_onehot_layout", "sc_initiator_onehot_pack", "sc_keyholder_onehot",
                 "sc_initiator_onehot_finish"):
        assert name in _lib.SYMBOLS
    for cls in (pkg.Initiator, pkg.KeyHolder):
        assert hasattr(cls, "perform_secure_onehot_batch") and hasattr(cls, "perform_secure_gather_batch")
    assert pkg.OnehotLayout(40, 10, 1000, 3, 2048).header == [40, 10, 1000, 3]
    assert lookup.default_index_bits(1) == 1 and lookup.default_index_bits(2) == 1 and lookup.default_index_bits(3) == 2
    assert lookup.default_index_bits(1000) == 10 and lookup.default_index_bits(1024) == 10

"""The announced exchange under the four families' player halves, without a GPU: a stub engine whose pack / answer / finish entries return
zero arrays of the right shapes and record that they ran, stub players whose comparison session is one stand-in message, and a recording
communicator.  The transcript of both halves of every family -- sender, message id, arrays, shapes, dtypes, header -- is held to a literal;
the key holder refuses a header that differs in any one field, or whose length is outside his family's range, before he draws, decrypts or
sends; sort and top-m run their sub-batches under `session_{sid}_sort_{i}` / `session_{sid}_topk_{i}` and refuse a sub-batch of the wrong
size.

The stub key has 256 bits, so that a row takes two messages and the last one is partial: one-hot k = 3 at ib = 2, kappa = 40 has fields of
43 bits, g = 5 of them per message, and m = 6 indices take M = 2 messages (5 + 1); the inner product at 8-bit operands has pairs of 98 bits,
g = 2, and k = g + 1 = 3 pairs take M = 2 messages (2 + 1)."""
import asyncio
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _oracle_engine import OracleEngine  # noqa: E402

KEY = bytes((7 * i + 3) & 0xFF for i in range(32))
N = (1 << 255) | 0x1234567_89ABCDEF_0F1E2D3C_4B5A6978 | 1           # any odd 256-bit integer: the stub never computes with it
NW, NW2 = 8, 16
B, L, KAPPA = 3, 16, 40
I32 = "torch.int32"


def _z(*shape):
    return torch.zeros(shape, dtype=torch.int32)


class StubEngine(OracleEngine):
    """Every scheme-level entry of the four families as zeros of the shape the library returns; `called` keeps their names in order."""

    def __init__(self):
        super().__init__()
        self.called = []
        self.rng_seed(KEY)

    def initiator_select_d(self, key, z_enc, r):
        return _z(z_enc.shape[0], NW2)

    def paillier_one_minus(self, key, c):
        return torch.zeros_like(c)

    def initiator_cx_differences(self, key, kappa, widths, f_enc, g_enc, d_key):
        return _z(len(widths), d_key.shape[0], NW2)

    def initiator_select_pack(self, key, kappa, widths, sigma_enc, d_enc, r_a, r_b, rho_p, ew):
        self.called.append("select_pack")
        nf, count = len(widths), sigma_enc.shape[0]
        return _z(count, NW2), _z(nf, count, ew), _z(nf, count, NW)

    def keyholder_select_mult(self, key, kappa, widths, P, rho_products):
        self.called.append("select_answer")
        return _z(len(widths), P.shape[0], NW2)

    def initiator_select_finish(self, key, kappa, widths, sigma_enc, d_enc, b_enc, products, r_a, e, rab):
        self.called.append("select_finish")
        return _z(len(widths), sigma_enc.shape[0], NW2)

    def initiator_cx_finish(self, key, kappa, widths, delta_enc, d_enc, f_enc, g_enc, products, r_a, e, rab, lo_index=None, hi_index=None,
                            out=None):
        self.called.append("cx_finish")
        return out

    def initiator_mul_pack(self, key, kappa, wx, wy, signed, x_enc, y_enc, r_a, r_b, rho_p, ew):
        self.called.append("mul_pack")
        nf, count = len(wy), x_enc.shape[0]
        return _z(count, NW2), _z(nf + 1, count, ew), _z(nf, count, NW)

    def keyholder_mul(self, key, kappa, wx, wy, P, rho_products):
        self.called.append("mul_answer")
        return _z(len(wy), P.shape[0], NW2)

    def initiator_mul_finish(self, key, kappa, wx, wy, x_enc, y_enc, products, e, rab, base=None, coef=1):
        self.called.append("mul_finish")
        return _z(len(wy), x_enc.shape[0], NW2)

    def initiator_dot_pack(self, key, kappa, wx, wy, signed, square, k, M, x_enc, y_enc, r_a, r_b, rho_p, ew):
        self.called.append("dot_pack")
        count = x_enc.shape[1]
        return _z(M, count, NW2), _z(k if square else 2 * k, count, ew), _z(count, NW)

    def keyholder_dot(self, key, kappa, wx, wy, square, k, M, P, rho_d):
        self.called.append("dot_answer")
        return _z(P.shape[1], NW2)

    def initiator_dot_finish(self, key, kappa, wx, wy, square, k, x_enc, y_enc, d_enc, e, S, base=None, coef=1):
        self.called.append("dot_finish")
        return _z(x_enc.shape[1], NW2)

    def initiator_onehot_pack(self, key, kappa, ib, k, m, M, index_enc, r, rho_p):
        self.called.append("onehot_pack")
        count = index_enc.shape[1]
        return _z(M, count, NW2), _z(m, count)

    def keyholder_onehot(self, key, kappa, ib, k, m, M, P, rho_e):
        self.called.append("onehot_answer")
        return _z(m, k, P.shape[1], NW2)

    def initiator_onehot_finish(self, key, kappa, ib, k, m, E, rot, out=None):
        self.called.append("onehot_finish")
        return torch.zeros_like(E)


class Recorder:
    """One endpoint of an in-memory transport; `log` (shared by both endpoints) keeps every message in the order it was sent as
    (sender, message id, number of arrays, [(shape, dtype)], the integers of a leading one-dimensional array -- the header -- or None)."""

    device_tensors = True

    def __init__(self, who, inner, log):
        self.who, self.inner, self.log = who, inner, log

    async def send(self, party, message, msg_id=None):
        arrays = message.arrays
        head = [int(v) for v in arrays[0].tolist()] if arrays[0].dim() == 1 else None
        self.log.append((self.who, msg_id, len(arrays), [(tuple(a.shape), str(a.dtype)) for a in arrays], head))
        await self.inner.send(party, message, msg_id=msg_id)

    async def recv(self, party, msg_id=None):
        return await self.inner.recv(party, msg_id=msg_id)


class Player:
    """What the families' coroutines use of an Initiator or a KeyHolder.  The comparison session is one stand-in message, `step_1_batch_{tag}`,
    of as many rows as the comparison has; the key holder's session returns that row count."""

    l_maximum_bit_length, scheme_dgk = L, None

    def __init__(self, who, other, inner, log):
        from protocols.secure_comparison_amd import Paillier

        self.engine = StubEngine()
        self.scheme_paillier = self._scheme_paillier = Paillier(N, engine=self.engine)
        self.communicator, self.other_party, self.session_id, self.who = Recorder(who, inner, log), other, 0, who

    async def _open_batch_session(self, *args):
        self.session_id += 1
        return self.session_id

    async def _batch_session(self, tag, *args, keep=None, **kw):
        from protocols.secure_comparison_amd import wire

        comm = self.communicator
        if self.who == "keyholder":
            (z,) = wire.incoming(await comm.recv(self.other_party, msg_id=f"step_1_batch_{tag}"), self.engine.device, expect=1)
            return z.shape[0]
        count = args[0].shape[0]
        await comm.send(self.other_party, wire.outgoing(comm, _z(count, NW2)), msg_id=f"step_1_batch_{tag}")
        if keep is not None:
            keep["z_enc"], keep["r"] = _z(count, NW2), _z(count, NW)
        return _z(count, NW2)


def _pair():
    from protocols.secure_comparison_amd import InMemoryCommunicator

    inner, log = InMemoryCommunicator(timeout_s=5.0), []
    return Player("initiator", "keyholder", inner, log), Player("keyholder", "initiator", inner.peer(), log), log


def _both(alice_half, bob_half):
    async def run():
        return await asyncio.gather(alice_half, bob_half)

    return asyncio.run(run())


# ---- 1. the transcript ---------------------------------------------------------------------------------------------------------------
DOT_K, ONEHOT_K, ONEHOT_M = 3, 3, 6


def _select(ini, kh):
    from protocols.secure_comparison_amd.selection import alice_minmax, bob_rounds

    return (alice_minmax(ini, _z(B, NW2), _z(B, NW2), object(), None, KAPPA, "device", None, None, 1, False),
            bob_rounds(kh, 1, None, None, KAPPA, "device", None, ()))


def _mul(ini, kh):
    from protocols.secure_comparison_amd.multiplication import alice_multiply, bob_multiply

    return (alice_multiply(ini, _z(B, NW2), _z(B, NW2), 8, 8, False, KAPPA, None, "device", None, None, 1),
            bob_multiply(kh, 8, 8, False, KAPPA, None, "device", None))


def _dot(ini, kh):
    from protocols.secure_comparison_amd.dotproduct import alice_dot, bob_dot

    return (alice_dot(ini, _z(DOT_K, B, NW2), _z(DOT_K, B, NW2), 8, 8, False, False, KAPPA, None, "device", None, None, 1),
            bob_dot(kh, DOT_K, 8, 8, False, False, KAPPA, None, "device", None))


def _onehot(ini, kh):
    from protocols.secure_comparison_amd.lookup import alice_onehot, bob_onehot

    return (alice_onehot(ini, _z(ONEHOT_M, B, NW2), ONEHOT_K, None, KAPPA, None, "device", None, None, 1),
            bob_onehot(kh, ONEHOT_K, ONEHOT_M, None, KAPPA, None, "device", None))


# Recorded with this stub on the commit before the families shared exchange.py; the shared exchange must reproduce it exactly.
TRANSCRIPT = {
    "select": (_select, [
        ("initiator", "step_1_batch_session_1", 1, [((3, 16), I32)], None),
        ("initiator", "select_1_batch_session_1", 2, [((2,), I32), ((3, 16), I32)], [40, 16]),
        ("keyholder", "select_2_batch_session_1", 1, [((1, 3, 16), I32)], None)],
        (["select_pack", "select_finish"], ["select_answer"])),
    "mul": (_mul, [
        ("initiator", "mul_1_batch_session_1", 2, [((5,), I32), ((3, 16), I32)], [40, 8, 0, 1, 8]),
        ("keyholder", "mul_2_batch_session_1", 1, [((1, 3, 16), I32)], None)],
        (["mul_pack", "mul_finish"], ["mul_answer"])),
    "dot": (_dot, [
        ("initiator", "dot_1_batch_session_1", 2, [((6,), I32), ((2, 3, 16), I32)], [40, 8, 8, 0, 0, 3]),
        ("keyholder", "dot_2_batch_session_1", 1, [((3, 16), I32)], None)],
        (["dot_pack", "dot_finish"], ["dot_answer"])),
    "onehot": (_onehot, [
        ("initiator", "onehot_1_batch_session_1", 2, [((4,), I32), ((2, 3, 16), I32)], [40, 2, 3, 6]),
        ("keyholder", "onehot_2_batch_session_1", 1, [((6, 3, 3, 16), I32)], None)],
        (["onehot_pack", "onehot_finish"], ["onehot_answer"])),
}


def test_the_shapes_take_two_messages_with_a_partial_last_one():
    from protocols.secure_comparison_amd import DotLayout, OnehotLayout

    dot, hot = DotLayout(KAPPA, 8, 8, DOT_K, nbits=N.bit_length()), OnehotLayout(KAPPA, 2, ONEHOT_K, ONEHOT_M, N.bit_length())
    assert N.bit_length() == 32 * NW and (dot.g, dot.M, DOT_K) == (2, 2, dot.g + 1) and (hot.g, hot.M) == (5, 2) and ONEHOT_M % hot.g == 1


@pytest.mark.parametrize("family", sorted(TRANSCRIPT))
def test_transcript(family):
    halves, want, (alice_calls, bob_calls) = TRANSCRIPT[family]
    ini, kh, log = _pair()
    _both(*halves(ini, kh))
    assert log == want
    assert ini.engine.called == alice_calls and kh.engine.called == bob_calls


# ---- 2. the refusals -----------------------------------------------------------------------------------------------------------------
def _key_holder_alone(family, head, P):
    """The key holder's half of `family` against one prepared announcement: (his exception or None, what he sent, his engine)."""
    from protocols.secure_comparison_amd import wire

    halves = TRANSCRIPT[family][0]
    ini, kh, log = _pair()
    alice_half, bob_half = halves(ini, kh)
    alice_half.close()

    async def run():
        inner = ini.communicator.inner
        if family == "select":
            await inner.send("keyholder", wire.DeviceArrays((_z(B, NW2),), None), msg_id="step_1_batch_session_1")
        await inner.send("keyholder", wire.DeviceArrays((head, P), None), msg_id=f"{family}_1_batch_session_1")
        try:
            await bob_half
        except ValueError as exc:
            return exc
        return None

    return asyncio.run(run()), log, kh.engine


def _announcement(family):
    """His own header and a P of his own shape, from the transcript."""
    _, want, _ = TRANSCRIPT[family]
    (_, _, _, shapes, head), = [e for e in want if e[1].startswith(f"{family}_1_")]
    return head, _z(*shapes[1][0])


def _refused_before_anything(got, log, eng, text):
    assert isinstance(got, ValueError) and text in str(got), got
    assert log == [] and eng.called == [] and eng._rng_call == 0          # nothing sent, nothing decrypted, nothing drawn


@pytest.mark.parametrize("family", sorted(TRANSCRIPT))
def test_key_holder_refuses_a_header_that_differs_in_one_field(family):
    head, P = _announcement(family)
    for i in range(len(head)):
        theirs = list(head)
        theirs[i] += 1
        got, log, eng = _key_holder_alone(family, torch.tensor(theirs, dtype=torch.int32), P)
        _refused_before_anything(got, log, eng, f"{family}: the initiator announces")
        assert str(theirs) in str(got) and str(head) in str(got)
    # his own header passes the comparison: he draws, answers and sends
    got, log, eng = _key_holder_alone(family, torch.tensor(head, dtype=torch.int32), P)
    assert got is None and [e[1] for e in log] == [f"{family}_2_batch_session_1"] and eng.called == [f"{family}_answer"] and eng._rng_call == 1


FIELDS = {"select": "kappa and widths", "mul": "(kappa, wx, signed, columns, widths)", "dot": "(kappa, wx, wy, signed, square, k)",
          "onehot": "(kappa, ib, k, m)"}


@pytest.mark.parametrize("family", sorted(TRANSCRIPT))
def test_the_refusal_names_the_fields(family):
    head, P = _announcement(family)
    got, _, _ = _key_holder_alone(family, torch.tensor([head[0] + 10, *head[1:]], dtype=torch.int32), P)
    assert f"{family}: the initiator announces {FIELDS[family]} {[head[0] + 10, *head[1:]]}, this key holder expects {head}" == str(got)


def _lengths():
    """(family, header length, whether that length reaches the comparison) at both ends of every family's accepted range."""
    from protocols.secure_comparison_amd.selection import MAX_FIELDS

    assert MAX_FIELDS == 4
    return [("select", 1 + MAX_FIELDS, True), ("select", 2 + MAX_FIELDS, False), ("mul", 4 + MAX_FIELDS, True), ("mul", 5 + MAX_FIELDS, False),
            ("dot", 5, False), ("dot", 7, False), ("onehot", 3, False), ("onehot", 5, False)]


@pytest.mark.parametrize("family,length,reaches", _lengths())
def test_header_lengths_at_the_ends_of_the_ranges(family, length, reaches):
    head, P = _announcement(family)
    theirs = (head + [1] * length)[:length]
    got, log, eng = _key_holder_alone(family, torch.tensor(theirs, dtype=torch.int32), P)
    _refused_before_anything(got, log, eng, f"{family}: the initiator announces" if reaches else f"{family}: malformed layout announcement")


@pytest.mark.parametrize("family", sorted(TRANSCRIPT))
def test_a_header_that_is_no_vector_is_malformed(family):
    head, P = _announcement(family)
    got, log, eng = _key_holder_alone(family, torch.tensor([head], dtype=torch.int32), P)
    _refused_before_anything(got, log, eng, f"{family}: malformed layout announcement")


# ---- 3. sort and top-m ---------------------------------------------------------------------------------------------------------------
SORT_K, SORT_B = 3, 2           # the smallest network with more than one layer


def _network_ids(word, opening, n):
    ids = [("initiator", opening)]
    for i in range(n):
        tag = f"session_1_{word}_{i}"
        ids += [("initiator", f"step_1_batch_{tag}"), ("initiator", f"select_1_batch_{tag}"), ("keyholder", f"select_2_batch_{tag}")]
    return ids


def test_sort_runs_its_sub_batches_under_sort_tags():
    from protocols.secure_comparison_amd.sorting import alice_sort, bob_sort, schedule_counts

    counts = schedule_counts(SORT_K, SORT_B, 65536)
    assert counts == [SORT_B] * 3
    ini, kh, log = _pair()
    _both(alice_sort(ini, _z(SORT_B, SORT_K, NW2), None, (), False, False, KAPPA, "device", None, None, 1, 65536),
          bob_sort(kh, SORT_K, (), False, KAPPA, "device", None, 65536))
    assert [(e[0], e[1]) for e in log] == _network_ids("sort", "sort_0_session_1", 3)
    assert log[0][2:] == (1, [((5,), I32)], [SORT_K, SORT_B, 65536, KAPPA, L])
    assert all(e[4] == [KAPPA, L] and e[3][1] == ((SORT_B, NW2), I32) for e in log if e[1].startswith("select_1_"))
    assert ini.engine.called == ["select_pack", "cx_finish"] * 3 and kh.engine.called == ["select_answer"] * 3


@pytest.mark.parametrize("m,only_last", [(2, False), (2, True)])
def test_topk_runs_its_sub_batches_under_topk_tags(m, only_last):
    from protocols.secure_comparison_amd.sorting import alice_topk, bob_topk, topk_counts

    counts = topk_counts(SORT_K, m, only_last, SORT_B, 65536)
    assert len(counts) > 1 and set(counts) == {SORT_B}
    ini, kh, log = _pair()
    _both(alice_topk(ini, _z(SORT_B, SORT_K, NW2), m, None, (), False, False, KAPPA, "device", None, None, 1, 65536, only_last),
          bob_topk(kh, SORT_K, m, (), False, KAPPA, only_last, "device", None, 65536))
    assert [(e[0], e[1]) for e in log] == _network_ids("topk", "topk_0_session_1", len(counts))
    assert log[0][2:] == (1, [((7,), I32)], [SORT_K, m, int(only_last), SORT_B, 65536, KAPPA, L])
    assert kh.engine.called == ["select_answer"] * len(counts)


@pytest.mark.parametrize("word", ["sort", "topk"])
def test_a_sub_batch_of_the_wrong_size_is_refused(word):
    """The opening header is his own; sub-batch 0 then carries one comparison more than the schedule has."""
    from protocols.secure_comparison_amd import wire
    from protocols.secure_comparison_amd.sorting import bob_sort, bob_topk

    ini, kh, log = _pair()
    head = [SORT_K, SORT_B, 65536, KAPPA, L] if word == "sort" else [SORT_K, 2, 0, SORT_B, 65536, KAPPA, L]

    async def run():
        inner = ini.communicator.inner
        await inner.send("keyholder", wire.DeviceArrays((torch.tensor(head, dtype=torch.int32),), None), msg_id=f"{word}_0_session_1")
        await inner.send("keyholder", wire.DeviceArrays((_z(SORT_B + 1, NW2),), None), msg_id=f"step_1_batch_session_1_{word}_0")
        if word == "sort":
            await bob_sort(kh, SORT_K, (), False, KAPPA, "device", None, 65536)
        else:
            await bob_topk(kh, SORT_K, 2, (), False, KAPPA, False, "device", None, 65536)

    with pytest.raises(ValueError, match=f"{word}: sub-batch 0 carries {SORT_B + 1} comparisons, the schedule has {SORT_B}"):
        asyncio.run(run())
    assert log == [] and kh.engine.called == []

"""The announced exchange under the two-player halves of the selection, the multiplication, the inner product and the one-hot encoding
(DESIGN.md §8h): `{name}_1_batch_{tag}` carries the initiator's layout as an int32 header and her packed P, `{name}_2_batch_{tag}` the key
holder's answer.  The key holder compares the announced header with the one his own arguments give before he decrypts, draws or sends, so
players that disagree fail loudly in either direction (a split kernel's flag alone catches only a P that is too wide for his layout).

A family passes what differs -- the message name, the header, the accepted header lengths, the shape of P and of the answer -- and keeps
its pack, its draws and its finish."""
from __future__ import annotations

import torch

from . import wire


def no_chunks(chunks) -> None:
    if int(chunks) != 1:
        raise ValueError("secure selection: chunks > 1 is not supported")


async def announce(ini, name: str, tag: str, layout_header: list[int], P: torch.Tensor, reply_shape: tuple[int, ...],
                   reply_what: str, reply_words: int | None = None) -> torch.Tensor:
    """The initiator's half: the header and P out, the key holder's answer back as [*reply_shape][2nw] (`reply_what` names it in a
    refusal).  reply_words: the answer's row width where it is not a Paillier ciphertext's (the division's DGK bits)."""
    comm, dev = ini.communicator, P.device
    head = torch.tensor(layout_header, dtype=torch.int32, device=dev)
    await comm.send(ini.other_party, wire.outgoing(comm, head, P), msg_id=f"{name}_1_batch_{tag}")
    (reply,) = wire.incoming(await comm.recv(ini.other_party, msg_id=f"{name}_2_batch_{tag}"), dev, expect=1)
    return wire.expect_array(reply, (*reply_shape, ini.scheme_paillier.mod_n2.nwords if reply_words is None else reply_words), reply_what)


async def receive_announced(kh, name: str, tag: str, header: list[int], fields: str, lengths: range, lead: tuple[int, ...],
                            count: int | None) -> tuple[torch.Tensor, int]:
    """The key holder's half up to his checked P [*lead][count][2nw]: ValueError "malformed" for a header that is no int32 vector of one
    of the `lengths` his family accepts, ValueError "announces" (`fields` names the entries) unless it is his own `header`.  count None:
    P's own row count.  lead: the axes of P before the rows, () or (M,)."""
    comm, pai = kh.communicator, kh.scheme_paillier
    head, P = wire.incoming(await comm.recv(kh.other_party, msg_id=f"{name}_1_batch_{tag}"), pai.engine.device, expect=2)
    if not isinstance(head, torch.Tensor) or head.dim() != 1 or head.shape[0] not in lengths:
        raise ValueError(f"{name}: malformed layout announcement")
    announced = [int(v) for v in head.cpu().tolist()]
    if announced != header:
        raise ValueError(f"{name}: the initiator announces {fields} {announced}, this key holder expects {header}")
    if count is None:
        if not isinstance(P, torch.Tensor) or P.dim() != len(lead) + 2:
            raise ValueError(f"{name}: P is not {'an [M]' if lead else 'a '}[B][words] array")
        count = P.shape[len(lead)]
    return wire.expect_array(P, (*lead, count, pai.mod_n2.nwords), "P"), count


async def answer(kh, name: str, tag: str, array: torch.Tensor) -> None:
    """The key holder's send."""
    comm = kh.communicator
    await comm.send(kh.other_party, wire.outgoing(comm, array), msg_id=f"{name}_2_batch_{tag}")

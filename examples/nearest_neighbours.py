"""Nearest neighbours under encryption on an MI355X: the squared Euclidean distances of B encrypted queries to k encrypted points,
then the m nearest of every query.

1. secure_squared_distance_batch: one row per (query, point) pair and one "pair" of the inner product per coordinate; the key holder
   answers with ONE ciphertext per row.
2. secure_topk_batch over the k distances of every query, the point's number travelling along as the index column.

Run:  python examples/nearest_neighbours.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import DGK, Paillier, secure_squared_distance_batch, secure_topk_batch  # noqa: E402
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(queries: int = 64, points: int = 16, dims: int = 8, bits: int = 8, nearest: int = 3) -> None:
    l = 2 * bits + (dims - 1).bit_length()                       # a squared distance is below dims 2^(2 bits)
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    rng = random.Random(7)
    q = [[rng.getrandbits(bits) for _ in range(dims)] for _ in range(queries)]
    p = [[rng.getrandbits(bits) for _ in range(dims)] for _ in range(points)]

    def encrypt(values):
        rho = uniform_below(n, len(values), e, nonzero=True)
        return alice_p.randomize_batch(alice_p.encrypt_raw_batch(e.upload(values, nw)), rho)

    # row b * points + t is the pair (query b, point t); plane j holds coordinate j of every row
    rows = queries * points
    x_enc = encrypt([q[r // points][j] for j in range(dims) for r in range(rows)]).reshape(dims, rows, -1)
    y_enc = encrypt([p[r % points][j] for j in range(dims) for r in range(rows)]).reshape(dims, rows, -1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dist = secure_squared_distance_batch(x_enc, y_enc, bits, alice_p, bob_p)                               # [rows][2nw]
    _, _, idx = secure_topk_batch(dist.reshape(queries, points, -1).contiguous(), nearest, l, alice_p, alice_d, bob_p, bob_d,
                                  return_indices=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got = e.download(bob_p.decrypt_raw_batch(idx.reshape(queries * nearest, -1).contiguous()))
    d2 = [[sum((a - b) ** 2 for a, b in zip(q[b_], p[t])) for t in range(points)] for b_ in range(queries)]
    ok = all(sorted(d2[b_])[:nearest] == [d2[b_][got[b_ * nearest + r]] for r in range(nearest)] for b_ in range(queries))
    print(f"[nearest] the {nearest} nearest of {points} points for {queries} queries in {dims} dimensions in {dt * 1e3:.0f} ms; all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

"""The label of the nearest neighbour under encryption on an MI355X: the squared distances of B encrypted queries to k encrypted
training points, the encrypted index of the nearest one, and the encrypted class label that index selects.

1. secure_squared_distance_batch: one row per (query, point) pair.
2. secure_argmin_batch over the k distances of every query: [[index of the nearest point]].
3. secure_lookup_batch: [[label[index]]] from the encrypted labels and the encrypted index -- a one-hot encoding of the index, then one
   inner product with the table.  Nobody learns which point was nearest.

Run:  python examples/label_lookup.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import DGK, Paillier, secure_argmin_batch, secure_lookup_batch, secure_squared_distance_batch  # noqa: E402
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(queries: int = 64, points: int = 12, dims: int = 8, bits: int = 8, classes: int = 5) -> None:
    l = 2 * bits + (dims - 1).bit_length()                       # a squared distance is below dims 2^(2 bits)
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    rng = random.Random(11)
    q = [[rng.getrandbits(bits) for _ in range(dims)] for _ in range(queries)]
    p = [[rng.getrandbits(bits) for _ in range(dims)] for _ in range(points)]
    label = [rng.randrange(classes) for _ in range(points)]
    label_bits = max(1, (classes - 1).bit_length())

    def encrypt(values):
        rho = uniform_below(n, len(values), e, nonzero=True)
        return alice_p.randomize_batch(alice_p.encrypt_raw_batch(e.upload(values, nw)), rho)

    # row b * points + t is the pair (query b, point t); plane j holds coordinate j of every row
    rows = queries * points
    x_enc = encrypt([q[r // points][j] for j in range(dims) for r in range(rows)]).reshape(dims, rows, -1)
    y_enc = encrypt([p[r % points][j] for j in range(dims) for r in range(rows)]).reshape(dims, rows, -1)
    table = encrypt([label[t] for t in range(points) for _ in range(queries)]).reshape(points, queries, -1)   # every query sees the same labels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dist = secure_squared_distance_batch(x_enc, y_enc, bits, alice_p, bob_p)                               # [rows][2nw]
    _, idx = secure_argmin_batch(dist.reshape(queries, points, -1).contiguous(), l, alice_p, alice_d, bob_p, bob_d)
    lab = secure_lookup_batch(table, idx.contiguous(), label_bits, alice_p, bob_p)                         # [queries][2nw]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got = e.download(bob_p.decrypt_raw_batch(lab))
    d2 = [[sum((a - b) ** 2 for a, b in zip(q[b_], p[t])) for t in range(points)] for b_ in range(queries)]
    ok = all(got[b_] == label[d2[b_].index(min(d2[b_]))] for b_ in range(queries))                         # ties go to the lowest index
    print(f"[label] the label of the nearest of {points} points for {queries} queries in {dims} dimensions in {dt * 1e3:.0f} ms; all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

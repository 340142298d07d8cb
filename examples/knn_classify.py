"""A k-nearest-neighbour classifier under encryption on an MI355X: the squared distances of B encrypted queries to k encrypted training
points, the labels of the m nearest, and the label most of them carry.  It continues nearest_neighbours.py and label_lookup.py.

1. secure_squared_distance_batch: one row per (query, point) pair.
2. secure_topk_batch over the k distances of every query with the encrypted label as payload: the m nearest labels.
3. secure_majority_batch: a one-hot encoding of the m labels, their sum per class, and the argmax of the counts:
   ([[class]], [[votes]]).  Ties go to the lowest class.  Nobody learns which points were near or how the others voted.

Run:  python examples/knn_classify.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import DGK, Paillier, secure_majority_batch, secure_squared_distance_batch, secure_topk_batch  # noqa: E402
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(queries: int = 64, points: int = 12, dims: int = 8, bits: int = 8, classes: int = 4, m: int = 5) -> None:
    l = 2 * bits + (dims - 1).bit_length()                       # a squared distance is below dims 2^(2 bits)
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    rng = random.Random(12)
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
    labels = encrypt([label[r % points] for r in range(rows)]).reshape(1, queries, points, -1)             # the payload column
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dist = secure_squared_distance_batch(x_enc, y_enc, bits, alice_p, bob_p)                               # [rows][2nw]
    _, near, _ = secure_topk_batch(dist.reshape(queries, points, -1).contiguous(), m, l, alice_p, alice_d, bob_p, bob_d,
                                   payload=labels, payload_bits=(label_bits,))                             # near: [1][queries][m][2nw]
    votes = near[0].permute(1, 0, 2).contiguous()                                                          # [m][queries][2nw]
    cls, cnt = secure_majority_batch(votes, classes, alice_p, alice_d, bob_p, bob_d, index_bits=label_bits)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got_cls, got_cnt = e.download(bob_p.decrypt_raw_batch(cls)), e.download(bob_p.decrypt_raw_batch(cnt))
    ok, checked = True, 0
    for b in range(queries):
        d2 = sorted((sum((a - c) ** 2 for a, c in zip(q[b], p[t])), t) for t in range(points))
        if m < points and d2[m - 1][0] == d2[m][0]:
            continue                                             # equal distances at the cut: which of them is among the m is the network's choice
        tally = [sum(1 for _, t in d2[:m] if label[t] == c) for c in range(classes)]
        ok = ok and got_cnt[b] == max(tally) and got_cls[b] == tally.index(max(tally))
        checked += 1
    print(f"[knn] the class of {queries} queries by the {m} nearest of {points} points in {dims} dimensions in {dt * 1e3:.0f} ms; "
          f"{checked} checked, all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

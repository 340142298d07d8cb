"""A linear classifier over encrypted features on an MI355X: B encrypted feature vectors, a public weight matrix with a bias for J
classes, the encrypted scores, and the encrypted label of the highest one.

1. linear_planes_batch: [[scores]] = W [[x]] + b, one launch of k_lin_axis over the K feature planes.  The model is
   public, the features are not; signed weights cost one batched inversion of the planes that carry a negative one.
2. secure_argmax_batch over the J scores of every row: ([[best score]], [[label]]).  The scores are shifted into
   0 .. 2^l - 1 by the bias first: the comparison orders non-negative l-bit values.  Ties go to the lowest label.

Run:  python examples/linear_score.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import DGK, Paillier, linear_planes_batch, secure_argmax_batch  # noqa: E402
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(rows: int = 64, features: int = 16, classes: int = 5, bits: int = 8, wbits: int = 8) -> None:
    rng = random.Random(7)
    W = [[rng.randrange(-(1 << wbits) + 1, 1 << wbits) for _ in range(features)] for _ in range(classes)]
    bias = [rng.randrange(-(1 << wbits), 1 << wbits) for _ in range(classes)]
    reach = max(sum(abs(w) for w in row) for row in W) * ((1 << bits) - 1) + (1 << wbits)     # |score| stays below it
    shift, l = reach, (2 * reach).bit_length()                                                  # score + shift in 0 .. 2^l - 1
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    x = [[rng.getrandbits(bits) for _ in range(rows)] for _ in range(features)]                 # plane k holds feature k of every row
    rho = uniform_below(n, features * rows, e, nonzero=True)
    x_enc = alice_p.randomize_batch(alice_p.encrypt_raw_batch(e.upload([v for plane in x for v in plane], nw)), rho).reshape(features, rows, -1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = linear_planes_batch(x_enc, W, alice_p, bias=[b + shift for b in bias], x_bits=bits)           # [classes][rows][2nw]
    top, label = secure_argmax_batch(scores.permute(1, 0, 2).contiguous(), l, alice_p, alice_d, bob_p, bob_d)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got_top, got_label = e.download(bob_p.decrypt_raw_batch(top)), e.download(bob_p.decrypt_raw_batch(label))
    ok = True
    for b in range(rows):
        s = [sum(w * x[k][b] for k, w in enumerate(row)) + bias[j] for j, row in enumerate(W)]
        ok = ok and got_top[b] == max(s) + shift and got_label[b] == s.index(max(s))
    print(f"[linear] the best of {classes} linear scores over {features} encrypted features for {rows} rows in {dt * 1e3:.0f} ms; all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

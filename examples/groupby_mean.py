"""The mean per group under encryption on an MI355X: B rows of an encrypted value and an encrypted group index, group sizes public.

1. secure_groupby_sum_batch inside secure_groupby_mean_batch: the one-hot encoding of the index, one multiplication batch, the sum over
   the rows: [[sum of the values of group t]].
2. The division of the k sums by the PUBLIC group sizes: the comparison's own steps on quotients and remainders that the
   kernel k_divmod_words computes on each side -- exact floor division, negative sums floor toward minus infinity like Python's //.
   (Group sizes that are themselves encrypted would need a division by an encrypted divisor, which the library does not have.)
3. secure_modulo_batch on the same sums: what the floor left over.

Run:  python examples/groupby_mean.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import (DGK, Paillier, secure_groupby_mean_batch, secure_groupby_sum_batch,  # noqa: E402
                                             secure_modulo_batch)
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(rows: int = 48, groups: int = 5, bits: int = 12) -> None:
    l = max(1, (rows - 1).bit_length())                          # the divisors are group sizes: at most `rows`
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    rng = random.Random(21)
    index = list(range(groups)) + [rng.randrange(groups) for _ in range(rows - groups)]
    values = [rng.randrange(-(1 << (bits - 1)), 1 << (bits - 1)) for _ in range(rows)]
    sizes = [index.count(t) for t in range(groups)]

    def encrypt(xs):
        rho = uniform_below(n, len(xs), e, nonzero=True)
        return alice_p.randomize_batch(alice_p.encrypt_raw_batch(e.upload([x % n for x in xs], nw)), rho)

    def decrypt(t):
        return [v - n if v > n // 2 else v for v in e.download(bob_p.decrypt_raw_batch(t.contiguous()))]

    v_enc, i_enc = encrypt(values), encrypt(index)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mean = secure_groupby_mean_batch(v_enc, i_enc, groups, bits, sizes, alice_p, bob_p, alice_d, bob_d, signed=True)     # [groups][2nw]
    sums = secure_groupby_sum_batch(v_enc, i_enc, groups, bits, alice_p, bob_p, signed=True)
    left = secure_modulo_batch(sums, sizes, bits + rows.bit_length(), alice_p, bob_p, alice_d, bob_d, signed=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    want = [sum(v for v, i in zip(values, index) if i == t) for t in range(groups)]
    ok = decrypt(mean) == [s // c for s, c in zip(want, sizes)] and decrypt(left) == [s % c for s, c in zip(want, sizes)]
    print(f"[mean] floor means of {groups} groups over {rows} rows in {dt * 1e3:.0f} ms: {decrypt(mean)}; all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

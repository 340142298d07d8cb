"""The cumulative distribution and the median of binned data under encryption on an MI355X: B rows of m encrypted values below k.

1. secure_cdf_batch: the one-hot encoding of every value (one round trip), summed over the values of a row into a
   histogram and then running-summed over the bins by the scan kernel: [[#{values <= t}]] for every bin t.
2. secure_histogram_median_batch: the number of bins whose cumulative count does not exceed the median's rank -- one comparison batch
   over (k - 1) B rows of bits(m) bits instead of a sorting network over the m values.
3. cumsum_rows_batch(exclusive=True) over the per-bin totals: the offset at which each bin would start in a sorted output.

Run:  python examples/histogram_median.py   (needs the GPU; builds nothing -- run `python -m protocols.secure_comparison_amd.build` first)
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from protocols.secure_comparison_amd import (DGK, Paillier, cumsum_rows_batch, secure_cdf_batch, secure_histogram_median_batch,  # noqa: E402
                                             sum_rows_batch)
from protocols.secure_comparison_amd.keygen import next_prime  # noqa: E402
from protocols.secure_comparison_amd.randomness import uniform_below  # noqa: E402


def main(rows: int = 32, values: int = 25, bins: int = 8) -> None:
    l = max(1, values.bit_length())                              # a count of at most `values`
    bob_p = Paillier.from_security_parameter(key_length=1024)   # small keys so that key generation takes seconds
    bob_d = DGK.from_security_parameter(v_bits=160, n_bits=1024, u=next_prime(1 << (l + 2)), full_decryption=False)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    e, n, nw = bob_p.engine, bob_p.public_key.n, bob_p.mod_n.nwords
    rng = random.Random(12)
    data = [[rng.randrange(bins) for _ in range(rows)] for _ in range(values)]

    rho = uniform_below(n, values * rows, e, nonzero=True)
    enc = alice_p.randomize_batch(alice_p.encrypt_raw_batch(e.upload([v for plane in data for v in plane], nw)), rho).reshape(values, rows, -1)
    dec = lambda t: e.download(bob_p.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cdf = secure_cdf_batch(enc, bins, alice_p, bob_p)                                                   # [bins][rows][2nw]
    median = secure_histogram_median_batch(enc, bins, alice_p, alice_d, bob_p, bob_d)                   # [rows][2nw]
    totals = sum_rows_batch(cdf, alice_p)                                                               # [bins][2nw]: over all rows
    offsets = cumsum_rows_batch(totals.unsqueeze(0), alice_p, exclusive=True)[0]                        # [bins][2nw]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    want_cdf = [sum(1 for q in range(values) if data[q][b] <= t) for t in range(bins) for b in range(rows)]
    want_median = [sorted(data[q][b] for q in range(values))[(values - 1) // 2] for b in range(rows)]
    per_bin = [sum(want_cdf[t * rows:(t + 1) * rows]) for t in range(bins)]
    ok = dec(cdf) == want_cdf and dec(median) == want_median and dec(offsets) == [sum(per_bin[:t]) for t in range(bins)]
    print(f"[median] distribution and median of {values} values in {bins} bins for {rows} rows in {dt * 1e3:.0f} ms; all correct: {ok}")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

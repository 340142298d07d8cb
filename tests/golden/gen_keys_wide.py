"""Generate the DGK key fixtures of the wide comparisons (tests/golden/keys_wide.json) with the repo's own oracle.

Run from the repo root:  python tests/golden/gen_keys_wide.py
Deterministic (seeded); u = next_prime(2^(l+2)) as in SC/keyholder.py:161-166, v_bits = 160: a 2048-bit key for l = 128, a
1024-bit and a 2048-bit key for l = 255 (the GPU tests and tools/gpu_wide_l.py).  The small keys of l = 65 / 96 are made in the tests.
These are TEST keys: the secret parts are public in this file on purpose.
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from oracle import sc_oracle as o  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "keys_wide.json")


def main() -> None:
    rng = random.Random(0x71DE5EED)
    keys = {}
    for name, v_bits, n_bits, l in (("dgk_2048_l128", 160, 2048, 128), ("dgk_1024_l255", 160, 1024, 255),
                                    ("dgk_2048_l255", 160, 2048, 255)):
        u = o.next_prime(1 << (l + 2))
        k = o.DGKKey.generate(v_bits, n_bits, u, rng)
        keys[name] = {"p": hex(k.p), "q": hex(k.q), "v_p": hex(k.v_p), "v_q": hex(k.v_q), "g": hex(k.g),
                      "h": hex(k.h), "u": hex(k.u), "t": v_bits, "l": l}
        print(name, flush=True)
    with open(OUT, "w") as f:
        json.dump(keys, f, indent=1)


if __name__ == "__main__":
    main()

"""Generate the Paillier keys that do not fill their words (tests/golden/keys_odd.json) with the repo's own oracle.

Run from the repo root:  python tests/golden/gen_keys_odd.py
Deterministic: key `paillier_<bits>` is oracle.sc_oracle.PaillierKey.generate(bits, random.Random(SEEDS[bits])), so p has bits // 2 bits
and q the rest (one more for an odd length).  Only p and q are stored, in hex, as in keys.json; tests/_odd_keys.py derives everything
else -- word counts, kernel configurations, the conditions each key meets -- from them.
These are TEST keys: the secret parts are public in this file on purpose.
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from oracle import sc_oracle as o  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "keys_odd.json")
SEEDS = {521: 521, 1025: 1025, 1040: 1040, 1041: 1041, 1100: 1100, 1540: 1540}


def generate(bits: int, seed: int):
    return o.PaillierKey.generate(bits, random.Random(seed))


def main() -> None:
    keys = {}
    for bits, seed in SEEDS.items():
        k = generate(bits, seed)
        keys[f"paillier_{bits}"] = {"bits": bits, "seed": seed, "p": hex(k.p), "q": hex(k.q)}
        print(bits, k.p.bit_length(), k.q.bit_length(), k.n2.bit_length(), flush=True)
    with open(OUT, "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

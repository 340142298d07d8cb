"""Two compare-exchange batches with a key and two payload columns (2048-bit keys), for a kernel trace of the second one:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gpu_cx_trace.py [--batch B] [--l L]
    python tools/cx_dispatches.py OUT/.../*_kernel_trace.csv

The first batch builds the programs and sizes the scratch; tools/cx_dispatches.py lists the dispatches of the second.
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--l", type=int, default=32)
    args = ap.parse_args()

    import torch

    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.schemes import default_engine
    from protocols.secure_comparison_amd.selection import SelectLayout
    from protocols.secure_comparison_amd.sorting import _cx_batch

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    pj, dj = keys["paillier_2048"], keys[{32: "dgk_2048_l32", 64: "dgk_2048_l64"}[args.l]]
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    e = default_engine()
    bob_p = Paillier(H(pj, "p") * H(pj, "q"), H(pj, "p"), H(pj, "q"), engine=e)
    bob_d = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
                engine=e, randomizer_bits=400)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    B, l, widths = args.batch, args.l, (12, 20)
    rng = random.Random(3)
    cols = lambda: torch.stack([alice_p.encrypt_raw_batch(e.upload([rng.getrandbits(w) for _ in range(B)], 2))  # noqa: E731
                                for w in (l, *widths)]).contiguous()
    f, g = cols(), cols()
    layout = SelectLayout(l, 40, widths, alice_p.public_key.n.bit_length())
    for _ in range(2):
        out = _cx_batch(layout, l, f, g, alice_p, alice_d, bob_p, bob_d)
        torch.cuda.synchronize()
    lo = e.download(bob_p.decrypt_raw_batch(out[0].reshape(-1, out.shape[-1])[:8].contiguous()))
    print(json.dumps({"B": B, "l": l, "payload_bits": widths, "lo_key_first_rows": lo}))


if __name__ == "__main__":
    main()

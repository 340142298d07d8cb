"""Rate of linear_planes_batch at 2048-bit keys against the route that existed before: Paillier.scalar_mul_batch per
plane followed by sum_planes_batch per output.

    python tools/gpu_linear_rate.py            # one JSON line per case

K = 64 planes, J = 16 outputs, B = 1024 rows; 16-bit and 64-bit non-negative weights.  Both routes run in one process, alternated, after
a warm-up of each; the median of five, wall time around a device synchronisation.  The two routes must agree bit for bit, and 16 rows of
each result are decrypted and checked against W x computed in Python.
"""
from __future__ import annotations

import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

K, J, B, TILE, REPS = 64, 16, 1024, 257, 5


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main() -> None:
    from protocols.secure_comparison_amd import Paillier, linear_planes_batch
    from protocols.secure_comparison_amd.aggregate import sum_planes_batch
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))
    pj = keys["paillier_2048"]
    p, q = int(pj["p"], 16), int(pj["q"], 16)
    n = p * q
    eng = default_engine()
    bp = Paillier(n, p, q, engine=eng)
    ap = bp.public_copy()
    nw = ap.mod_n.nwords
    rng = random.Random(11)
    plain = [rng.getrandbits(32) for _ in range(TILE)]
    base = ap.randomize_batch(ap.encrypt_raw_batch(eng.upload(plain, nw)), eng.upload([rng.randrange(1, n) for _ in plain], nw))
    x = base[torch.arange(K * B, device=base.device) % TILE].reshape(K, B, -1).contiguous()       # x[k][b] = plain[(k B + b) mod 257]
    dec = lambda t: eng.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    device = torch.cuda.get_device_name(eng.device)

    for wbits in (16, 64):
        W = [[rng.getrandbits(wbits) | 1 << (wbits - 1) for _ in range(K)] for _ in range(J)]
        scalars = [[eng.upload([w] * B, 2) for w in row] for row in W]                             # the per-row exponents the existing route needs

        def existing():
            return torch.stack([sum_planes_batch(torch.stack([ap.scalar_mul_batch(x[k], scalars[j][k], wbits) for k in range(K)]), ap) for j in range(J)])

        def kernel():
            return linear_planes_batch(x, W, ap)

        _once(kernel), _once(existing)                                                            # warm-up
        t_new, t_old = [], []
        for _ in range(REPS):
            ms, new = _once(kernel)
            t_new.append(ms)
            ms, old = _once(existing)
            t_old.append(ms)
        assert torch.equal(new, old)
        want = [sum(W[j][k] * plain[(k * B + b) % TILE] for k in range(K)) % n for j in range(J) for b in range(16)]
        assert dec(new[:, :16]) == want and dec(old[:, :16]) == want
        ms_new, ms_old = statistics.median(t_new), statistics.median(t_old)
        print(json.dumps({"case": "linear_planes_batch", "K": K, "J": J, "B": B, "weight_bits": wbits, "ms": round(ms_new, 3),
                          "scalar_mul_sum_ms": round(ms_old, 3), "ratio": round(ms_old / ms_new, 2), "outputs_per_s": round(J * B / ms_new * 1e3),
                          "device": device}), flush=True)


if __name__ == "__main__":
    main()

"""Rates of the sums along an axis at 2048-bit keys, each against the route that existed before: Paillier.add_batch.

    python tools/gpu_reduce_rate.py            # one JSON line per case

sum_planes_batch over k B = 65536 ciphertexts with k in {16, 256, 1024} against k - 1 add_batch calls of B rows; sum_rows_batch of one
plane of 65536 rows against add_batch over halves (16 calls: the shortest add_batch route to one total; 65535 calls of one row would
only measure launches); secure_histogram_batch beside the secure_onehot_batch it contains.  Same process, after a warm-up, best of three,
wall time around a device synchronisation; the two routes must agree bit for bit and 16 results are decrypted and checked.
"""
from __future__ import annotations

import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TOTAL, TILE = 65536, 257


def _time(fn, reps=3):
    fn()
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3, out


def main() -> None:
    from protocols.secure_comparison_amd import Paillier, secure_histogram_batch, secure_onehot_batch
    from protocols.secure_comparison_amd.aggregate import sum_planes_batch, sum_rows_batch
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))["paillier_2048"]
    p, q = int(keys["p"], 16), int(keys["q"], 16)
    n = p * q
    eng = default_engine()
    bp = Paillier(n, p, q, engine=eng)
    ap = bp.public_copy()
    nw = ap.mod_n.nwords
    rng = random.Random(8)
    plain = [rng.getrandbits(32) for _ in range(TILE)]
    base = ap.randomize_batch(ap.encrypt_raw_batch(eng.upload(plain, nw)), eng.upload([rng.randrange(1, n) for _ in plain], nw))
    tiled = base[torch.arange(TOTAL, device=base.device) % TILE].contiguous()
    dec = lambda t: eng.download(bp.decrypt_raw_batch(t.contiguous()))  # noqa: E731
    device = torch.cuda.get_device_name(eng.device)

    for k in (16, 256, 1024):
        B = TOTAL // k
        x = tiled.reshape(k, B, -1)

        def chain():
            acc = ap.add_batch(x[0], x[1])
            for j in range(2, k):
                acc = ap.add_batch(acc, x[j])
            return acc

        ms_new, new = _time(lambda: sum_planes_batch(x, ap))
        ms_old, old = _time(chain)
        assert torch.equal(new, old)
        assert dec(new[:16]) == [sum(plain[(j * B + b) % TILE] for j in range(k)) % n for b in range(16)]
        print(json.dumps({"case": "sum_planes_batch", "k": k, "B": B, "ms": round(ms_new, 3), "add_batch_ms": round(ms_old, 3),
                          "add_batch_calls": k - 1, "ratio": round(ms_old / ms_new, 2), "device": device}), flush=True)

    x = tiled.reshape(1, TOTAL, -1)

    def halves():
        acc = tiled
        while acc.shape[0] > 1:
            h = acc.shape[0] // 2
            acc = ap.add_batch(acc[:h].contiguous(), acc[h:].contiguous())
        return acc

    ms_new, new = _time(lambda: sum_rows_batch(x, ap))
    ms_old, old = _time(halves)
    assert torch.equal(new, old) and dec(new) == [sum(plain[i % TILE] for i in range(TOTAL)) % n]
    print(json.dumps({"case": "sum_rows_batch", "rows": TOTAL, "ms": round(ms_new, 3), "add_batch_ms": round(ms_old, 3), "add_batch_calls": 16,
                      "ratio": round(ms_old / ms_new, 2), "device": device}), flush=True)

    m, k, B = 8, 16, 512
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    i_t = ap.randomize_batch(ap.encrypt_raw_batch(eng.upload([v for r in idx for v in r], nw)),
                             eng.upload([rng.randrange(1, n) for _ in range(m * B)], nw)).reshape(m, B, -1).contiguous()
    ms_hot, _ = _time(lambda: secure_onehot_batch(i_t, k, ap, bp))
    ms_hist, hist = _time(lambda: secure_histogram_batch(i_t, k, ap, bp))
    assert dec(hist[:, 0]) == [sum(1 for qq in range(m) if idx[qq][0] == t) for t in range(k)]
    print(json.dumps({"case": "secure_histogram_batch", "m": m, "k": k, "B": B, "ms": round(ms_hist, 3), "onehot_ms": round(ms_hot, 3),
                      "device": device}), flush=True)


if __name__ == "__main__":
    main()

"""Rates of the running sums along an axis at 2048-bit keys, each against the route that existed before: Paillier.add_batch.

    python tools/gpu_scan_rate.py            # one JSON line per case

cumsum_planes_batch at (k, B) = (16, 4096), (256, 256), (1024, 64) against the k - 1 dependent add_batch calls of B rows that produce
the same k prefixes; cumsum_rows_batch over one plane of 65536 rows against the doubling route (log2 B rounds of add_batch on shifted
views: round s adds row b - 2^s to row b; add_batch is Engine.modmul modulo N^2, called here with its `out` argument so that no
route pays a copy of its results); secure_histogram_median_batch at m = 256, k = 16, B = 64 beside secure_median_batch over the
sorting network on the same data.  Same process, after a warm-up, best of three, wall time around a device synchronisation; the two
routes must agree bit for bit and 16 results are decrypted and checked.
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
    from protocols.secure_comparison_amd import DGK, Paillier, secure_histogram_median_batch, secure_median_batch
    from protocols.secure_comparison_amd.aggregate import cumsum_planes_batch, cumsum_rows_batch
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "keys.json")))
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    pj, dj = keys["paillier_2048"], keys["dgk_2048_l16"]
    p, q = H(pj, "p"), H(pj, "q")
    n = p * q
    eng = default_engine()
    bp = Paillier(n, p, q, engine=eng)
    bd = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
             engine=eng, randomizer_bits=400)
    ap, ad = bp.public_copy(), bd.public_copy()
    nw = ap.mod_n.nwords
    rng = random.Random(9)
    plain = [rng.getrandbits(32) for _ in range(TILE)]
    enc = lambda vals: ap.randomize_batch(ap.encrypt_raw_batch(eng.upload(vals, nw)), eng.upload([rng.randrange(1, n) for _ in vals], nw))  # noqa: E731
    base = enc(plain)
    tiled = base[torch.arange(TOTAL, device=base.device) % TILE].contiguous()
    dec = lambda t: eng.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    device = torch.cuda.get_device_name(eng.device)

    for k in (16, 256, 1024):
        B = TOTAL // k
        x = tiled.reshape(k, B, -1)

        def chain():
            out = torch.empty_like(x)
            out[0] = x[0]
            for j in range(1, k):
                eng.modmul(ap.mod_n2, out[j - 1], x[j], out=out[j])        # add_batch, written in place
            return out

        ms_new, new = _time(lambda: cumsum_planes_batch(x, ap))
        ms_old, old = _time(chain)
        assert torch.equal(new, old)
        assert dec(new[-1, :16]) == [sum(plain[(j * B + b) % TILE] for j in range(k)) % n for b in range(16)]
        print(json.dumps({"case": "cumsum_planes_batch", "k": k, "B": B, "ms": round(ms_new, 3), "add_batch_ms": round(ms_old, 3),
                          "add_batch_calls": k - 1, "ratio": round(ms_old / ms_new, 2), "device": device}), flush=True)

    x = tiled.reshape(1, TOTAL, -1)

    def doubling():
        acc, s = tiled, 1
        while s < TOTAL:
            nxt = acc.clone()
            eng.modmul(ap.mod_n2, acc[s:].contiguous(), acc[:TOTAL - s].contiguous(), out=nxt[s:])
            acc, s = nxt, 2 * s
        return acc

    ms_new, new = _time(lambda: cumsum_rows_batch(x, ap))
    ms_old, old = _time(doubling)
    assert torch.equal(new[0], old)
    at = [0, 1, 2, 255, 256, 257, 1000, 4095, 4096, 30000, 32767, 32768, 50000, 65533, 65534, 65535]
    assert dec(new[0][at]) == [sum(plain[i % TILE] for i in range(b + 1)) % n for b in at]
    print(json.dumps({"case": "cumsum_rows_batch", "rows": TOTAL, "ms": round(ms_new, 3), "add_batch_ms": round(ms_old, 3), "add_batch_calls": 16,
                      "ratio": round(ms_old / ms_new, 2), "device": device}), flush=True)

    m, k, B = 256, 16, 64
    idx = [[rng.randrange(k) for _ in range(B)] for _ in range(m)]
    i_t = enc([v for r in idx for v in r]).reshape(m, B, -1).contiguous()
    rows = i_t.permute(1, 0, 2).contiguous()
    ms_hist, ours = _time(lambda: secure_histogram_median_batch(i_t, k, ap, ad, bp, bd))
    ms_sort, theirs = _time(lambda: secure_median_batch(rows, 4, ap, ad, bp, bd)[0])
    want = [sorted(idx[qq][b] for qq in range(m))[(m - 1) // 2] for b in range(B)]
    assert dec(ours) == dec(theirs) == want
    print(json.dumps({"case": "secure_histogram_median_batch", "m": m, "k": k, "B": B, "ms": round(ms_hist, 3), "secure_median_batch_ms": round(ms_sort, 3),
                      "ratio": round(ms_sort / ms_hist, 2), "device": device}), flush=True)


if __name__ == "__main__":
    main()

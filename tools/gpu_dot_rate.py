"""Secure inner products per second, 2048-bit Paillier keys, beside the composition they replace:

    python tools/gpu_dot_rate.py [--pairs 65536] [--bits 32] [--kappa 40] [--check 16]

One run measures (both players in one process, device-side draws, one timed call each after a warm-up on 64 rows), with k B = --pairs:
secure_dot_batch at k = 14 and k = 64 and secure_squared_distance_batch at k = 64.  The yardstick, in the same process, is the
way to the same ciphertext without the inner product: k calls of secure_multiply_batch on B rows, then add_batch.  One JSON line; K rows
of every result are decrypted and checked against Python.  DESIGN.md §8g holds the cost model these figures are compared with.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--kappa", type=int, default=40)
    ap.add_argument("--check", type=int, default=16)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import (Paillier, secure_dot_batch, secure_multiply_batch, secure_squared_distance_batch)
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    w, K, kappa = args.bits, args.check, args.kappa
    pj = keys["paillier_2048"]
    p, q = int(pj["p"], 16), int(pj["q"], 16)
    sk = o.PaillierKey(p * q, p, q)
    e = default_engine()
    bp = Paillier(sk.n, sk.p, sk.q, engine=e)
    ap_ = bp.public_copy()
    n = sk.n
    rng = random.Random(13)
    dec = lambda t: e.download(bp.decrypt_raw_batch(t[:K].contiguous()))  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    def composition(x_t, y_t):
        """The same sum from the multiplication alone: k round trips of B rows, then k - 1 additions."""
        acc = None
        for j in range(x_t.shape[0]):
            prod = secure_multiply_batch(x_t[j], y_t[j], w, w, ap_, bp, kappa=kappa)
            acc = prod if acc is None else ap_.add_batch(acc, prod)
        return acc

    out, ok = {}, {}
    for k in (14, 64):
        B = args.pairs // k
        xs = [[rng.getrandbits(w) for _ in range(B)] for _ in range(k)]
        ys = [[rng.getrandbits(w) for _ in range(B)] for _ in range(k)]
        up = lambda cols: ap_.encrypt_raw_batch(e.upload([v for c in cols for v in c], (w + 31) // 32)).reshape(k, B, -1).contiguous()  # noqa: E731
        x_t, y_t = up(xs), up(ys)
        xw, yw = x_t[:, :64].contiguous(), y_t[:, :64].contiguous()
        secure_dot_batch(xw, yw, w, w, ap_, bp, kappa=kappa)
        composition(xw[:2], yw[:2])
        dot, t_dot = timed(lambda: secure_dot_batch(x_t, y_t, w, w, ap_, bp, kappa=kappa))
        comp, t_comp = timed(lambda: composition(x_t, y_t))
        want = [sum(xs[j][i] * ys[j][i] for j in range(k)) % n for i in range(K)]
        ok[f"dot_k{k}"] = dec(dot) == want
        ok[f"composition_k{k}"] = dec(comp) == want
        out[f"k{k}"] = {"rows": B, "dot_s": round(t_dot, 3), "composition_s": round(t_comp, 3), "gain": round(t_comp / t_dot, 2),
                        "dot_rows_per_s": round(B / t_dot), "dot_pairs_per_s": round(k * B / t_dot), "composition_pairs_per_s": round(k * B / t_comp)}
        if k == 64:
            secure_squared_distance_batch(xw, yw, w, ap_, bp, kappa=kappa)
            dist, t_dist = timed(lambda: secure_squared_distance_batch(x_t, y_t, w, ap_, bp, kappa=kappa))
            ok["distance_k64"] = dec(dist) == [sum((xs[j][i] - ys[j][i]) ** 2 for j in range(k)) % n for i in range(K)]
            out["distance_k64"] = {"rows": B, "seconds": round(t_dist, 3), "rows_per_s": round(B / t_dist), "pairs_per_s": round(k * B / t_dist)}
    print(json.dumps({"pairs": args.pairs, "bits": w, "kappa": kappa, "keys": "2048", **out,
                      "checked": {k: "ok" if v else "FAIL" for k, v in ok.items()}}), flush=True)
    if not all(ok.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

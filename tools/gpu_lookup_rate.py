"""Secure one-hot encodings and table lookups per second, 2048-bit Paillier keys, beside the composition they replace:

    python tools/gpu_lookup_rate.py [--cells 65536] [--bits 32] [--kappa 40] [--check 16] [--composition-rows 256]

One run measures (both players in one process, device-side draws, one timed call each after a warm-up on 64 rows), with k B = --cells:
secure_onehot_batch and secure_lookup_batch at k = 16 and k = 256.  The yardstick, in the same process, is the way to the same ciphertext
without the one-hot: k calls of secure_equal_batch against the public positions 0 .. k - 1, then secure_dot_batch with the table -- at
--composition-rows rows, a size that finishes, so its figure is a rate per row and not a time for the same batch.  One JSON line; K rows
of every result are decrypted and checked against Python.  DESIGN.md §8i holds the cost model these figures are compared with.
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
    ap.add_argument("--cells", type=int, default=65536)
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--kappa", type=int, default=40)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--composition-rows", type=int, default=256)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import (DGK, Paillier, secure_dot_batch, secure_equal_batch, secure_lookup_batch, secure_onehot_batch)
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    w, K, kappa = args.bits, args.check, args.kappa
    pj, dj = keys["paillier_2048"], keys["dgk_2048_l16"]
    p, q = int(pj["p"], 16), int(pj["q"], 16)
    sk = o.PaillierKey(p * q, p, q)
    e = default_engine()
    bp = Paillier(sk.n, sk.p, sk.q, engine=e)
    ap_ = bp.public_copy()
    dp, dq = int(dj["p"], 16), int(dj["q"], 16)
    bd = DGK(dp * dq, int(dj["g"], 16), int(dj["h"], 16), int(dj["u"], 16), dj["t"], dp, dq, int(dj["v_p"], 16), int(dj["v_q"], 16), engine=e)
    ad = bd.public_copy()
    n, nw = sk.n, bp.mod_n.nwords
    rng = random.Random(17)
    dec = lambda t: e.download(bp.decrypt_raw_batch(t.reshape(-1, t.shape[-1])[:K].contiguous()))  # noqa: E731
    up = lambda vals: ap_.encrypt_raw_batch(e.upload(vals, nw))  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    def composition(table_t, idx_t, k):
        """The same ciphertext from k equalities and a dot: [[ [i == t] ]] for every public t, then the inner product with the table."""
        rows = idx_t.shape[0]
        planes = [secure_equal_batch(idx_t, up([t] * rows), 16, ap_, ad, bp, bd, kappa=kappa)[0] for t in range(k)]
        return secure_dot_batch(table_t, torch.stack(planes).contiguous(), w, 1, ap_, bp, kappa=kappa)

    out, ok = {}, {}
    for k in (16, 256):
        B, C = args.cells // k, min(args.composition_rows, args.cells // k)
        idx = [rng.randrange(k) for _ in range(B)]
        table = [[rng.getrandbits(w) for _ in range(B)] for _ in range(k)]
        idx_t, table_t = up(idx), up([v for row in table for v in row]).reshape(k, B, -1).contiguous()
        secure_lookup_batch(table_t[:, :64].contiguous(), idx_t[:64].contiguous(), w, ap_, bp, kappa=kappa)
        oh, t_oh = timed(lambda: secure_onehot_batch(idx_t, k, ap_, bp, kappa=kappa))
        lk, t_lk = timed(lambda: secure_lookup_batch(table_t, idx_t, w, ap_, bp, kappa=kappa))
        comp, t_comp = timed(lambda: composition(table_t[:, :C].contiguous(), idx_t[:C].contiguous(), k))
        ok[f"onehot_k{k}"] = dec(oh[0]) == [1 if idx[b] == 0 else 0 for b in range(K)] and \
            dec(oh[:, 0]) == [1 if idx[0] == t else 0 for t in range(min(K, k))]
        ok[f"lookup_k{k}"] = dec(lk) == [table[idx[b]][b] for b in range(K)]
        ok[f"composition_k{k}"] = dec(comp) == [table[idx[b]][b] for b in range(K)]
        out[f"k{k}"] = {"rows": B, "onehot_s": round(t_oh, 3), "lookup_s": round(t_lk, 3), "onehots_per_s": round(B / t_oh), "lookups_per_s": round(B / t_lk),
                        "onehot_cells_per_s": round(k * B / t_oh), "composition_rows": C, "composition_s": round(t_comp, 3),
                        "composition_lookups_per_s": round(C / t_comp, 1), "gain": round((B / t_lk) / (C / t_comp), 1)}
    print(json.dumps({"cells": args.cells, "bits": w, "kappa": kappa, "keys": "2048", "n": n.bit_length(), **out,
                      "checked": {k: "ok" if v else "FAIL" for k, v in ok.items()}}), flush=True)
    if not all(ok.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

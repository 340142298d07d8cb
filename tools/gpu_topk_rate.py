"""Rows per second of the secure top-m against the full secure sort at the same k, 2048-bit Paillier and DGK keys:

    python tools/gpu_topk_rate.py [--shapes 16:4,64:8,256:8] [--l L] [--floor 4096] [--rows R] [--check K]

For every (k, m): secure_topk_batch(m) and secure_sort_batch over the same R rows of k values, l = 32 by default.  R is the smallest
row count at which every layer of both networks holds at least `floor` comparisons (R = ceil(floor / the thinnest layer), 4096 when
a layer is a single comparator) unless --rows fixes it.  The timed windows hold the device-side draws and the randomized protocol,
both players in one process, after a warm-up on a slice of 64 rows (programs, tables).  One JSON line per shape with the comparator
and layer counts, the rates, their ratio beside the comparator ratio, and the sizes of the top-m network's layers in comparisons;
K rows (default 16) of every result are decrypted and checked against Python.
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
    ap.add_argument("--shapes", default="16:4,64:8,256:8")
    ap.add_argument("--l", type=int, default=32)
    ap.add_argument("--floor", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--check", type=int, default=16)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.schemes import default_engine
    from protocols.secure_comparison_amd.sorting import batcher_network, secure_sort_batch, secure_topk_batch, topk_network

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    pj, dj = keys["paillier_2048"], keys[{32: "dgk_2048_l32", 64: "dgk_2048_l64"}[args.l]]
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    sk = o.PaillierKey(H(pj, "p") * H(pj, "q"), H(pj, "p"), H(pj, "q"))
    e = default_engine()
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=e)
    bob_d = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
                engine=e, randomizer_bits=400)
    players = (bob_p.public_copy(), bob_d.public_copy(), bob_p, bob_d)
    l, K = args.l, args.check
    rng = random.Random(7)
    dec = lambda t: e.download(bob_p.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    for shape in args.shapes.split(","):
        k, m = (int(x) for x in shape.split(":"))
        top, full = topk_network(k, m), batcher_network(k)
        thinnest = min(len(layer) for layer in top + full)
        R = args.rows or -(-args.floor // thinnest)
        rows = [[rng.choice([rng.getrandbits(l), 5]) for _ in range(k)] for _ in range(R)]
        v = players[0].encrypt_raw_batch(e.upload([x for r in rows for x in r], 2)).reshape(R, k, -1).contiguous()
        warm = v[:min(R, 64)].contiguous()
        secure_topk_batch(warm, m, l, *players)
        secure_sort_batch(warm, l, *players)
        (t_out, _, _), t_top = timed(lambda: secure_topk_batch(v, m, l, *players))
        (s_out, _, _), t_sort = timed(lambda: secure_sort_batch(v, l, *players))
        n = min(K, R)
        got_t, got_s = dec(t_out[:n]), dec(s_out[:n])
        ok_t = [got_t[b * m:(b + 1) * m] for b in range(n)] == [sorted(r)[:m] for r in rows[:n]]
        ok_s = [got_s[b * k:(b + 1) * k] for b in range(n)] == [sorted(r) for r in rows[:n]]
        c_top, c_full = sum(len(x) for x in top), sum(len(x) for x in full)
        print(json.dumps({
            "k": k, "m": m, "rows": R, "l": l, "keys": "2048/2048",
            "topk_comparators": c_top, "topk_layers": len(top), "sort_comparators": c_full, "sort_layers": len(full),
            "topk_rows_per_s": round(R / t_top, 1), "sort_rows_per_s": round(R / t_sort, 1),
            "topk_cx_per_s": round(R * c_top / t_top), "sort_cx_per_s": round(R * c_full / t_sort),
            "speedup": round(t_sort / t_top, 3), "comparator_ratio": round(c_full / c_top, 3),
            "seconds": {"topk": round(t_top, 3), "sort": round(t_sort, 3)},
            "topk_layer_comparisons": [R * len(layer) for layer in top],
            "checked": {"topk": "ok" if ok_t else "FAIL", "sort": "ok" if ok_s else "FAIL"}}), flush=True)
        del v, t_out, s_out


if __name__ == "__main__":
    main()

"""Compare-exchanges per second against minimums and comparisons per second, and sorts per second, 2048-bit Paillier and DGK keys:

    python tools/gpu_sort_rate.py [--batch B] [--sort-batch S] [--l L] [--reps R] [--check K]

B = 65536 and l = 32 by default.  The timed windows hold the device-side draws and the randomized protocol: the comparison alone
(secure_comparison_batch), the secure minimum (the comparison plus a selection) and the compare-exchange (the comparison plus one
selection that returns both min and max), each over B pairs; then whole sorts of S rows (default 4096) of k = 8 and k = 16 values,
with and without the index column.  One JSON line; K rows (default 64) of every result are decrypted and checked against Python.
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
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--sort-batch", type=int, default=4096)
    ap.add_argument("--l", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=64)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.batch import secure_comparison_batch
    from protocols.secure_comparison_amd.schemes import default_engine
    from protocols.secure_comparison_amd.selection import _comparison_draws, secure_minimum_batch
    from protocols.secure_comparison_amd.sorting import secure_compare_exchange_batch, secure_sort_batch

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    pj, dj = keys["paillier_2048"], keys[{32: "dgk_2048_l32", 64: "dgk_2048_l64"}[args.l]]
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    sk = o.PaillierKey(H(pj, "p") * H(pj, "q"), H(pj, "p"), H(pj, "q"))
    e = default_engine()
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=e)
    bob_d = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
                engine=e, randomizer_bits=400)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    B, S, l, K = args.batch, args.sort_batch, args.l, args.check
    rng = random.Random(7)
    xs = [rng.getrandbits(l) for _ in range(B)]
    ys = [x if i % 16 == 0 else rng.getrandbits(l) for i, x in enumerate(xs)]
    x_enc = alice_p.encrypt_raw_batch(e.upload(xs, 2))
    y_enc = alice_p.encrypt_raw_batch(e.upload(ys, 2))
    rows = {k: [[rng.choice([rng.getrandbits(l), 5]) for _ in range(k)] for _ in range(S)] for k in (8, 16)}
    v_enc = {k: alice_p.encrypt_raw_batch(e.upload([x for r in rows[k] for x in r], 2)).reshape(S, k, -1).contiguous() for k in rows}
    players = (alice_p, alice_d, bob_p, bob_d)

    def compare():
        d = _comparison_draws(B, l, *players)
        return secure_comparison_batch(x_enc, y_enc, l, *players, d)

    legs = [("compare", B, compare, 3),
            ("minimum", B, lambda: secure_minimum_batch(x_enc, y_enc, l, *players)[0], 3),
            ("compare_exchange", B, lambda: secure_compare_exchange_batch(x_enc, y_enc, l, *players), 3)]
    for k in (8, 16):
        for ind in (False, True):
            legs.append((f"sort_k{k}" + ("_indices" if ind else ""), S,
                         (lambda k=k, ind=ind: secure_sort_batch(v_enc[k], l, *players, return_indices=ind)), 1))
    out, times = {}, {}
    for name, _, fn, reps in legs:
        fn()                                   # warm-up: programs, tables, scratch
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(1, min(reps, args.reps))):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name], times[name] = res, sorted(ts)

    dec = lambda t: e.download(bob_p.decrypt_raw_batch(t.reshape(-1, t.shape[-1]).contiguous()))  # noqa: E731
    checks = {"minimum": dec(out["minimum"][:K]) == [min(x, y) for x, y in zip(xs[:K], ys[:K])],
              "compare_exchange": (dec(out["compare_exchange"][0][:K]) == [min(x, y) for x, y in zip(xs[:K], ys[:K])] and
                                   dec(out["compare_exchange"][1][:K]) == [max(x, y) for x, y in zip(xs[:K], ys[:K])])}
    for k in (8, 16):
        for ind in (False, True):
            name = f"sort_k{k}" + ("_indices" if ind else "")
            got_v = dec(out[name][0][:K])
            ok = [got_v[b * k:(b + 1) * k] for b in range(K)] == [sorted(r) for r in rows[k][:K]]
            if ind:
                got_i = dec(out[name][2][:K])
                ok = ok and all(rows[k][b][got_i[b * k + i]] == got_v[b * k + i] and sorted(got_i[b * k:(b + 1) * k]) == list(range(k))
                                for b in range(K) for i in range(k))
            checks[name] = ok
    med = {name: ts[len(ts) // 2] for name, ts in times.items()}
    size = {name: n for name, n, _, _ in legs}
    line = {"B": B, "sort_rows": S, "l": l, "keys": "2048/2048",
            "compare_per_s": round(B / med["compare"]), "minimum_per_s": round(B / med["minimum"]),
            "compare_exchange_per_s": round(B / med["compare_exchange"]),
            "cx_over_minimum": round(med["minimum"] / med["compare_exchange"], 3)}
    for name in med:
        if name.startswith("sort_"):
            line[name + "_rows_per_s"] = round(size[name] / med[name], 1)
    line["seconds"] = {name: [round(t, 4) for t in ts] for name, ts in times.items()}
    line["checked"] = {name: ("ok" if v else "FAIL") for name, v in checks.items()}
    print(json.dumps(line))


if __name__ == "__main__":
    main()

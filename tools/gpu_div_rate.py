"""Divisions per second beside comparisons per second at the same l, 2048-bit Paillier and DGK keys:

    python tools/gpu_div_rate.py [--batch B] [--reps R] [--check K]

B = 4096 by default, l in {8, 32, 64}.  Both routes run in one process, alternated rep by rep (division, comparison, division, ..),
and the median of R = 5 reps of each is reported.  A timed window holds the device-side draws and the randomized protocol of both
players: division.secure_divide_batch with a shared divisor d whose remainders have l bits (bits(d - 1) = l), and
batch.secure_comparison_batch at that l.  K rows (default 64) of each result are decrypted and checked against Python.  Then
k_divmod_words alone (sc_plain_divmod into outputs allocated beforehand), a pair of device events around every launch, over rows of the
words of N: the median launch's time and the bytes it moves.  One JSON line.

The timed inputs are unrandomized ciphertexts 1 + m N (encrypt_raw_batch): neither route's work depends on the ciphertext's value, and
both windows hold their own draws (draw_div inside secure_divide_batch, _comparison_draws), so the two routes are treated alike.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

DIVISORS = {8: 200, 32: (1 << 32) - 5, 64: (1 << 64) - 59}       # bits(d - 1) = l


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=64)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import DGK, Paillier, secure_divide_batch
    from protocols.secure_comparison_amd.batch import secure_comparison_batch
    from protocols.secure_comparison_amd.schemes import default_engine
    from protocols.secure_comparison_amd.selection import _comparison_draws

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    pj = keys["paillier_2048"]
    sk = o.PaillierKey(H(pj, "p") * H(pj, "q"), H(pj, "p"), H(pj, "q"))
    e = default_engine()
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=e)
    alice_p = bob_p.public_copy()
    B, K, x_bits = args.batch, args.check, 64
    rng = random.Random(11)
    dec = lambda t: e.download(bob_p.decrypt_raw_batch(t[:K].contiguous()))  # noqa: E731
    line = {"B": B, "keys": "2048/2048", "x_bits": x_bits, "reps": args.reps, "l": {}}

    for l, d in DIVISORS.items():
        assert max(1, (d - 1).bit_length()) == l
        dj = keys["dgk_2048_l64" if l > 32 else "dgk_2048_l32"]
        bob_d = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
                    engine=e, randomizer_bits=400)
        alice_d = bob_d.public_copy()
        xs = [rng.getrandbits(x_bits) for _ in range(B)]
        a = [rng.getrandbits(l) for _ in range(B)]
        b = [v if i % 16 == 0 else rng.getrandbits(l) for i, v in enumerate(a)]
        x_enc, a_enc, b_enc = (alice_p.encrypt_raw_batch(e.upload(v, 2)) for v in (xs, a, b))

        def divide():
            return secure_divide_batch(x_enc, d, x_bits, alice_p, bob_p, alice_d, bob_d)

        def compare():
            return secure_comparison_batch(a_enc, b_enc, l, alice_p, alice_d, bob_p, bob_d, _comparison_draws(B, l, alice_p, alice_d, bob_p, bob_d))

        routes = {"divide": divide, "compare": compare}
        out, times = {}, {name: [] for name in routes}
        for fn in routes.values():                      # warm-up: programs, tables, scratch
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in routes.items():             # alternated
                t0 = time.perf_counter()
                out[name] = fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        ok = dec(out["divide"]) == [x // d for x in xs[:K]] and dec(out["compare"]) == [int(u <= v) for u, v in zip(a[:K], b[:K])]
        line["l"][str(l)] = {"divisor": d, "divide_per_s": round(B / med["divide"]), "compare_per_s": round(B / med["compare"]),
                             "ratio": round(med["compare"] / med["divide"], 3),
                             "seconds": {name: [round(t, 4) for t in ts] for name, ts in times.items()}, "checked": "ok" if ok else "FAIL"}

    # k_divmod_words alone: rows of the words of N, divisors of 64 bits; bytes = dividend in, quotient out, divisor in, remainder out
    nw = bob_p.mod_n.nwords
    kernel = {}
    for count in (B, 65536):
        x = e.upload([rng.getrandbits(32 * nw) for _ in range(count)], nw)
        dv = e.upload_u64([rng.getrandbits(64) | 1 << 63 for _ in range(count)])
        q, rem = e.plain_divmod(x, dv)                  # warm-up; its outputs are reused below, so no timed call allocates
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
        e._sync_stream()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * 20)]
        for i in range(20):                             # one pair of events per launch: each difference is one kernel's time on the
            ev[2 * i].record()                          # stream, not the host's rate of issuing calls
            e._check(e.lib.sc_plain_divmod(e.ctx, P(x), nw, P(dv), count, P(q), P(rem)))
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        per = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(20))
        ms = per[len(per) // 2]
        nbytes = count * (2 * nw * 4 + 16)
        kernel[str(count)] = {"nw": nw, "ms_median": round(ms, 4), "ms_min": round(per[0], 4), "GB_per_s": round(nbytes / ms / 1e6, 1),
                              "rows_per_s": round(count / ms * 1e3)}
        e.ctx_synchronize()
    line["k_divmod_words"] = kernel
    print(json.dumps(line))
    if any(v["checked"] != "ok" for v in line["l"].values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

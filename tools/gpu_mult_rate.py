"""Secure multiplications and equality tests per second, 2048-bit Paillier and DGK keys, beside the selection and the comparison:

    python tools/gpu_mult_rate.py [--batch 65536] [--bits 32] [--kappa 40] [--check 16]

One run measures, over the same B rows (both players in one process, device-side draws, one timed call each after a warm-up on 64
rows): secure_multiply_batch with wx = wy = --bits; secure_equal_batch at l = --bits (ONE comparison batch of 2B rows, then one AND);
select_batch alone (one column of l bits, the selector and the difference of a real comparison) and secure_comparison_batch alone as
the yardsticks.  One JSON line; K rows of every result are decrypted and checked against Python.  DESIGN.md §8e holds the cost model
these figures are compared with.
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
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--kappa", type=int, default=40)
    ap.add_argument("--check", type=int, default=16)
    args = ap.parse_args()

    import torch

    from oracle import sc_oracle as o
    from protocols.secure_comparison_amd import DGK, Paillier, secure_equal_batch, secure_multiply_batch
    from protocols.secure_comparison_amd import selection as sel
    from protocols.secure_comparison_amd.batch import secure_comparison_batch
    from protocols.secure_comparison_amd.schemes import default_engine

    keys = json.load(open(os.path.join(GOLDEN, "keys.json")))
    l, B, K, kappa = args.bits, args.batch, args.check, args.kappa
    pj, dj = keys["paillier_2048"], keys[{32: "dgk_2048_l32", 64: "dgk_2048_l64", 16: "dgk_2048_l16"}[l]]
    H = lambda k, s: int(k[s], 16)  # noqa: E731
    sk = o.PaillierKey(H(pj, "p") * H(pj, "q"), H(pj, "p"), H(pj, "q"))
    e = default_engine()
    bp = Paillier(sk.n, sk.p, sk.q, engine=e)
    bd = DGK(H(dj, "p") * H(dj, "q"), H(dj, "g"), H(dj, "h"), H(dj, "u"), dj["t"], H(dj, "p"), H(dj, "q"), H(dj, "v_p"), H(dj, "v_q"),
             engine=e, randomizer_bits=400)
    ap_, ad = bp.public_copy(), bd.public_copy()
    players = (ap_, ad, bp, bd)
    rng = random.Random(11)
    xs = [rng.getrandbits(l) for _ in range(B)]
    ys = [x if i % 4 == 0 else rng.getrandbits(l) for i, x in enumerate(xs)]
    x_t = ap_.encrypt_raw_batch(e.upload(xs, (l + 31) // 32))
    y_t = ap_.encrypt_raw_batch(e.upload(ys, (l + 31) // 32))
    dec = lambda t: e.download(bp.decrypt_raw_batch(t[:K].contiguous()))  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0

    lay = sel.SelectLayout(l, kappa, (), sk.n.bit_length())
    w = slice(0, min(B, 64))
    xw, yw = x_t[w].contiguous(), y_t[w].contiguous()
    secure_multiply_batch(xw, yw, l, l, ap_, bp, kappa=kappa)
    secure_equal_batch(xw, yw, l, *players, kappa=kappa)
    dw, ddw = sel._compare(xw, yw, l, *players, None)
    sel.select_batch(lay, dw, ddw.unsqueeze(0), xw.unsqueeze(0), ap_, bp, sel.draw_select(xw.shape[0], lay, ap_))

    prod, t_mul = timed(lambda: secure_multiply_batch(x_t, y_t, l, l, ap_, bp, kappa=kappa))
    (eq, le, ge), t_eq = timed(lambda: secure_equal_batch(x_t, y_t, l, *players, kappa=kappa))
    delta, t_cmp = timed(lambda: secure_comparison_batch(x_t, y_t, l, *players, sel._comparison_draws(B, l, *players)))
    _, d = sel._compare(x_t, y_t, l, *players, None)
    d3, x3 = d.unsqueeze(0), x_t.unsqueeze(0)
    mx, t_sel = timed(lambda: sel.select_batch(lay, delta, d3, x3, ap_, bp, sel.draw_select(B, lay, ap_)))
    n = sk.n
    ok = {"multiply": dec(prod) == [x * y % n for x, y in zip(xs[:K], ys[:K])],
          "equal": dec(eq) == [int(x == y) for x, y in zip(xs[:K], ys[:K])] and dec(le) == [int(x <= y) for x, y in zip(xs[:K], ys[:K])]
          and dec(ge) == [int(y <= x) for x, y in zip(xs[:K], ys[:K])],
          "comparison": dec(delta) == [int(x <= y) for x, y in zip(xs[:K], ys[:K])],
          "select": dec(mx[0]) == [max(x, y) for x, y in zip(xs[:K], ys[:K])]}
    print(json.dumps({
        "batch": B, "bits": l, "kappa": kappa, "keys": "2048/2048",
        "multiplications_per_s": round(B / t_mul), "equalities_per_s": round(B / t_eq), "select_per_s": round(B / t_sel),
        "comparisons_per_s": round(B / t_cmp),
        "mult_vs_select": round(t_sel / t_mul, 3),
        "equal_expected_per_s": round(B / (2 * t_cmp + t_mul)),      # two comparisons' worth in one batch, plus one bit multiplication
        "seconds": {"multiply": round(t_mul, 3), "equal": round(t_eq, 3), "comparison": round(t_cmp, 3), "select": round(t_sel, 3)},
        "checked": {k: "ok" if v else "FAIL" for k, v in ok.items()}}), flush=True)


if __name__ == "__main__":
    main()

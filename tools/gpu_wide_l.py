"""Comparisons per second at l = 32, 64, 128 and 255 bits, 2048-bit Paillier and 2048-bit DGK (u = next_prime(2^(l+2))):

    python tools/gpu_wide_l.py [--lines 32,64,128,255] [--batch B] [--reps R] [--check K]

One line of JSON per l.  B = 65536 (16384 at l = 255, where the blinding launch alone takes seconds).  The timed window holds the
device-side draws of both players (batch.draw_alice / draw_bob) and the whole randomized batch (secure_comparison_batch, every
`.randomize()` of the protocol); the inputs x, y are uniform over the full l bits.  K rows per line (default 64) are checked
against the CPU oracle with the very draws the device made.  Keys: tests/golden/keys.json (l = 32, 64) and keys_wide.json (128, 255).
"""
import argparse
import json
import multiprocessing
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
RBITS = 400
DGK_KEYS = {32: ("keys.json", "dgk_2048_l32"), 64: ("keys.json", "dgk_2048_l64"), 128: ("keys_wide.json", "dgk_2048_l128"),
            255: ("keys_wide.json", "dgk_2048_l255")}


def _oracle_keys(l):
    from oracle import sc_oracle as o

    pj = json.load(open(os.path.join(GOLDEN, "keys.json")))["paillier_2048"]
    p, q = int(pj["p"], 16), int(pj["q"], 16)
    fname, name = DGK_KEYS[l]
    k = json.load(open(os.path.join(GOLDEN, fname)))[name]
    H = lambda s: int(k[s], 16)  # noqa: E731
    return o.PaillierKey(p * q, p, q), o.DGKKey(H("p") * H("q"), H("g"), H("h"), H("u"), k["t"], H("p"), H("q"), H("v_p"), H("v_q"))


def _oracle_row(args):
    from oracle import sc_oracle as o

    l, x_enc, y_enc, fields = args
    sk, dgk = _oracle_keys(l)
    return o.compare(x_enc, y_enc, l, sk, dgk, o.Draws(**fields), True)


def run_line(l, B, reps, check, pool):
    import random

    import torch

    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.batch import BatchDraws, draw_alice, draw_bob, secure_comparison_batch
    from protocols.secure_comparison_amd.limbs import ints_to_words
    from protocols.secure_comparison_amd.schemes import default_engine

    e = default_engine()
    sk, od = _oracle_keys(l)
    bob_p = Paillier(sk.n, sk.p, sk.q, engine=e)
    bob_d = DGK(od.n, od.g, od.h, od.u, od.t, od.p, od.q, od.v_p, od.v_q, engine=e, randomizer_bits=RBITS)
    alice_p, alice_d = bob_p.public_copy(), bob_d.public_copy()
    nw = bob_p.mod_n.nwords
    rng = random.Random(l)
    xs = [rng.randrange(1 << l) for _ in range(B)]
    ys = [xs[i] if i % 8 == 0 else rng.randrange(1 << l) for i in range(B)]
    x_enc = alice_p.encrypt_raw_batch(e.upload_words(ints_to_words(xs, nw)))
    y_enc = alice_p.encrypt_raw_batch(e.upload_words(ints_to_words(ys, nw)))

    def once():
        a, b = draw_alice(B, l, alice_p, alice_d), draw_bob(B, l, bob_p, bob_d)
        draws = BatchDraws(r=a.r, delta_a=a.delta_a, rhos=a.rhos, permutation=a.permutation, rho_z=a.rho_z, r_bob_dgk=b.r_bob_dgk,
                           r_alice_dgk=a.r_alice_dgk, rho_zeta_1=b.rho_zeta_1, rho_zeta_2=b.rho_zeta_2, rho_delta_b=b.rho_delta_b)
        return draws, secure_comparison_batch(x_enc, y_enc, l, alice_p, alice_d, bob_p, bob_d, draws)

    once()                                    # warm-up: programs built and uploaded, buffers sized
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        draws, res = once()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dec = bob_p.decrypt_raw_batch(res)
    expect = torch.tensor([int(x <= y) for x, y in zip(xs, ys)], dtype=torch.int32, device=dec.device)
    all_ok = bool(((dec[:, 0] == expect) & (dec[:, 1:] == 0).all(dim=1)).all().item())
    # the oracle rows: the device's own draws as Python integers (only the K sampled comparisons leave the device)
    rows = sorted(random.Random(1).sample(range(B), check))
    sel = torch.tensor(rows, dtype=torch.int64, device=res.device)
    D = lambda t: e.download(t.index_select(0, sel).contiguous())  # noqa: E731
    P = lambda t: [e.download(t[i].index_select(0, sel).contiguous()) for i in range(l + 1)]  # noqa: E731
    xe, ye, got = D(x_enc), D(y_enc), D(res)
    r, rz, z1, z2, zd = D(draws.r), D(draws.rho_z), D(draws.rho_zeta_1), D(draws.rho_zeta_2), D(draws.rho_delta_b)
    rhos, rb, ra = P(draws.rhos), P(draws.r_bob_dgk), P(draws.r_alice_dgk)
    da, perm = draws.delta_a.index_select(0, sel).tolist(), draws.permutation.index_select(0, sel).tolist()
    jobs = []
    for j in range(len(rows)):
        fields = dict(r=r[j], delta_a=da[j], rhos=[rhos[i][j] for i in range(l + 1)], perm=perm[j], rho_z=rz[j], r_d=rb[0][j],
                      r_beta=[rb[i][j] for i in range(1, l + 1)], r_c=[ra[perm[j][k]][j] for k in range(l + 1)],
                      rho_zeta1=z1[j], rho_zeta2=z2[j], rho_delta_b=zd[j])
        jobs.append((l, xe[j], ye[j], fields))
    want = list(pool.map(_oracle_row, jobs))
    equal = sum(int(g == w) for g, w in zip(got, want))
    best = min(times)
    return {"l": l, "B": B, "paillier_bits": 2048, "dgk_bits": 2048, "comparisons_per_s": round(B / best, 1), "best_s": round(best, 4),
            "all_s": [round(t, 4) for t in times], "all_rows_decrypt_ok": all_ok, "oracle_rows_equal": f"{equal}/{len(rows)}"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", default="32,64,128,255")
    ap.add_argument("--batch", type=int, default=0, help="B (default: 65536, 16384 at l = 255)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--check", type=int, default=64)
    args = ap.parse_args()
    ok = True
    # fresh interpreters for the oracle rows (never a fork of the process that drives the GPU); at most 16 CPUs are ours
    with ProcessPoolExecutor(max_workers=16, mp_context=multiprocessing.get_context("spawn")) as pool:
        for l in (int(v) for v in args.lines.split(",")):
            B = args.batch or (16384 if l == 255 else 65536)
            line = run_line(l, B, args.reps, args.check, pool)
            print(json.dumps(line), flush=True)
            ok = ok and line["all_rows_decrypt_ok"] and line["oracle_rows_equal"] == f"{args.check}/{args.check}"
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""The oracle side of the wrap-row table (tests/_wrap_rows.py), shared by its CPU and its GPU module: draws with a row's r and
delta_A planted, and oracle.compare with its trace for a list of rows -- in fresh worker processes where the Python integers
would take more than a few seconds in one (no worker touches a GPU)."""
import multiprocessing
import os
import random
from concurrent.futures import ProcessPoolExecutor

from oracle import sc_oracle as o

KEEP = ("z_enc", "z", "d_sent", "beta_enc", "c_enc", "delta_b", "zeta1", "zeta2", "delta_b_enc", "result")


# name -> (Paillier bits, l, committed DGK key or None = generated here for u = next_prime(2^(l+2)), randomizer bits)
WORLDS = {"1024_l16": (1024, 16, "dgk_1024_l16", 400), "tiny_l16": (1024, 16, "dgk_tiny_l16", 50), "l1": (1024, 1, None, 100),
          "l5": (1024, 5, None, 100), "2048_l32": (2048, 32, "dgk_2048_l32", 400), "l65": (1024, 65, None, 64), "l128": (1024, 128, None, 64)}
GPU_WORLDS = ("1024_l16", "l1", "l5", "2048_l32", "l65", "l128")


def world(keys, name):
    """(oracle Paillier key, oracle DGK key, l, randomizer bits) of a named case."""
    from conftest import oracle_dgk, oracle_paillier

    bits, l, dname, rbits = WORLDS[name]
    dgk = oracle_dgk(keys, dname) if dname else o.DGKKey.generate(40, 512, o.next_prime(1 << (l + 2)), random.Random(400 + l))
    return oracle_paillier(keys, bits), dgk, l, rbits


def planted_draws(rows, l, sk, dgk, rbits, seed, shuffle=True):
    """One oracle Draws per row: everything seeded, r and delta_A the row's."""
    rng = random.Random(f"wrap-rows:{seed}:{l}")
    drs = [o.draw(rng, l, sk, dgk, rbits, shuffle) for _ in rows]
    for d, row in zip(drs, rows):
        d.r, d.delta_a = row.r, row.delta_a
    return drs


def _traced(x, y, l, sk, dgk, dr, randomize):
    trace = {}
    o.compare(sk.enc_raw(x), sk.enc_raw(y), l, sk, dgk, dr, randomize, trace)
    return {k: trace[k] for k in KEEP}


def traces(rows, l, sk, dgk, drs, randomize, workers=0):
    """[trace of oracle.compare(Enc(x), Enc(y), ...)] for the rows; the inputs are the unrandomized encryptions."""
    args = ([r.x for r in rows], [r.y for r in rows], [l] * len(rows), [sk] * len(rows), [dgk] * len(rows), drs, [randomize] * len(rows))
    workers = min(workers, os.cpu_count() or 1, len(rows))
    if workers <= 1:
        return list(map(_traced, *args))
    with ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn")) as pool:
        return list(pool.map(_traced, *args))


class PlantedStream:
    """A session's seeded stream with the row's draws planted: the first draw below N is r (step 1), the first coin is delta_A (step
    4g, before the shuffle's own draw below 2); every other value, and the stream's position, are the seeded stream's."""

    def __init__(self, rng, n, row):
        self.rng, self.n, self.r, self.delta_a = rng, n, row.r, row.delta_a

    def randrange(self, m):
        v = self.rng.randrange(m)
        if m == self.n and self.r is not None:
            v, self.r = self.r, None
        elif m == 2 and self.delta_a is not None:
            v, self.delta_a = self.delta_a, None
        return v

    def getrandbits(self, k):
        return self.rng.getrandbits(k)


def session_rows(n, l, count=16):
    """Rows for concurrent single comparisons: every one in the wrap cell, in turn from the rows the protocol gets wrong (by the
    value they give) and the rows it gets right."""
    import _wrap_rows as W

    groups = {}
    for row in W.rows(n, l):
        if W.conditions(n, l, row).wrap:
            groups.setdefault((W.protocol_is_right(n, l, row), W.protocol_value(n, l, row)), []).append(row)
    order = sorted(groups)                               # wrong before right; each group's rows in table order, spread out
    rows = [groups[k][(i * len(groups[k])) // count] for i in range(count) for k in order][:count * len(order)]
    rows = list(dict.fromkeys(rows[i] for i in range(len(rows))))[:count]
    assert len(rows) == count and {W.protocol_value(n, l, r) for r in rows} == {0, 1, 2, n - 1}
    return rows


def check_sessions(rows, l, sk, dgk, bob_p, bob_d):
    """`rows` as concurrent perform_secure_comparison sessions whose streams are planted: through the coalescer and one by one
    (the fused single comparison), every message equal; step 1 carries the row's z, [d] the row's d, the result the predicted value."""
    import _wrap_rows as W
    from _coalesce_harness import run_sessions

    n = sk.n
    pairs = [(row.x, row.y) for row in rows]
    plant = lambda tag, i, rng: PlantedStream(rng, n, rows[i]) if tag == "a" else rng  # noqa: E731
    co_res, co_sent, stats = run_sessions(pairs, l, bob_p, bob_d, coalesce=True, streams=plant)
    un_res, un_sent, _ = run_sessions(pairs, l, bob_p, bob_d, coalesce=False, streams=plant)
    assert co_sent.keys() == un_sent.keys() and len(co_sent) == 4 * len(rows)
    for k in co_sent:
        assert co_sent[k] == un_sent[k], k
    assert co_res == un_res
    for i, row in enumerate(rows):
        z = ((1 << l) + row.r + row.y - row.x) % n
        assert [sk.dec_raw(c) for c in co_sent[f"step_1_session_{i + 1}"]] == [z], row
        d_sent, betas = co_sent[f"step_4b_session_{i + 1}"][0], co_sent[f"step_4b_session_{i + 1}"][1:]
        assert int(not dgk.is_zero(d_sent)) == W.conditions(n, l, row).d == 1 and len(betas) == l
        assert [int(not dgk.is_zero(b)) for b in betas] == o.to_bits(z % (1 << l), l)
        z1, z2, _ = co_sent[f"step_5_session_{i + 1}"]
        assert sk.dec_raw(z1) == z >> l and sk.dec_raw(z2) == (z + n) >> l
        assert sk.dec_raw(co_res[i]) == W.protocol_value(n, l, row), row
    return stats

"""GPU tests added in round 2: the per-GPU shares of BASELINE configs[3] / configs[4] at full size, the exact
non-invertible index, shared fixed-base tables, one context alternating between streams, and bench.py's rank handling."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, oracle_dgk, oracle_paillier
from oracle import sc_oracle as o
from test_gpu_parity import _draw_tensors, _schemes

pytestmark = pytest.mark.gpu


def _oracle_rows(engine, idx, l, sk, dgk, x_enc, y_enc, draws):
    """oracle.compare on rows `idx` of a device-resident batch (inputs and every random draw downloaded)."""
    it = torch.tensor(idx, device=engine.device)
    ints = lambda t: engine.download(t[it])                                  # noqa: E731
    perb = lambda t: [engine.download(t[:, i]) for i in idx]                 # noqa: E731
    M = (1 << 64) - 1
    perms = [None] * len(idx) if draws.permutation is None else draws.permutation[it].tolist()
    rows = zip(ints(x_enc), ints(y_enc), ints(draws.r), [int(v) & M for v in draws.delta_a[it].tolist()], perb(draws.rhos),
               ints(draws.rho_z), perb(draws.r_bob_dgk), perb(draws.r_alice_dgk), ints(draws.rho_zeta_1), ints(draws.rho_zeta_2),
               ints(draws.rho_delta_b), perms)
    expect = []
    for xe, ye, r, da, rhos, rho_z, rb, rc, z1, z2, zb, pm in rows:
        if pm is not None:       # the library randomizes c_j with r_alice[j] before the shuffle, the oracle output k after it
            rc = [rc[src] for src in pm]
        dr = o.Draws(r=r, delta_a=da, rhos=rhos, perm=pm, rho_z=rho_z, r_d=rb[0], r_beta=rb[1:], r_c=rc, rho_zeta1=z1,
                     rho_zeta2=z2, rho_delta_b=zb)
        expect.append(o.compare(xe, ye, l, sk, dgk, dr, True))
    return expect


@pytest.mark.parametrize("pbits, dname, B, l", [
    # (configs[3]'s share of 131072 and configs[4]'s with the 2048-bit DGK key run with two concurrent shards, as bench.py runs
    #  them, in test_gpu_round3.py::test_the_configuration_bench_times -- under the oracle as well)
    (3072, "dgk_3072_l64", 32768, 64),       # configs[4]: 262144 over 8 GPUs -> 32768 per GPU, DGK size unspecified there: the 3072-bit variant, one stream
])
def test_per_gpu_shares_of_the_eight_gpu_configs_full_size(engine, keys, pbits, dname, B, l):
    """Full-size per-GPU shares (scratch arena, parking buffer, inversion-tree depth, 67-bit rho at l = 64): Dec(result) ==
    [x <= y] for every comparison, and a sampled subset -- first, last, one in the last partially filled wave of every kernel
    configuration -- bit-exact against the oracle, shuffle included."""
    import bench
    from protocols.secure_comparison_amd.batch import secure_comparison_batch

    sk, dgk = oracle_paillier(keys, pbits), oracle_dgk(keys, dname)
    engine.set_latency_mode(1)
    try:
        alice_p, alice_d, bob_p, bob_d = _schemes(engine, sk, dgk, 400)
        x, y, x_enc, y_enc, draws = bench.synth_inputs(engine, l, alice_p, bob_p, bob_d, B, 400, seed=l + pbits, shuffle=True)
        res = secure_comparison_batch(x_enc, y_enc, l, alice_p, alice_d, bob_p, bob_d, draws)
        dec = bob_p.decrypt_raw_batch(res)
        assert bool(((dec[:, 0] == (x <= y).to(torch.int32)) & (dec[:, 1:] == 0).all(dim=1)).all().item())
        idx = [0, 1, 8, 9, B // 2 + 3, B - 67, B - 2, B - 1]
        assert engine.download(res[torch.tensor(idx, device=engine.device)]) == _oracle_rows(engine, idx, l, sk, dgk, x_enc, y_enc, draws)
    finally:
        engine.set_latency_mode(0)


def test_not_invertible_index_is_exact(engine):
    """sc_modinv names a non-invertible element itself (not the chunk it sits in), at every depth of the inversion tree.  The planted
    elements are canonical residues like every operand (an unreduced one is an argument error: tests/test_gpu_kernel_edges.py)."""
    from protocols.secure_comparison_amd.engine import NotInvertibleError

    rng = random.Random(5)
    n = 3 * 5 * 7 * (rng.getrandbits(1000) | 1)
    mod = engine.modulus(n)
    import math

    def units(k):
        out = []
        while len(out) < k:
            v = rng.randrange(2, n)
            if math.gcd(v, n) == 1:
                out.append(v)
        return out

    for count, bad_at in ((3, 1), (48, 47), (49, 0), (500, 333), (5000, 4999), (70000, 12345)):
        xs = units(min(count, 600))
        xs = (xs * (count // len(xs) + 1))[:count]
        xs[bad_at] = 35 * xs[bad_at] % n
        with pytest.raises(NotInvertibleError) as ei:
            engine.modinv(mod, engine.upload(xs, mod.nwords))
        assert ei.value.index == bad_at and str(bad_at) in str(ei.value)
    # two bad elements: one of them is named
    xs = units(300)
    xs[17], xs[250] = xs[17] * 3 % n, xs[250] * 7 % n
    with pytest.raises(NotInvertibleError) as ei:
        engine.modinv(mod, engine.upload(xs, mod.nwords))
    assert ei.value.index in (17, 250)
    # and a clean batch still inverts
    xs = units(300)
    assert engine.download(engine.modinv(mod, engine.upload(xs, mod.nwords))) == [pow(v, -1, n) for v in xs]


def test_shared_fixed_base_tables(engine, keys):
    """A second library context imports the first one's tables (sc_fbt_import): same residues, no second copy, and the rows
    outlive the context that built them."""
    from protocols.secure_comparison_amd import DGK
    from protocols.secure_comparison_amd.engine import Engine

    dgk = oracle_dgk(keys, "dgk_1024_l16")
    rng = random.Random(8)
    e1, e2 = Engine(), Engine()
    mk = lambda e: DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=e, randomizer_bits=400, fixed_base_window=8)  # noqa: E731
    bob1, bob2 = mk(e1), mk(e2)
    alice1, alice2 = bob1.public_copy(), bob2.public_copy()
    bob2.share_tables_from(bob1)
    alice2.share_tables_from(alice1)
    rs = [rng.getrandbits(400) for _ in range(50)]
    cs = [dgk.enc_raw(rng.randrange(dgk.u)) for _ in rs]
    expect = [dgk.randomize(c, r) for c, r in zip(cs, rs)]
    for sch in (alice1, alice2, bob1, bob2):
        e = sch.engine
        assert e.download(sch.randomize_batch(e.upload(cs, sch.mod_n.nwords), e.upload(rs, 13))) == expect
    assert alice2.table_build_s == 0.0 and bob2.table_build_s == 0.0 and alice1.table_build_s > 0.0
    assert alice2.table_bytes() == alice1.table_bytes() > 0 and bob2.table_bytes() == bob1.table_bytes() > 0
    assert bob1.table_bytes() < alice1.table_bytes()     # the key holder's CRT path builds half-size tables only: none for h mod n
    e1.close()                                     # the builder goes away; the importer keeps the rows alive
    assert e2.download(alice2.randomize_batch(e2.upload(cs, alice2.mod_n.nwords), e2.upload(rs, 13))) == expect
    other = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, engine=e2, randomizer_bits=300, fixed_base_window=8)
    with pytest.raises(ValueError):
        other.share_tables_from(alice2)
    e2.close()


def test_one_context_alternating_between_streams(keys):
    """Engine follows torch's current stream; the context's scratch arena / temporaries / parked tables are reused from call
    to call, so sc_ctx_set_stream must order the previous stream's work before the next stream's (regression for silently
    wrong residues when a scheme object is used under `with torch.cuda.stream(s)` for some calls only)."""
    from protocols.secure_comparison_amd import DGK, Paillier
    from protocols.secure_comparison_amd.engine import Engine

    sk, dgk = oracle_paillier(keys, 2048), oracle_dgk(keys, "dgk_2048_l32")
    eng = Engine()
    eng.set_latency_mode(0)
    pai = Paillier(sk.n, sk.p, sk.q, engine=eng)
    alice = pai.public_copy()
    rng = random.Random(12)
    B = 3000                                           # long enough launches that an unordered successor would overlap
    rho = eng.upload([1 + rng.randrange(sk.n - 1) for _ in range(B)], alice.mod_n.nwords)
    ms = [rng.randrange(sk.n) for _ in range(B)]
    c = alice.encrypt_raw_batch(eng.upload(ms, alice.mod_n.nwords))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for k in range(6):                                 # randomize on one stream, decrypt right away on another: both use the
        with torch.cuda.stream(s1 if k % 2 == 0 else s2):   # same scratch arena and temporaries
            r = alice.randomize_batch(c, rho)
        with torch.cuda.stream(s2 if k % 2 == 0 else s1):
            s = torch.cuda.current_stream()
            s.wait_stream(s1 if k % 2 == 0 else s2)    # the caller's own buffers follow the usual stream rules
            outs.append(pai.decrypt_raw_batch(r))
    torch.cuda.synchronize()
    for d in outs:
        assert eng.download(d) == ms
    eng.close()


def test_bench_rank_handling_on_one_gpu():
    """`bench.py --gpus 1 --force-dist` goes through RCCL with one rank and says so; `--gpus 2` on a one-GPU box fails."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    bench = os.path.join(ROOT, "bench.py")
    cp = subprocess.run([sys.executable, bench, "--gpus", "1", "--force-dist", "--c-abi-gather", "--batch", "512", "--l", "16", "--dgk", "dgk_2048_l16", "--fb-window", "8",
                         "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"], env=env, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-2000:]
    line = json.loads(cp.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["rccl_ranks"] == 1 and line["rank_devices"] == [0] and line["value"] > 0
    assert line["c_abi_gather"] == {"equal_to_torch_gather": True, "ranks": 1}
    assert 0 < line["roofline"]["frac"] < 1 and line["config"]["fixed_base_table_bytes"] > 0
    if torch.cuda.device_count() < 2:
        cp = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=300)
        assert cp.returncode != 0 and "n_gpus" not in cp.stdout


def _prime_and_non_residue(bits, _cache={}):
    """A seeded prime of `bits` bits and a quadratic non-residue modulo it."""
    if bits not in _cache:
        from protocols.secure_comparison_amd.keygen import next_prime

        p = next_prime(random.Random(f"prime:{bits}").getrandbits(bits - 2) | (1 << (bits - 1)))
        assert p.bit_length() == bits
        z = next(z for z in range(2, 200) if pow(z, (p - 1) // 2, p) == p - 1)
        _cache[bits] = (p, z)
    return _cache[bits]


@pytest.mark.parametrize("bits", [523, 600, 1000, 1024, 1028])
def test_onelane_configuration_primitives(onelane_engine, bits):
    """The one-lane (1, 37, 28-bit) kernels forced on: shared-exponent powers (short / long exponents, wide operands reduced
    first, fused multiply, is-one flags) and pair arithmetic modulo m^2, against Python integers, incl. operands 0, 1, m - 1
    and ragged batch sizes around a wave of 64 numbers."""
    eng = onelane_engine
    rng = random.Random(bits)
    m = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    mod = eng.modulus(m)
    mod2 = eng.modulus(m * m, 2 * mod.nwords)
    for count in (1, 63, 64, 65, 200):
        xs = [0, 1, m - 1][: min(3, count)] + [rng.randrange(m) for _ in range(max(0, count - 3))]
        t = eng.upload(xs, mod.nwords)
        for e in (rng.getrandbits(65) | (1 << 64), rng.getrandbits(bits) | 1, (1 << 200) - 1):
            assert eng.download(eng.modexp_shared(mod, t, e)) == [pow(x, e, m) for x in xs]
        e = rng.getrandbits(160) | (1 << 159)
        ys = [rng.randrange(m) for _ in xs]
        assert eng.download(eng.modexp_shared(mod, t, e, mul_into=eng.upload(ys, mod.nwords))) == [pow(x, e, m) * y % m for x, y in zip(xs, ys)]
        wide = [rng.getrandbits(2 * bits + 40) for _ in xs]                       # wider than the modulus: reduced first
        tw = eng.upload(wide, 2 * mod.nwords + 2)
        assert eng.download(eng.modexp_shared(mod, tw, e)) == [pow(x % m, e, m) for x in wide]
        flags = eng.modexp_shared_isone(mod, t, e).tolist()
        assert flags == [int(pow(x, e, m) == 1) for x in xs]
        if bits == 1024:
            # operands whose power IS 1: modulo a prime p, x^((p-1)/2) = 1 exactly for the quadratic residues -- squares at the even
            # rows, a non-residue times a square at the odd ones
            p, z = _prime_and_non_residue(bits)
            half = (p - 1) // 2
            sq = [pow(rng.randrange(1, p), 2, p) for _ in range(count)]
            planted = [s if i % 2 == 0 else s * z % p for i, s in enumerate(sq)]
            planted[0] = 1
            want = [int(i % 2 == 0) for i in range(count)]
            assert want == [int(pow(x, half, p) == 1) for x in planted]
            mod_p = eng.modulus(p)
            assert eng.modexp_shared_isone(mod_p, eng.upload(planted, mod_p.nwords), half).tolist() == want
        # pair arithmetic: x^e mod m^2 from operands of 1, 2 and (wide) 3+ chunks, with and without the fused product
        for width, src in ((mod.nwords, xs), (2 * mod.nwords, [rng.randrange(m * m) for _ in xs])):
            tx = eng.upload(src, width)
            ee = rng.getrandbits(bits) | (1 << (bits - 1))
            assert eng.download(eng.modexp_shared_sq(mod, mod2, tx, ee)) == [pow(x, ee, m * m) for x in src]
            into = [rng.randrange(m * m) for _ in src]
            assert eng.download(eng.modexp_shared_sq(mod, mod2, tx, ee, mul_into=eng.upload(into, 2 * mod.nwords))) == \
                [pow(x, ee, m * m) * v % (m * m) for x, v in zip(src, into)]


def test_onelane_whole_comparisons(onelane_engine, keys):
    """Whole comparisons with the one-lane kernels forced on for every 1024-bit modulus of the key holder's CRT paths and
    the DGK zero test (2048-bit keys, l = 32), bit-exact against the oracle; and the three kernel policies agree."""
    from protocols.secure_comparison_amd.batch import secure_comparison_batch

    eng = onelane_engine
    sk, dgk = oracle_paillier(keys, 2048), oracle_dgk(keys, "dgk_2048_l32")
    l, B, rbits = 32, 70, 400
    alice_p, alice_d, bob_p, bob_d = _schemes(eng, sk, dgk, rbits)
    rng = random.Random(2048)
    xs = [rng.randrange(1 << l) for _ in range(B)]
    ys = [xs[i] if i % 4 == 0 else rng.randrange(1 << l) for i in range(B)]
    drs = [o.draw(rng, l, sk, dgk, rbits) for _ in range(B)]
    x_enc = [sk.randomize(sk.enc_raw(x), 1 + rng.randrange(sk.n - 1)) for x in xs]
    y_enc = [sk.randomize(sk.enc_raw(y), 1 + rng.randrange(sk.n - 1)) for y in ys]
    expect = [o.compare(a, b, l, sk, dgk, d, True) for a, b, d in zip(x_enc, y_enc, drs)]
    nw = bob_p.mod_n.nwords
    draws = _draw_tensors(eng, drs, l, nw, (dgk.u.bit_length() + 31) // 32, (rbits + 31) // 32, eng.device)
    tx, ty = eng.upload(x_enc, 2 * nw), eng.upload(y_enc, 2 * nw)
    assert eng.download(secure_comparison_batch(tx, ty, l, alice_p, alice_d, bob_p, bob_d, draws)) == expect
    eng.set_onelane_mode(0)
    assert eng.download(secure_comparison_batch(tx, ty, l, alice_p, alice_d, bob_p, bob_d, draws)) == expect
    assert [sk.dec_raw(c) for c in expect] == [int(x <= y) for x, y in zip(xs, ys)]


def test_scattered_store_is_the_shuffle(engine, keys):
    """sc_modexp_var_scatter: the result of item i lands in row dest[i] -- equal to computing in place and gathering; rows named
    out of range are dropped (nothing is written outside the output array), and Initiator.step_4i_batch refuses permutations
    that are not int64 [B][l+1] (entries out of range are clamped: no host round trip in the middle of a step)."""
    from protocols.secure_comparison_amd import DGK, Initiator

    dgk = oracle_dgk(keys, "dgk_1024_l16")
    rng = random.Random(3)
    sch = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, engine=engine, randomizer_bits=400)
    mod = sch.mod_n
    count = 333
    xs = [rng.randrange(1, dgk.n) for _ in range(count)]
    es = [rng.randrange(1, dgk.u) for _ in range(count)]
    perm = list(range(count))
    rng.shuffle(perm)
    tx, te = engine.upload(xs, mod.nwords), engine.upload(es, 1)
    dest = torch.tensor(perm, dtype=torch.int64, device=engine.device)
    got = engine.download(engine.modexp_var(mod, tx, te, 18, dest=dest))
    expect = [None] * count
    for i, d in enumerate(perm):
        expect[d] = pow(xs[i], es[i], dgk.n)
    assert got == expect
    # out-of-range destinations: guard words around the output stay untouched
    buf = torch.full((count + 2, mod.nwords), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    bad = dest.clone()
    bad[7], bad[100] = count + 5, 1 << 40
    engine.modexp_var(mod, tx, te, 18, out=buf[1:count + 1], dest=bad)
    torch.cuda.synchronize()
    assert bool((buf[0] == 0x5A5A5A5A).all()) and bool((buf[count + 1] == 0x5A5A5A5A).all())
    # the protocol-level entry
    l, B = 16, 9
    c = engine.upload([rng.randrange(1, dgk.n) for _ in range((l + 1) * B)], mod.nwords).reshape(l + 1, B, mod.nwords)
    rhos = engine.upload([rng.randrange(1, dgk.u) for _ in range((l + 1) * B)], 1).reshape(l + 1, B, 1)
    pm = torch.stack([torch.randperm(l + 1) for _ in range(B)]).to(engine.device)
    plain = Initiator.step_4i_batch(c, sch, rhos, None)
    shuffled = Initiator.step_4i_batch(c, sch, rhos, pm)
    idx = pm.t().reshape(l + 1, B, 1).expand(l + 1, B, mod.nwords)
    assert torch.equal(shuffled, torch.gather(plain, 0, idx))
    for wrong in (pm[:, :-1], pm.to(torch.int32), pm[:-1]):
        with pytest.raises(ValueError):
            Initiator.step_4i_batch(c, sch, rhos, wrong)


@pytest.mark.parametrize("mode", [0, 2])
def test_fused_any_zero_equals_or_of_zero_tests(engine, keys, mode):
    """sc_modexp_shared_isone_any (delta_B in the zero-test launch) against the per-item flags OR-ed on the host side, with
    zero plaintexts planted in known planes, ragged batch, both kernel policies for the 1024-bit prime."""
    from protocols.secure_comparison_amd import DGK

    dgk = oracle_dgk(keys, "dgk_2048_l32")
    sch = DGK(dgk.n, dgk.g, dgk.h, dgk.u, dgk.t, dgk.p, dgk.q, dgk.v_p, dgk.v_q, engine=engine, randomizer_bits=400)
    rng = random.Random(44)
    planes, B = 33, 77
    ms = [[rng.randrange(1, dgk.u) for _ in range(B)] for _ in range(planes)]
    for b in (0, 5, 76):
        ms[rng.randrange(planes)][b] = 0
    ms[3][40] = ms[20][40] = 0                                   # two zero planes in one comparison
    c = torch.stack([engine.upload([dgk.randomize(dgk.enc_raw(m), rng.getrandbits(400)) for m in row], sch.mod_n.nwords) for row in ms])
    engine.set_onelane_mode(mode)
    try:
        got = sch.any_zero_batch(c).tolist()
        flags = sch.is_zero_batch(c.reshape(planes * B, -1)).reshape(planes, B)
    finally:
        engine.set_onelane_mode(1)
    expect = [int(any(ms[i][b] == 0 for i in range(planes))) for b in range(B)]
    assert got == expect == (flags != 0).any(dim=0).to(torch.int64).tolist() and sum(expect) == 4


def test_selected_constant_product(engine, keys):
    """sc_modmul_const_sel: a[i] * (flag ? c1 : c0), the residue 1 as default constant, in place, ragged count."""
    dgk = oracle_dgk(keys, "dgk_2048_l32")
    rng = random.Random(9)
    mod = engine.modulus(dgk.n)
    count = 201
    xs = [0, 1, dgk.n - 1] + [rng.randrange(dgk.n) for _ in range(count - 3)]
    fl = [rng.randrange(2) * rng.choice([1, 1, 255]) for _ in range(count)]
    t = engine.upload(xs, mod.nwords)
    flags = torch.tensor(fl, dtype=torch.uint8, device=engine.device)
    assert engine.download(engine.modmul_const_sel(mod, t, None, dgk.g, flags)) == [x * (dgk.g if f else 1) % dgk.n for x, f in zip(xs, fl)]
    assert engine.download(engine.modmul_const_sel(mod, t, dgk.h, dgk.g, flags, out=t)) == [x * (dgk.g if f else dgk.h) % dgk.n for x, f in zip(xs, fl)]
    with pytest.raises(ValueError):
        engine.modmul_const_sel(mod, t, None, dgk.g, flags[:-1])
    with pytest.raises(ValueError):
        engine.modmul_const_sel(mod, t, None, dgk.g, flags.to(torch.int32))


def test_c_abi_allgather_single_rank(engine):
    """sc_comm_unique_id / sc_comm_init / sc_allgather / sc_comm_destroy through RCCL with one rank (the boxes of this build have
    one GPU): the gather is the identity, asynchronous on the engine's stream, and a second init is refused."""
    from protocols.secure_comparison_amd.engine import Engine

    eng = Engine()
    cid = eng.comm_unique_id()
    assert len(cid) == 128 and any(cid)
    with pytest.raises(Exception):
        eng.allgather(torch.zeros((2, 4), dtype=torch.int32, device=eng.device))      # no communicator yet
    eng.comm_init(cid, 0, 1)
    with pytest.raises(ValueError):
        eng.comm_init(cid, 0, 1)
    x = torch.arange(3 * 5 * 128, dtype=torch.int32, device=eng.device).reshape(3, 5, 128)
    got = eng.allgather(x)
    torch.cuda.synchronize()
    assert got.shape == (3, 5, 128) and torch.equal(got, x)
    eng.comm_destroy()
    eng.close()

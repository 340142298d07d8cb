"""CPU tier of the linear maps with public weights: the signed split against the plain model, the fit rule one bit
either side of its boundary for 512- to 3072-bit N, the refusals of the Python layer, linear_planes_batch / linear_rows_batch on the
stand-in engine against plain Python (decrypted, signed, with bias and re-randomization), and the two new symbols."""
import ctypes
import os
import random
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _linear_model as LM  # noqa: E402
from test_aggregate_cpu import StandIn, _decrypt, _encrypt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sk():
    from oracle import sc_oracle as o

    return o.PaillierKey.generate(512, random.Random(20263))


class LinStandIn(StandIn):
    """The stand-in engine with the linear map as the plain model; geometry and weights of every call are recorded."""

    def __init__(self):
        super().__init__()
        self.maps = []

    def paillier_linear_axis(self, key, c, outer, K, inner, weights, out=None):
        self.maps.append((outer, K, inner, [list(r) for r in weights]))
        flat = self._ints(c.reshape(-1, c.shape[-1]))
        return self.upload(LM.lin_axis(key.mod_n2.n, flat, outer, K, inner, weights), key.mod_n2.nwords)


def _lin_players(sk):
    from protocols.secure_comparison_amd import Paillier

    eng = LinStandIn()
    return eng, Paillier(sk.n, engine=eng), Paillier(sk.n, sk.p, sk.q, engine=eng)


# ---- the model and the split -------------------------------------------------------------------------------------------------------
def test_model_lin_axis():
    rng = random.Random(3)
    n = rng.getrandbits(200) | 1 | 1 << 199
    outer, K, inner = 2, 3, 5
    x = [rng.randrange(1, n) for _ in range(outer * K * inner)]
    at = lambda o, k, i: (o * K + k) * inner + i  # noqa: E731
    W = [[0, 0, 0], [0, 1, 0], [2, 0, 3], [1, 1, 1]]
    got = LM.lin_axis(n, x, outer, K, inner, W)
    out = lambda o, j, i: got[(o * len(W) + j) * inner + i]  # noqa: E731
    assert all(out(o, 0, i) == 1 and out(o, 1, i) == x[at(o, 1, i)] for o in range(outer) for i in range(inner))
    assert out(1, 2, 4) == x[at(1, 0, 4)] ** 2 * x[at(1, 2, 4)] ** 3 % n
    assert out(0, 3, 2) == x[at(0, 0, 2)] * x[at(0, 1, 2)] * x[at(0, 2, 2)] % n
    assert LM.lin_axis(n, x, 1, outer * K, inner, [[1] * (outer * K)]) != LM.lin_axis(n, x, 1, inner, outer * K, [[1] * inner])
    rows = LM.edge_rows(7)
    assert rows[0] == [0] * 7 and sorted(rows[1]) == [0] * 6 + [1] and sorted(rows[2]) == [0] * 6 + [1 << 63] and rows[3] == [LM.U64] * 7
    assert len({max(r).bit_length() for r in rows}) >= 3 and {v.bit_length() for v in rows[4]} >= {1, 8, 16, 33, 64}
    assert all(sorted(map(tuple, LM.matrix(K, 5, s))) == sorted(map(tuple, LM.edge_rows(K, s))) for K in (1, 2, 3, 7, 33) for s in range(6))


def test_signed_split_matches_the_model():
    from protocols.secure_comparison_amd.linear import split_signed

    rng = random.Random("split")
    for trial in range(200):
        J, K = rng.randrange(1, 6), rng.randrange(1, 9)
        W = [[rng.choice((0, 0, 1, -1, rng.randrange(-(1 << 64) + 1, 1 << 64))) for _ in range(K)] for _ in range(J)]
        negated, nonneg = split_signed(W)
        members, want = LM.split_signed(W)
        assert negated == [k for k in range(K) if any(row[k] < 0 for row in W)]           # negated only if it carries a negative weight
        assert [(k, False) for k in range(K)] + [(k, True) for k in negated] == members and nonneg == want
        assert all(0 <= v < 1 << 64 for row in nonneg for v in row)
        x = [rng.randrange(-50, 50) for _ in range(K)]
        xs = x + [-x[k] for k in negated]
        assert [sum(w * v for w, v in zip(row, xs)) for row in nonneg] == [sum(w * v for w, v in zip(row, x)) for row in W]
    assert split_signed([[1, 2], [3, 0]]) == ([], [[1, 2], [3, 0]])
    assert split_signed([[1, -2, 0], [0, 5, -(1 << 64) + 1]]) == ([1, 2], [[1, 0, 0, 2, 0], [0, 5, 0, 0, (1 << 64) - 1]])


# ---- the fit rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", (512, 1024, 1536, 2048, 3072))
def test_fit_rule_at_its_boundary(nbits):
    """bits(sum |W|) + x_bits + 1 < nbits - 1: the last width that fits and the first that does not, the row named."""
    from protocols.secure_comparison_amd.linear import check_fit

    for W in ([[1]], [[3, -4]], [[(1 << 64) - 1] * 5], [[1, 1], [-(1 << 40), 1 << 40]]):
        for j in range(len(W)):
            sbits = sum(abs(v) for v in W[j]).bit_length()
            if any(sum(abs(v) for v in row).bit_length() > sbits for row in W):
                continue                                                                   # row j must be the widest: it decides
            edge = nbits - 3 - sbits                                                       # sbits + edge + 1 == nbits - 2: the last that fits
            check_fit(W, edge, nbits)
            assert all(LM.fits(W, edge, nbits)) and not LM.fits(W, edge + 1, nbits)[j]
            first = LM.fits(W, edge + 1, nbits).index(False)
            with pytest.raises(ValueError, match=rf"row {first}\b"):
                check_fit(W, edge + 1, nbits)
    with pytest.raises(ValueError):
        check_fit([[1]], 0, nbits)


# ---- refusals of the Python layer ----------------------------------------------------------------------------------------------------
def test_python_layer_refusals(sk):
    from protocols.secure_comparison_amd import linear_planes_batch, linear_rows_batch

    eng, ap, bp = _lin_players(sk)
    rng = random.Random("refuse")
    x = _encrypt(eng, sk, rng, list(range(6))).reshape(2, 3, -1)
    for bad, what in (([[1, 2], [3]], "row 1"), ([[1, 2, 3]], "row 0"), ([[1, 1 << 64]], "2\\^64"), ([[-(1 << 64), 1]], "2\\^64"),
                      ([[1.5, 2]], "integers"), ([[True, 2]], "integers"), ([], "at least one"), ([[]], "at least one"),
                      (torch.ones(2, 2, dtype=torch.int32), "int64"), (torch.ones(2, dtype=torch.int64), "int64")):
        with pytest.raises(ValueError, match=what):
            linear_planes_batch(x, bad, ap)
    for bias in ([1], [1, 2, 3], [1.0, 2], [sk.n, 0], 5):
        with pytest.raises(ValueError, match="bias"):
            linear_planes_batch(x, [[1, 2], [3, 4]], ap, bias=bias)
    for seg in (0, 2, 4, -1):
        with pytest.raises(ValueError, match="divisor"):
            linear_rows_batch(x, [[1] * max(seg, 1)], ap, segment=seg)
    with pytest.raises(ValueError, match="row 0"):
        linear_rows_batch(x, [[1, 2]], ap)                                                # B = 3 weights wanted
    with pytest.raises(ValueError, match=r"row 1\b"):
        linear_planes_batch(x, [[1, 1], [1 << 60, 1 << 60]], ap, x_bits=sk.n.bit_length() - 62)
    with pytest.raises(ValueError):
        linear_planes_batch(x[0], [[1]], ap)
    with pytest.raises(ValueError, match="at most 1024"):
        linear_planes_batch(x, [[1, 2]] * 1025, ap)
    assert eng.maps == []                                                                  # nothing reached the engine


# ---- the Python layer on the stand-in engine ------------------------------------------------------------------------------------------
def test_planes_on_the_stand_in(sk):
    from protocols.secure_comparison_amd import linear_planes_batch

    eng, ap, bp = _lin_players(sk)
    rng, K, B = random.Random("planes"), 4, 6
    plain = [[rng.randrange(-1000, 1000) for _ in range(B)] for _ in range(K)]
    x = _encrypt(eng, sk, rng, [v for row in plain for v in row]).reshape(K, B, -1)
    clone = x.clone()
    W = [[3, 0, -2, 1], [0, 0, 0, 0], [0, 1, 0, 0], [-(1 << 64) + 1, 5, -7, (1 << 64) - 1], [1, 2, 3, 4]]
    bias = [5, -9, 0, 1 << 70, -(1 << 70)]
    out = linear_planes_batch(x, W, ap, bias=bias, x_bits=11)
    assert tuple(out.shape) == (len(W), B, x.shape[-1]) and torch.equal(x, clone)
    assert _decrypt(eng, sk, out, signed=True) == [v for row in LM.signed_map(W, bias, plain) for v in row]
    outer, Kp, inner, Wp = eng.maps[-1]
    assert (outer, Kp, inner) == (1, K + 2, B) and Wp == LM.split_signed(W)[1]             # planes 0 and 2 negated, 1 and 3 not
    # the residues: the model on the members the split names, times the unrandomized [[b_j]]
    flat = eng.download(x.reshape(K * B, -1))
    members = flat + [pow(c, -1, sk.n2) for k in (0, 2) for c in flat[k * B:(k + 1) * B]]
    want = [c * (1 + (b % sk.n) * sk.n) % sk.n2 for c, b in zip(LM.lin_axis(sk.n2, members, 1, K + 2, B, Wp), [b for b in bias for _ in range(B)])]
    assert eng.download(out.reshape(len(W) * B, -1)) == want
    # without negative weights nothing is inverted; a tensor of weights is a list of weights
    t = torch.tensor([[1, 2, 3, 4], [0, 0, 9, 0]], dtype=torch.int64)
    pos = linear_planes_batch(x, t, ap)
    assert eng.maps[-1] == (1, K, B, t.tolist())
    assert _decrypt(eng, sk, pos, signed=True) == [v for row in LM.signed_map(t.tolist(), None, plain) for v in row]
    # rho changes every residue and no plaintext
    rho = eng.upload([rng.randrange(1, sk.n) for _ in range(2 * B)], ap.mod_n.nwords).reshape(2, B, -1)
    fresh = linear_planes_batch(x, t, ap, rho=rho)
    a, b = eng.download(pos.reshape(2 * B, -1)), eng.download(fresh.reshape(2 * B, -1))
    assert b == [c * pow(r, sk.n, sk.n2) % sk.n2 for c, r in zip(a, eng.download(rho.reshape(2 * B, -1)))] and all(u != v for u, v in zip(a, b))
    assert _decrypt(eng, sk, fresh, signed=True) == _decrypt(eng, sk, pos, signed=True)


def test_rows_on_the_stand_in(sk):
    from protocols.secure_comparison_amd import linear_rows_batch

    eng, ap, bp = _lin_players(sk)
    rng, P, B = random.Random("rows"), 3, 6
    plain = [[rng.randrange(-1000, 1000) for _ in range(B)] for _ in range(P)]
    x = _encrypt(eng, sk, rng, [v for row in plain for v in row]).reshape(P, B, -1)
    for seg in (None, 1, 2, 3, 6):
        s = B if seg is None else seg
        W = [[rng.randrange(-9, 10) for _ in range(s)] for _ in range(2)] + [[0] * s]
        bias = [7, -3, 0]
        out = linear_rows_batch(x, W, ap, segment=seg, bias=bias)
        assert tuple(out.shape) == (P,) + (() if seg is None else (B // s,)) + (3, x.shape[-1])
        assert eng.maps[-1][:3] == (P * (B // s), len(LM.split_signed(W)[0]), 1)
        want = [sum(w * v for w, v in zip(row, plain[p][t:t + s])) + b for p in range(P) for t in range(0, B, s) for row, b in zip(W, bias)]
        assert _decrypt(eng, sk, out, signed=True) == want
    one = linear_rows_batch(x[0], [[1] * B], ap)                                          # a single plane: [B][w] -> [1][w]
    assert tuple(one.shape) == (1, x.shape[-1]) and _decrypt(eng, sk, one, signed=True) == [sum(plain[0])]


# ---- the symbols ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.build import ALL_UNITS, HOST_UNITS, LINEAR_UNITS, UNITS, build_lib
    from protocols.secure_comparison_amd.engine import Engine

    dev = open(os.path.join(ROOT, "include", "sc_amd_dev.h")).read()
    pub = open(os.path.join(ROOT, "include", "sc_amd.h")).read()
    assert re.search(r"\bint sc_modlin_axis\(sc_ctx\* ctx, int mod,", dev) and "int sc_modlin_axis(" not in pub
    assert re.search(r"\bint sc_paillier_linear_axis\(sc_ctx\* ctx, int key,", pub)
    assert "bit 30 k_lin_axis" in dev and re.search(r"#define SC_ABI_VERSION 5\b", pub)
    lib = ctypes.CDLL(build_lib(verbose=False))
    for name in ("sc_modlin_axis", "sc_paillier_linear_axis"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert len(getattr(_lib.load(), name).argtypes) == 9
    assert callable(Engine.modlin_axis) and callable(Engine.paillier_linear_axis) and _lib.ABI_VERSION == 5
    assert LINEAR_UNITS == [("sc_launch_lin", "sc_launch_lin.hip", [])] and ALL_UNITS == UNITS + LINEAR_UNITS + HOST_UNITS and len(ALL_UNITS) == 17
    unit = open(os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc", "sc_launch_lin.hip")).read()
    assert '#include "sc_launch_axis.h"' in unit and not re.search(r"#define\s+SC_\w*INSTANCES", unit) and "asm" not in unit
    import protocols.secure_comparison_amd as pkg

    assert all(name in pkg.__all__ and callable(getattr(pkg, name)) for name in ("linear_planes_batch", "linear_rows_batch"))

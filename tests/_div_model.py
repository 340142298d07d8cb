"""The secure division's model: Python's divmod as the truth, a restatement of the digit loop of
csrc/div/sc_divmod_words.h that COUNTS per row which branches it took, the edge table both test tiers run, the ledger of the kernels under
csrc/div/, and the stand-in engine's division entries."""
import random

import torch

MASK64 = (1 << 64) - 1
SATURATED, FIRST, SECOND = 0, 1, 2            # DivBranch of sc_divmod_words.h
BRANCHES = ("saturated estimate (r1 == v1)", "first correction", "second correction")

# every __global__ under csrc/div/: file (relative to csrc/) and the test that owns it
KERNELS = {"k_divmod_words": ("div/sc_kernel_divmod.h", "tests/test_gpu_division.py::test_plain_divmod_edge_table")}
# everything else the subdirectory may hold: the digit loop the kernel file includes
DIV_HEADERS = ("sc_divmod_words.h", "sc_kernel_divmod.h")


def digit_loop(x, nw, d, w=32):
    """(x div d, x mod d, [saturated, first, second]) by the steps of divmod_row / div_digit with digits of w bits: x of nw digits, 1 <= d <
    2^(2 w).  w = 32 is the kernel; a small w lets a test walk EVERY row."""
    b, mask = 1 << w, (1 << w) - 1
    assert nw >= 1 and 0 <= x < 1 << (w * nw) and 1 <= d < 1 << (2 * w)
    s = 2 * w - d.bit_length()
    v = d << s
    v1, v0 = v >> w, v & mask
    ws, bs = s // w, s % w

    def word(i):
        return (x >> (w * i)) & mask if 0 <= i < nw else 0

    def digit(k):
        return (((word(k - ws) << bs) | (word(k - ws - 1) >> (w - bs))) & mask) if bs else word(k - ws)

    R = (digit(nw + 1) << w) | digit(nw)
    assert R < v
    tally, q = [0, 0, 0], 0
    for k in range(nw - 1, -1, -1):
        u = digit(k)
        r1, r0 = R >> w, R & mask
        if r1 == v1:
            qhat, rhat = b - 1, r0 + v1
            tally[SATURATED] += 1
        else:
            qhat, rhat = divmod(R, v1)
        if rhat < b and qhat * v0 > ((rhat << w) | u):
            qhat, rhat = qhat - 1, rhat + v1
            tally[FIRST] += 1
            if rhat < b and qhat * v0 > ((rhat << w) | u):
                qhat, rhat = qhat - 1, rhat + v1
                tally[SECOND] += 1
        R = (rhat << w) + u - qhat * v0
        assert 0 <= R < v and 0 <= qhat < b, (x, nw, d, k)
        q |= qhat << (w * k)
    return q, R >> s, tally


# ---- the edge table ----------------------------------------------------------------------------------------------------------------------
NWS = (1, 2, 3, 16, 32, 33, 64, 96)
DIVISORS = (1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1)


def dividends(nw, d):
    """0, d - 1, d, d + 1, all ones, and q d + (d - 1) with every word of q all ones (the widest such q that fits nw words)."""
    full = (1 << (32 * nw)) - 1
    out = [0, d - 1, d, d + 1, full]
    qw = (full // d).bit_length() // 32                   # whole all-ones words of q with q d + d - 1 <= full
    while qw and ((1 << (32 * qw)) - 1) * d + d - 1 > full:
        qw -= 1
    out.append(((1 << (32 * qw)) - 1) * d + d - 1)
    return sorted({x for x in out if x <= full})          # (d, d + 1 do not fit one word under a wide divisor)


# Rows built to take every branch (x, nw, d).  The saturated estimate needs a partial remainder whose high digit equals v1: the top two
# digits of x are v - 1.  The corrections need a small v1 under a large v0 (Hacker's Delight's divmnu add-back vectors are of this
# kind; with a two-digit divisor the exact test makes add-back itself impossible, so they end in the second correction instead).
BRANCH_ROWS = (                                                                                # branches taken (model):
    ((((1 << 63) + 5 - 1) << 32) | 0x12345678, 3, (1 << 63) + 5),                              # saturated, first
    (0x80000000fffffffe << 32, 3, 0x80000000ffffffff),                                         # saturated, first
    ((0x7fffffff << 64) | (0x80000000 << 32), 3, 0x80000000ffffffff),                          # first, second
    (0x7fffffff << 64, 3, 0x80000001ffffffff),                                                 # first, second
    ((0x3fffffff << 66) | 1, 4, 0x20000000ffffffff),                                           # first, second under a shifted divisor (s = 2)
    (0xfe175330a11d459a2f978d87, 3, 0x80000000ffffffff),                                       # first, second (found by search)
    (0x800000012265b14e612e7696, 3, 0x800000012265b1f5),                                       # saturated, first (found by search)
    (0xfffffffe00000000, 2, 0xffffffff),                                                       # none: a divisor below 2^32 (s = 32, v0 = 0)
)


def edge_rows(nws=NWS):
    """[(x, nw, d)]: the table of the issue crossed over nws, then the branch rows."""
    rows = [(x, nw, d) for nw in nws for d in DIVISORS for x in dividends(nw, d)]
    return rows + list(BRANCH_ROWS)


def random_rows(count, seed, nws=(1, 2, 3, 5, 8, 33)):
    rng = random.Random(seed)
    rows = []
    for _ in range(count):
        nw = rng.choice(nws)
        d = rng.getrandbits(rng.choice((1, 8, 31, 32, 33, 48, 63, 64))) or 1
        x = rng.getrandbits(32 * nw) if rng.random() < 0.7 else ((rng.getrandbits(32 * nw) // d) * d + rng.choice((0, d - 1))) & ((1 << (32 * nw)) - 1)
        rows.append((x, nw, d))
    return rows


# ---- the stand-in engine's division entries (tests/_oracle_engine.py has none): mix into an OracleEngine subclass -----------------------------
class DivisionEntries:
    """plain_divmod by the restated digit loop (checked against divmod on the way), and the two scheme-level entries composed from it the way
    csrc/sc_schemes.hip composes them."""

    def plain_divmod(self, x, d, in_place=False):
        nw = x.shape[-1]
        out = []
        for xv, dv in zip(self._ints(x), [int(v) & MASK64 for v in d.tolist()]):
            q, r, _ = digit_loop(xv, nw, dv)
            assert (q, r) == divmod(xv, dv)
            out.append((q, r))
        q = self.upload([a for a, _ in out], nw)
        if in_place:
            x.copy_(q)
            q = x
        return q, self.upload_u64([b for _, b in out])

    def ctx_synchronize(self):
        pass

    def initiator_div_blind(self, key, kappa, x_bits, signed, x_enc, r, rho, d, ready=False, out=None):
        from protocols.secure_comparison_amd.division import div_fits

        if not div_fits(key.mod_n.n.bit_length(), kappa, x_bits, signed):
            raise ValueError("sc_initiator_div_blind: the blinded dividend does not fit")
        z = self.modmul(key.mod_n2, x_enc, self.paillier_encrypt(key, r))
        z = self.modmul(key.mod_n2, z, rho) if ready else self.paillier_randomize(key, z, rho)
        rq, rm = self.plain_divmod(r, d)
        return z, rq, rm

    def keyholder_div_open(self, key, z_enc, d):
        return self.plain_divmod(self.paillier_decrypt(key, z_enc), d, in_place=True)

    def modexp_var_sq(self, mod_m, mod_m2, x, e, ebits, mul_into=None, out=None):
        acc = [1] * x.shape[1]
        for j in range(x.shape[0]):
            acc = [a * pow(b, c & ((1 << ebits) - 1), mod_m2.n) % mod_m2.n for a, b, c in zip(acc, self._ints(x[j]), self._ints(e[j]))]
        if mul_into is not None:
            acc = [a * b % mod_m2.n for a, b in zip(acc, self._ints(mul_into))]
        return self.upload(acc, mod_m2.nwords)


def words_tensor(values, nwords):
    from protocols.secure_comparison_amd.limbs import ints_to_words
    import numpy as np

    return torch.from_numpy(ints_to_words(values, nwords).view(np.int32))

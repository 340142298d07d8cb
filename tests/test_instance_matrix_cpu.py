"""The instance matrix (tests/_instance_matrix.py) against the sources it describes, without a GPU: csrc/sc_route.h lists exactly the
instances the matrix lists, every matrix modulus gets the configuration the matrix claims under the first-fit rule restated from
kConfigs, the inversion operands satisfy their conditions, and the plain-integer references agree with themselves."""
import math
import os
import re
import subprocess

import _instance_matrix as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc")

# prints the list of sc_route.h, the header the launchers expand: one line per instance, in the fields of M.INSTANCES
PROGRAM = r"""
#include "sc_route.h"

#include <cstdio>

#define PUT_VM(G, L, W, NEG1) printf("vm %d %d %d %d 0 0\n", G, L, W, (int)NEG1);
#define PUT_PVM(G, L, NEG1, STAMP, DIG) printf("pvm %d %d %d %d %d %d\n", G, L, sc_host::kPairW, (int)NEG1, (int)STAMP, (int)DIG);

int main() {
  SC_VM_INSTANCES(PUT_VM)
  SC_PVM_INSTANCES(PUT_PVM)
  return 0;
}
"""


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def compiled_instances(workdir, header=None):
    """Every k_vm / k_pvm instance of the list in sc_route.h (or in the text `header`, a changed copy of it), printed by a stand-alone
    program that includes that header alone.  A header that does not compile raises CalledProcessError with the compiler's words."""
    include = CSRC
    if header is not None:
        include = str(workdir)
        (workdir / "sc_route.h").write_text(header)
    src, exe = workdir / "instances.cpp", workdir / "instances"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", include, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = []
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, g, l, w, neg1, stamp, dig = line.split()
        out.append((kind, int(g), int(l), int(w), neg1 == "1", stamp == "1", dig == "1"))
    return out


def test_matrix_lists_exactly_the_compiled_instances(tmp_path):
    got = compiled_instances(tmp_path)
    assert len(got) == len(set(got)) == 37, sorted(got)
    assert sorted(got) == sorted(M.INSTANCES)
    assert len([i for i in got if i[0] == "vm"]) == 17 and len([i for i in got if i[0] == "pvm"]) == 20
    assert len({M.instance_id(i) for i in M.INSTANCES}) == 37


def _changed(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_the_list_notices_a_new_or_a_missing_instance(tmp_path):
    text = _read("sc_route.h")
    more_vm = _changed(text, "X(16, 14, 29, false)", "X(16, 14, 29, false) X(16, 27, 29, false)")
    fewer_pvm = _changed(text, " X(8, 14, false, false, true)", "")
    more_neg1 = _changed(text, "X(8, 14, true, false, false)", "X(8, 14, true, false, false) X(8, 18, true, false, false)")
    for header in (more_vm, fewer_pvm, more_neg1):
        assert sorted(compiled_instances(tmp_path, header)) != sorted(M.INSTANCES)
    # a row that a rule can pick -- (16, 9) is the small-batch form of an (8, 18) modulus -- cannot be taken out: the header's
    # static_asserts refuse to compile
    try:
        compiled_instances(tmp_path, _changed(text, " X(16, 9, 29, false)", ""))
    except subprocess.CalledProcessError as e:
        assert "static assertion failed" in e.stderr and "has no (2G, 9) k_vm instance" in e.stderr
    else:
        raise AssertionError("sc_route.h compiled without k_vm<16, 9>")


def source_configs():
    text = _read("sc_route.h")
    body = re.search(r"constexpr Config kConfigs\[\] = \{(.*?)\};", text, re.S).group(1)
    return [(int(g), int(l), int(w)) for g, l, w in re.findall(r"\{(\d+), (\d+), (\d+), true\}", body)]


def source_first_fit(bits, nwords):
    """sc_mod_create's rule, restated from the source table: the first configuration with capacity >= bits + 8 that holds whole words,
    then (second pass) the first with capacity >= bits + 8."""
    for need_words in (True, False):
        for g, l, w in source_configs():
            if w * g * l >= bits + 8 and (not need_words or w * g * l >= 32 * nwords):
                return (g, l)
    return None


def test_every_matrix_modulus_selects_the_configuration_the_matrix_claims():
    cfgs = source_configs()
    assert [(g, l) for g, l, w in cfgs] == M.K_CONFIGS and all(w == 29 for _, _, w in cfgs)
    assert sorted(w * g * l for g, l, w in cfgs) == [w * g * l for g, l, w in cfgs]          # "ordered by capacity"
    seen = 0
    for inst in M.INSTANCES:
        kind, g, l, w, neg1, stamp, dig = inst
        cases = M.cases_for(inst)
        assert cases or stamp, M.instance_id(inst)
        for c in cases:
            seen += 1
            where = (M.instance_id(inst), c.label)
            assert c.n % 2 == 1 and c.n.bit_length() == int(c.label.split("-")[0]), where
            assert source_first_fit(c.bits, M.nwords_of(c.bits)) == c.primary == M.first_fit(c.bits), where
            if dig:                                   # sc_modexp_var_sq: the pair configuration, whatever the low limb
                assert M.pair_config(c.bits) == (g, l), where
            elif "multiple" in c.label:               # k_vm<4,18,NEG1> through M = c n: sc_modexp_var of a (4,18) modulus short enough
                assert c.primary == (4, 18) and M.has_neg1_multiple(c.n, (4, 18)), where
            else:
                assert M.expected_instance(c, kind) == inst[:5], where
            if c.pair:                                # the square must be a modulus of the library
                assert M.first_fit((c.n * c.n).bit_length()) is not None, where
            if neg1 and not c.pair and "multiple" not in c.label:
                assert M.is_neg1(c.n), where
    assert seen > 200
    # the sizes the issue names
    assert {c.bits for c in M.cases_for(("vm", 4, 18, 29, False, False, False))} >= {2052, 2080}
    for cfg in M.K_CONFIGS:
        lo, hi = M.size_range(cfg)
        assert hi <= 29 * cfg[0] * cfg[1] - 8 and source_first_fit(hi + 1, M.nwords_of(hi + 1)) != cfg
        assert lo == M.MIN_BITS or source_first_fit(lo - 1, M.nwords_of(lo - 1)) != cfg
    # the multiple M = c n of a modulus of cap - 37 bits needs a word more than the limbs hold: no twin, the plain instance
    for inst, bits in ((("pvm", 4, 14, 29, False, False, False), 1587), (("pvm", 8, 14, 29, False, False, False), 3211)):
        labels = {c.label for c in M.cases_for(inst)}
        assert {f"{bits}-one", f"{bits}-rand"} <= labels, labels
        n = M.make_modulus(bits, "one")
        assert 32 * M.nwords_of(M.neg1_multiple(n).bit_length()) > 29 * inst[1] * inst[2] and M.neg1_multiple(n) % (1 << 29) == (1 << 29) - 1
    # finding: a 1028-bit modulus fits the one-lane capacity (28 * 37 - 8) but not its whole-words condition
    assert not M.onelane_fits(M.ONE_LANE_UNREACHABLE_BITS) and M.onelane_fits(1024)


def test_inversion_operands():
    for inst in M.INSTANCES:
        for c in M.cases_for(inst):
            edge = M.edge_operands(c.n, inst)
            assert all(0 <= v < c.n for v in edge)
            assert sum(1 for v in set(edge) if v and math.gcd(v, c.n) == 1) >= 5, (M.instance_id(inst), c.label)
            inv = M.coprime_operands(c.n, inst, 11)
            assert len(inv) == 11 and all(math.gcd(v, c.n) == 1 for v in inv)
    # the not-invertible case runs on products of two matrix moduli: each factor is a residue without an inverse
    for small, large in M.NOT_INVERTIBLE:
        n = small * large
        assert math.gcd(small, n) == small > 1 and small < n and M.first_fit(n.bit_length()) is not None


def test_references_on_the_two_smallest_sizes():
    inst = ("vm", 1, 18, 29, False, False, False)
    for c in M.cases_for(inst)[:2]:
        n = c.n
        xs = M.operands(n, inst, 67)
        assert len(xs) == 67 and xs[:4] == [0, 1, 2, n - 1]
        for e in M.shared_exponents(n):
            got = M.expected_modexp_shared(n, xs, e)
            assert got[1] == 1 and got[0] == (1 if e == 0 else 0) and got[3] == (1 if e % 2 == 0 else n - 1)
            assert M.expected_isone(n, xs, e)[1] == 1
        inv = M.coprime_operands(n, inst, 9)
        assert M.expected_modmul(n, inv, M.expected_modinv(n, inv)) == [1] * 9
        assert M.expected_modmul(n, xs, [5]) == M.expected_modmul_const(n, xs, 5) == M.expected_modmul_const_sel(n, xs, None, 5, [1] * 67)
        es = M.row_exponents(5, 67)
        assert es[:3] == [0, 1, 31] and M.expected_modexp_var(n, xs, es)[:3] == [1, 1, pow(2, 31, n)]
        assert M.expected_modexp_var(n, xs[:3], [1, 1, 1], dest=[2, 0, 1]) == [1, 2, 0]
        assert M.expected_fixedbase_pow(n, 3, [0, 1, 2]) == [1, 3, 9]
        assert M.expected_isone_any(n, [1, 2, 2, 2], 1, 2) == [1, 0]
        big = 1000003
        enc = M.expected_paillier_encrypt_raw(big, [0, 1, big + 2])
        assert enc == [1, 1 + big, 1 + 2 * big]
        assert M.expected_modmul(big * big, enc, M.expected_paillier_encrypt_raw(big, [0, 1, big + 2], negate=True)) == [1, 1, 1]
        assert M.expected_paillier_l_mul(big, 7, enc) == [0, 7, 14]
        assert M.expected_crt_combine(7, 11, [3], [5]) == [38]
        lo, hi = M.expected_select_finish_cx(n, [2], [3], [11], [5], [7])
        assert (lo, hi) == ([7 * 4 * 11 % n], [5 * 9 * 11 % n])
        assert M.expected_modexp_var_sq(n, [[2, 3], [5, 7]], [[1, 2], [3, 0]], [1, 2]) == [2 * 125 % n, 9 * 2 % n]
        # DGK step 4 with every flag clear and beta = alpha = 0: c_-1 and c_i follow the oracle
        out = M.expected_dgk_step4(n, 3, 1, [[1]], [1], [0], [0], [0], [0])
        assert len(out) == 2 and len(out[0]) == 1
    assert M.counts_for(("vm", 16, 18, 29, False, False, False)) == [1, 3, 4, 5, 11]
    assert M.counts_for(M.VM[-1]) == [1, 63, 64, 65, 131]
    assert M.over_one_round(M.VM[-1], 256) == 256 * 16 * 64 + 65 and all(math.gcd(M.TILE, 64 // g) == 1 for g in (1, 2, 4, 8, 16))
    assert M.pair9_counts(("pvm", 8, 9, 29, False, False, False), 256) == [65, 71, 72, 73, 83]

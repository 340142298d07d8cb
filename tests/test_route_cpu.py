"""csrc/sc_route.h, the host policy that picks the k_vm / k_pvm instance of a launch, against its independent restatement in Python
(tests/_instance_matrix.py, tests/_odd_keys.py) -- without a GPU and without the library: a small program that includes the header
alone is built with g++ and answers every query of this module in one run.  Comparison is by equality.

The header holds single rules; what sc_lib.hip does with them in sequence (one-lane twin, then k_vm instance; small-batch pair twin,
else pair twin, then the multiple M = c n, then k_pvm instance) is followed here by `vm_route` / `pvm_route`: every rule such a
route may need is asked up front, and the route picks among the answers the way the library does."""
import os
import shutil
import subprocess

import pytest

import _instance_matrix as M
import _odd_keys as O
from conftest import ROOT

CSRC = os.path.join(ROOT, "protocols", "secure_comparison_amd", "csrc")
NUM_CU = 256

PROGRAM = r"""
#include "sc_route.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace sc_host;

static void put(const Config* c) { if (c) printf("%d %d %d\n", c->G, c->L, c->W); else printf("-\n"); }
static void put(const Instance& k) { printf("%d %d %d %d\n", k.G, k.L, k.W, (int)k.neg1); }
static void put(bool b) { printf("%d\n", (int)b); }

int main() {
  std::string line, cmd;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    long long v[12] = {0};
    int n = 0;
    in >> cmd;
    while (n < 12 && in >> v[n]) n++;
    // a modulus (G L W neg1) comes first, then the switches (latency one-lane chip-share num_cu), then the rest
    const Config c = {(int)v[0], (int)v[1], (int)v[2], false};
    const Instance m = {(int)v[0], (int)v[1], (int)v[2], v[3] != 0};
    const Policy p = {(int)v[4], (int)v[5], (int)v[6], (int)v[7]};
    const uint64_t count = (uint64_t)v[8];
    if (cmd == "fit") put(first_fit((int)v[0], (int)v[1], v[2] != 0));
    else if (cmd == "forced") put(forced_fit(c, (int)v[3]));
    else if (cmd == "capable") put(pair_capable(c.G, c.L, c.W));
    else if (cmd == "fits") put(fits(c, (int)v[3], (int)v[4], v[5] != 0));
    else if (cmd == "small") put(small_batch(m, p, count));
    else if (cmd == "vm") put(vm_instance(m, p, count));
    else if (cmd == "pvm") put(pvm_instance(m, p, count));
    else if (cmd == "latpair") put(latency_pair_config(m, (int)v[9], (int)v[10], p, count));
    else if (cmd == "cand") put(neg1_candidate(m, (int)v[4]));
    else if (cmd == "negvm") put(neg1_vm_allowed(m, p, count));
    else if (cmd == "onelane") put(onelane_eligible(m, (int)v[4], (int)v[5]));
    else if (cmd == "hasvm") put(has_vm(m.G, m.L, m.W, m.neg1));
    else if (cmd == "haspvm") put(m.W == kPairW && has_pvm(m.G, m.L, m.neg1, v[4] != 0, v[5] != 0));
    else if (cmd == "cost") {
      const OneLaneCal cal;
      const OneLaneCost k = onelane_cost(cal, (uint64_t)v[0], (int)v[1], (int)v[2]);
      printf("%.17g %.17g %d\n", k.one, k.two, (int)onelane_faster(cal, (uint64_t)v[0], (int)v[1], (int)v[2]));
    } else { fprintf(stderr, "unknown query: %s\n", line.c_str()); return 2; }
  }
  return 0;
}
"""


class Queries:
    """Collects the queries of one run; `ask` returns a handle whose `.value` is the answer once `run` has been called."""

    class Handle:
        value = None

    def __init__(self):
        self.lines, self.handles = [], []

    def ask(self, cmd, *args):
        self.lines.append(" ".join([cmd] + [str(int(a)) for a in args]))
        self.handles.append(self.Handle())
        return self.handles[-1]

    def run(self, exe):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(self.lines)
        for h, line in zip(self.handles, out):
            h.value = None if line == "-" else tuple(float(t) if "." in t or "e" in t else int(t) for t in line.split())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    d = tmp_path_factory.mktemp("route")
    src, out = d / "route.cpp", d / "route"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", CSRC, str(src), "-o", str(out)], check=True)
    return str(out)


def shape(cfg, n, w=M.W):
    """(G, L, W, n = -1 mod 2^W): a registered modulus as the policy sees it."""
    return (cfg[0], cfg[1], w, n % (1 << w) == (1 << w) - 1)


def vm_route(q, n, words, latency, onelane, share, count):
    """modexp_shared_impl with an exponent of more than 64 bits: onelane_for, then run_vm."""
    bits, own = n.bit_length(), M.first_fit(n.bit_length(), words)
    pol = (latency, onelane, share, NUM_CU)
    eligible = q.ask("onelane", *shape(own, n), bits, words)
    twin = q.ask("forced", *M.ONE_LANE, bits)
    on_twin = q.ask("vm", *shape(M.ONE_LANE[:2], n, M.ONE_LANE[2]), *pol, count)
    on_own = q.ask("vm", *shape(own, n), *pol, count)

    def answer():
        assert onelane in (0, 2)                     # mode 1 asks the measured round times: test_onelane_comparison
        if onelane == 2 and eligible.value == (1,):
            assert twin.value == M.ONE_LANE
            return ("vm",) + on_twin.value[:3] + (bool(on_twin.value[3]),)
        return ("vm",) + on_own.value[:3] + (bool(on_own.value[3]),)
    return answer


def pvm_route(q, n, words, latency, share, count):
    """sc_modexp_shared_sq: latency_pair_twin, else pair_twin; neg1_twin unless the small-batch rule holds; then run_pvm."""
    bits, own = n.bit_length(), M.first_fit(n.bit_length(), words)
    pol = (latency, 0, share, NUM_CU)
    capable = q.ask("capable", own[0], own[1], M.W)
    lat = q.ask("latpair", *shape(own, n), *pol, count, bits, words)
    pair_fit = q.ask("fit", bits, words, 1)
    pcfg = own if M.pair_capable(*own) else M.first_fit(bits, words, for_pairs=True)
    mult = M.neg1_multiple(n)
    small = q.ask("small", *shape(pcfg, n), *pol, count)
    cand = q.ask("cand", *shape(pcfg, n), bits)
    whole = q.ask("fits", pcfg[0], pcfg[1], M.W, mult.bit_length(), M.nwords_of(mult.bit_length()), 1)
    on_lat = q.ask("pvm", 4 * own[0], 5, M.W, shape(own, n)[3], *pol, count)
    on_pair = q.ask("pvm", *shape(pcfg, n), *pol, count)
    on_mult = q.ask("pvm", pcfg[0], pcfg[1], M.W, 1, *pol, count)

    def answer():
        assert capable.value == (int(M.pair_capable(*own)),)
        if lat.value is not None:
            assert lat.value == (4 * own[0], 5, M.W)
            k = on_lat.value
        else:
            assert capable.value == (1,) or pair_fit.value == pcfg + (M.W,)
            k = on_mult.value if small.value == (0,) and cand.value == (1,) and whole.value == (1,) else on_pair.value
        return ("pvm",) + k[:3] + (bool(k[3]),)
    return answer


def matrix_instances():
    return [i for i in M.INSTANCES if not i[5] and not i[6]]          # STAMP and DIG: not what expected_instance describes


def test_header_is_plain_cxx_without_the_gpu_runtime():
    text = open(os.path.join(CSRC, "sc_route.h")).read()
    assert "hip_runtime" not in text and "sc_ctx" not in text.replace("sc_ctx_set_", "") and "namespace sc_host" in text
    assert [ln for ln in text.splitlines() if ln.startswith("#include")] == ["#include <cmath>", "#include <cstdint>"]
    assert '#include "sc_route.h"' in open(os.path.join(CSRC, "sc_internal.h")).read()


def test_first_fit(exe):
    q, asked = Queries(), []
    for bits in range(M.MIN_BITS, M.MAX_BITS + 2):
        for words in (M.nwords_of(bits), M.nwords_of(bits) + 1):
            for for_pairs in (False, True):
                asked.append((bits, words, for_pairs, q.ask("fit", bits, words, for_pairs)))
    q.run(exe)
    for bits, words, for_pairs, h in asked:
        want = M.first_fit(bits, words, for_pairs)
        assert h.value == (want + (M.W,) if want else None), (bits, words, for_pairs)
    assert M.first_fit(M.MAX_BITS + 1) is None and M.first_fit(M.MAX_BITS) == (16, 18)


def matrix_routes(q):
    """The single-modulus and the pair route of every matrix case at every matrix batch size: (where, the instance the matrix expects,
    the route's answer once `q` has run)."""
    asked = []
    for inst in matrix_instances():
        for c in M.cases_for(inst):
            words = M.nwords_of(c.bits)
            for count in (M.pair9_counts(inst, NUM_CU) if c.pair9 else M.counts_for(inst)):
                where = (M.instance_id(inst), c.label, count)
                asked.append((where, M.expected_instance(c, "pvm"), pvm_route(q, c.n, words, c.latency, c.chip_share, count)))
                if not c.pair9:         # the k_pvm<2G, 9> window is a statement about pair calls only
                    asked.append((where, M.expected_instance(c, "vm"), vm_route(q, c.n, words, c.latency, c.onelane, c.chip_share, count)))
    return asked


def test_matrix_instances(exe):
    q = Queries()
    asked = matrix_routes(q)
    q.run(exe)
    for where, want, answer in asked:
        assert answer() == want, where
    assert len(asked) > 2000


def test_every_matrix_route_lands_on_a_compiled_instance(exe):
    """Where the policy sends a launch, the header's own list has a kernel: has_vm / has_pvm of every route's instance."""
    q = Queries()
    asked = matrix_routes(q)
    q.run(exe)
    q2, has = Queries(), []
    for where, _, answer in asked:
        kind, g, l, w, neg1 = answer()
        has.append((where, q2.ask("has" + kind, g, l, w, neg1, 0, 0)))
    absent = [q2.ask("hasvm", 16, 27, M.W, 0), q2.ask("haspvm", 8, 18, M.W, 1, 0, 0), q2.ask("haspvm", 4, 18, 28, 0, 0, 0),
              q2.ask("haspvm", 4, 18, M.W, 0, 1, 0), q2.ask("haspvm", 16, 18, M.W, 0, 0, 1)]
    q2.run(exe)
    assert len(has) == 2425
    for where, h in has:
        assert h.value == (1,), where
    assert [h.value for h in absent] == [(0,)] * 5


def test_matrix_cases_land_on_their_instance(exe):
    """The same routes against the instance itself, as tests/test_instance_matrix_cpu.py asks of the Python model; the "multiple"
    cases reach k_vm<4,18,NEG1> through neg1_vm_twin (sc_modexp_var)."""
    q, asked = Queries(), []
    pol = (0, 0, 1, NUM_CU)
    for inst in matrix_instances():
        for c in M.cases_for(inst):
            count, words, where = M.counts_for(inst)[-1], M.nwords_of(c.bits), (M.instance_id(inst), c.label)
            if c.pair9:
                count = M.pair9_counts(inst, NUM_CU)[0]
            if "multiple" in c.label:
                mult = M.neg1_multiple(c.n)
                hs = [q.ask("negvm", *shape(c.primary, c.n), *pol, count), q.ask("cand", *shape(c.primary, c.n), c.bits),
                      q.ask("fits", *c.primary, M.W, mult.bit_length(), M.nwords_of(mult.bit_length()), 1)]
                on_mult = q.ask("vm", *shape(c.primary, mult), *pol, count)
                asked.append((where, inst[:5], lambda hs=hs, k=on_mult: [h.value for h in hs] == [(1,)] * 3 and ("vm",) + k.value[:3] + (bool(k.value[3]),)))
            elif inst[0] == "vm":
                asked.append((where, inst[:5], vm_route(q, c.n, words, c.latency, c.onelane, c.chip_share, count)))
            else:
                asked.append((where, inst[:5], pvm_route(q, c.n, words, c.latency, c.chip_share, count)))
    q.run(exe)
    for where, want, answer in asked:
        assert answer() == want, where
    assert len(asked) > 200


def test_neg1_multiple(exe):
    q, asked = Queries(), []
    moduli = {c.n for inst in matrix_instances() for c in M.cases_for(inst)} | {M.make_modulus(b, s) for b in (1587, 3211) for s in ("one", "rand")}
    for n in sorted(moduli):
        cfg, mult = M.pair_config(n.bit_length()), M.neg1_multiple(n)
        asked.append((n, cfg, q.ask("cand", *shape(cfg, n), n.bit_length()),
                      q.ask("fits", *cfg, M.W, mult.bit_length(), M.nwords_of(mult.bit_length()), 1)))
    q.run(exe)
    yes = 0
    for n, cfg, cand, whole in asked:
        got = cand.value == (1,) and whole.value == (1,)
        assert got == M.has_neg1_multiple(n, cfg), (n.bit_length(), cfg)
        yes += got
        if n.bit_length() in (1587, 3211) and not M.is_neg1(n):           # cap - 37 bits: a candidate whose M needs one word too many
            assert cand.value == (1,) and whole.value == (0,) and cfg == {1587: (4, 14), 3211: (8, 14)}[n.bit_length()]
    assert 20 < yes < len(asked) - 20


def test_onelane_eligibility(exe):
    q = Queries()
    asked = [(bits, q.ask("onelane", *shape(M.first_fit(bits), (1 << bits) - 3), bits, M.nwords_of(bits))) for bits in range(M.MIN_BITS, 1101)]
    own_width = q.ask("onelane", *M.ONE_LANE, 0, 512, 16)                  # the twin itself has no twin
    q.run(exe)
    for bits, h in asked:
        assert h.value == (int(M.onelane_fits(bits)),), bits
    assert dict(asked)[1024].value == (1,) and dict(asked)[M.ONE_LANE_UNREACHABLE_BITS].value == (0,) and own_width.value == (0,)


def test_odd_keys(exe):
    q, asked = Queries(), []
    for key in O.load().values():
        for name, (n, words) in O.moduli(key).items():
            where = (key.bits, name)
            own = q.ask("fit", n.bit_length(), words, 0)
            asked.append((where, O.config(n, words) + (M.W,), lambda h=own: h.value))
            pair = q.ask("fit", n.bit_length(), words, 1)
            capable = q.ask("capable", *O.config(n, words), M.W)
            asked.append((where, O.pair_config(n, words) + (M.W,), lambda o=own, p=pair, c=capable: o.value if c.value == (1,) else p.value))
            for count in (1, 4096):
                asked.append((where, O.pvm(n, words)[:5], pvm_route(q, n, words, 0, 1, count)))
    q.run(exe)
    assert len(asked) == 6 * 6 * 4
    for where, want, answer in asked:
        assert answer() == want, where


def test_onelane_comparison(exe):
    """Full rounds plus one partial round per form, on the built-in round times 1.0 / 0.5 / 0.6 / 0.27 / 0.38 and 256 CUs."""
    table = [(196608, 1, 1.5, 1.8, 1), (98304, 1, 1.0, 0.87, 0), (131072, 1, 1.0, 1.2, 1), (32768, 1, 0.5, 0.38, 0), (98304, 2, 1.5, 1.8, 1)]
    q = Queries()
    hs = [q.ask("cost", count, share, NUM_CU) for count, share, _, _, _ in table]
    q.run(exe)
    for (count, share, one, two, faster), h in zip(table, hs):
        assert h.value[0] == pytest.approx(one, abs=1e-12) and h.value[1] == pytest.approx(two, abs=1e-12) and h.value[2] == faster, (count, share)


def test_small_batch_rule_at_its_edge(exe):
    q = Queries()
    m418 = (4, 18, M.W, 0)
    edge = 512 * 16                                                          # 2 num_cu waves of 64 / 4 items
    want = [(q.ask("small", *m418, 1, 0, 1, NUM_CU, edge), 1), (q.ask("small", *m418, 1, 0, 1, NUM_CU, edge + 1), 0)]
    for count in (1, edge, edge + 1, 1 << 30):
        want += [(q.ask("small", *m418, 0, 0, 1, NUM_CU, count), 0), (q.ask("small", *m418, 2, 0, 1, NUM_CU, count), 1)]
        want += [(q.ask("small", 16, 18, M.W, 0, mode, 0, 1, NUM_CU, count), 0) for mode in (0, 1, 2)]
    q.run(exe)
    assert [h.value for h, _ in want] == [(w,) for _, w in want]

// Which k_vm / k_pvm instances exist and which of them a call lands on: the list of every compiled instance, the configurations a
// modulus can have, the fit rule, and every rule that sends a launch to another instance or to a twin context of its modulus -- the
// small-batch forms, the pair twins, the multiple M = c n and the one-lane form.  Pure functions of plain numbers: no GPU runtime,
// no context and no allocation in here, so that a stand-alone host program can include this file alone (tests/test_route_cpu.py
// compares it with the Python restatement in tests/_instance_matrix.py and tests/_odd_keys.py on a machine without a GPU, and
// tests/test_instance_matrix_cpu.py prints the list from it).  sc_lib.hip asks these functions and keeps what needs a context: the
// twin registry, the big-integer work of M = c n and the calibration launches.
#pragma once
#include <cmath>
#include <cstdint>

// ---- the instances ---------------------------------------------------------------------------------------------------------------
// Every instance of the two interpreters that the library compiles, once: a row per instance, a list per compilation unit
// (sc_launch_vm.hip / sc_launch_pvm.hip with -DSC_PART=0/1/2 expand their own part and nothing else, in this order), and the list of
// all parts.  What reads it: the launchers, the table of keys below with has_vm / has_pvm, through them the policy and the
// static_asserts after the rules, and the list that tests/test_instance_matrix_cpu.py prints.
// k_vm, X(G, L, W, NEG1); NEG1: a modulus = -1 (mod 2^W), no quotient multiply
#define SC_VM_PART0(X) X(4, 18, 29, true) X(4, 18, 29, false) X(2, 18, 29, false) X(1, 18, 29, false) X(2, 9, 29, false) X(4, 9, 29, false)
#define SC_VM_PART1(X) X(1, 37, 28, false) X(8, 18, 29, false) X(16, 18, 29, false) X(8, 9, 29, false) X(16, 9, 29, false) X(2, 27, 29, false)
#define SC_VM_PART2(X) X(4, 27, 29, false) X(8, 27, 29, false) X(4, 14, 29, false) X(8, 14, 29, false) X(16, 14, 29, false)
#define SC_VM_INSTANCES(X) SC_VM_PART0(X) SC_VM_PART1(X) SC_VM_PART2(X)
// k_pvm, X(G, L, NEG1, STAMP, DIG), all with kPairW-bit limbs; STAMP: the diagnostic twin of (4,18,NEG1) that sc_clock_probe
// launches; DIG: the instances with PV_MULTDIG (sc_modexp_var_sq), the pair configurations of Paillier moduli N -- (2,18) for
// 1024-bit, (4,18) for 2048-bit, (8,14) for 3072-bit N -- without the latency and n = -1 (mod 2^29) variants
#define SC_PVM_PART0(X) \
  X(4, 18, true, true, false) X(4, 18, true, false, false) X(4, 18, false, false, false) X(2, 18, false, false, false) X(1, 18, false, false, false) \
  X(2, 18, false, false, true) X(4, 18, false, false, true)
#define SC_PVM_PART1(X) \
  X(8, 18, false, false, false) X(16, 18, false, false, false) X(2, 9, false, false, false) X(4, 9, false, false, false) X(8, 9, false, false, false) \
  X(4, 5, false, false, false) X(8, 5, false, false, false) X(16, 5, false, false, false)
#define SC_PVM_PART2(X) \
  X(4, 14, true, false, false) X(4, 14, false, false, false) X(8, 14, true, false, false) X(8, 14, false, false, false) X(8, 14, false, false, true)
#define SC_PVM_INSTANCES(X) SC_PVM_PART0(X) SC_PVM_PART1(X) SC_PVM_PART2(X)

namespace sc_host {

constexpr int kPairW = 29;
// The key of an interpreter instance: in the launch counts of a context (the packing include/sc_amd_dev.h documents), in its cache of
// occupancy answers, and in the launchers' tables.  The fields do not overlap for G, L, W below 256.
constexpr uint32_t launch_key(bool pvm, int G, int L, int W, bool neg1, bool stamp, bool dig) {
  return (uint32_t)L | ((uint32_t)G << 8) | ((uint32_t)W << 16) | (neg1 ? 1u << 24 : 0u) | (stamp ? 1u << 25 : 0u) | (dig ? 1u << 26 : 0u) |
         (pvm ? 1u << 27 : 0u);
}
// the key of a k_prod_axis instance there: bit 28 set, L, G and W where the interpreters have them
constexpr uint32_t reduce_launch_key(int G, int L) { return (uint32_t)L | ((uint32_t)G << 8) | (29u << 16) | (1u << 28); }
// ... and of a k_scan_axis instance: bit 29 set
constexpr uint32_t scan_launch_key(int G, int L) { return (uint32_t)L | ((uint32_t)G << 8) | (29u << 16) | (1u << 29); }
// ... and of a k_lin_axis instance: bit 30 set; with bit 24 its lifting launch k_lin_lift
constexpr uint32_t lin_launch_key(int G, int L, bool lift) { return (uint32_t)L | ((uint32_t)G << 8) | (29u << 16) | (1u << 30) | (lift ? 1u << 24 : 0u); }

#define SC_VM_KEY(G, L, W, NEG1) launch_key(false, G, L, W, NEG1, false, false),
#define SC_PVM_KEY(G, L, NEG1, STAMP, DIG) launch_key(true, G, L, kPairW, NEG1, STAMP, DIG),
constexpr uint32_t kInstanceKeys[] = {SC_VM_INSTANCES(SC_VM_KEY) SC_PVM_INSTANCES(SC_PVM_KEY)};
#undef SC_VM_KEY
#undef SC_PVM_KEY
constexpr bool has_instance(uint32_t key) {
  for (uint32_t k : kInstanceKeys)
    if (k == key) return true;
  return false;
}
constexpr bool has_vm(int G, int L, int W, bool neg1) { return has_instance(launch_key(false, G, L, W, neg1, false, false)); }
constexpr bool has_pvm(int G, int L, bool neg1, bool stamp, bool dig) { return has_instance(launch_key(true, G, L, kPairW, neg1, stamp, dig)); }

struct Config { int G, L, W; bool primary; };   // primary: eligible as a modulus's own configuration (sc_mod_create)
// ordered by capacity W*G*L; sc_mod_create takes the first one that fits.  A 28-bit-limb L = 37 family ((2,37), (4,37)) was
// built and measured in round 1: it needs > 256 registers (one wave per SIMD plus AGPR copies) and came out 2-3 % slower
// than (4,18) / (8,18), so it is not compiled in; the limb width stays a template parameter for such experiments.
constexpr Config kConfigs[] = {{1, 18, 29, true}, {2, 18, 29, true}, {2, 27, 29, true}, {4, 14, 29, true}, {4, 18, 29, true}, {4, 27, 29, true},
                           {8, 14, 29, true}, {8, 18, 29, true}, {8, 27, 29, true}, {16, 14, 29, true}, {16, 18, 29, true}};
// The one-lane configuration for moduli up to 1028 bits (the primes of 2048-bit Paillier / DGK keys): (1, 37) with 28-bit limbs.
// A number lives in ONE lane, so the per-limb-step bookkeeping is paid once per number instead of once per lane of a group, the
// operand of a squaring never leaves the registers and the modulus sits in scalar registers: 1.15 - 1.25x the (2, 18) rate
// per number.  It needs 64 numbers per wave, i.e. large batches, and is therefore never a modulus's own configuration: the
// shared-exponent entry points switch to an internal twin context of the same modulus when the batch fills the chip
// (onelane_for, sc_ctx_set_onelane_mode).
constexpr Config kOneLane = {1, 37, 28, false};
// configurations with a pair kernel (k_pvm): every L = 18 one, and (4,14) / (8,14) for the 1536 / 3072-bit sizes whose direct
// configuration is L = 27 (the pair arithmetic needs the L <= 18 column bound)
// (the one-lane (1, 37, 28) configuration has no pair kernel: measured on the MI355X its pair squarings run 3 % faster than the
// (2, 18) ones but its pair products -- three passes over a single LDS staging area, the second area would cost the eighth wave
// of the CU -- 2.6x a squaring instead of 1.4x, a net loss of 12 % on x^p mod p^2; the one-lane form is used where it wins:
// the single-modulus exponentiations)
// (8,5) / (16,5): the SMALL-BATCH pair configurations of 1024 / 2048-bit moduli (kLatencyPair below)
constexpr bool pair_capable(int G, int L, int W) { return W == 29 && (L == 18 || (L == 14 && (G == 4 || G == 8)) || (L == 5 && (G == 4 || G == 8 || G == 16))); }
// Small batches of pair exponentiations (Alice's rho^N mod N^2, the key holder's c^(p-1) mod p^2 at B = 4096) are one dependent
// chain of ~2400 pair squarings per item, and a wave's time per squaring is its own instruction count: S limb steps of
// (L + L/2) multiply-adds + ~7 bookkeeping instructions each, whatever the number of lanes.  When even the (2G, 9) form
// leaves half of the SIMDs without a wave, 4x the lanes with 5 limbs each -- (16,5) for 2048-bit, (8,5) for 1024-bit moduli,
// S = 80 / 40 limbs -- shorten every limb step from ~22 to ~15 instructions at a multiply-add density (45 %) that would be
// wasteful on a full chip but costs nothing on an empty one.  A twin context of the same modulus, like the other twins.
constexpr Config kLatencyPair16 = {16, 5, 29, false}, kLatencyPair8 = {8, 5, 29, false}, kLatencyPair4 = {4, 5, 29, false};   // (4,5): 512-bit primes of 1024-bit keys

// ---- the fit rule ----------------------------------------------------------------------------------------------------------------
// A modulus of nbits bits fits a configuration that leaves 8 guard bits below R = 2^(W G L).  whole_words: the nwords words it is
// stored in must lie below R as well -- a wide operand is read in raw chunks of that many words, and bits of a chunk at or above R
// are dropped by the limb conversion.  Every twin is asked for both; a modulus's own configuration prefers both (first_fit).
inline bool fits(const Config& c, int nbits, int nwords, bool whole_words) {
  const int cap = c.W * c.G * c.L;
  return cap >= nbits + 8 && (!whole_words || cap >= 32 * nwords);
}
// The first configuration (for_pairs: the first with a pair kernel) that fits in whole words, else the first that fits at all.
inline const Config* first_fit(int nbits, int nwords, bool for_pairs) {
  for (int pass = 0; pass < 2; pass++)
    for (const Config& c : kConfigs)
      if (c.primary && (!for_pairs || pair_capable(c.G, c.L, c.W)) && fits(c, nbits, nwords, pass == 0)) return &c;
  return nullptr;
}
// This configuration or none (the twins, which have tested the whole words themselves).
inline const Config* forced_fit(const Config& c, int nbits) { return fits(c, nbits, 0, false) ? &c : nullptr; }

// ---- what the rules are asked with -----------------------------------------------------------------------------------------------
// the switches and sizes of a context that the policy reads (sc_ctx_set_latency_mode, sc_ctx_set_onelane_mode, sc_ctx_set_chip_share)
struct Policy { int latency_mode, onelane_mode, chip_share, num_cu; };
// A modulus as the policy sees it -- its configuration, and whether n = -1 (mod 2^W), i.e. n0inv == 1 -- and equally the kernel
// instance a launch takes, where neg1 names the instance without the quotient multiply.
struct Instance { int G, L, W; bool neg1; };

// ---- the small-batch rule ----------------------------------------------------------------------------------------------------------
// Small batches: an L = 18 configuration with count * G lanes fills only part of the chip, and the run time is the latency of
// one wave's chain of products.  The same limb arrays (S = G L limbs, identical layout in memory) can be worked on by twice
// the lanes with half the limbs each -- (2G, 9) -- which doubles the waves and shortens the chain by 1.8x; the multiply-add
// density drops from 88 % to 78 % of the instruction stream, so this is used only while the L = 18 launch would leave at
// least half of the SIMDs without a wave.
inline bool small_batch(const Instance& m, const Policy& p, uint64_t count) {
  if (p.latency_mode == 0 || m.L != 18 || m.W != 29 || m.G > 8) return false;
  if (p.latency_mode == 2) return true;
  const uint64_t waves = (count + (64 / m.G) - 1) / (64 / m.G);
  return waves <= (uint64_t)p.num_cu * 2;
}

// ---- the instance of a launch ----------------------------------------------------------------------------------------------------
// Where an instance without the quotient multiply exists, a modulus = -1 (mod 2^W) takes it; the list is that rule.  Today its
// NEG1 rows are k_vm (4,18,29) and k_pvm (4,18), (4,14), (8,14): the truth tables of has_vm(G, L, W, true) and
// has_pvm(G, L, true, false, false) are, for every input, those of the tests `G == 4 && L == 18 && W == 29` and
// `(G == 4 && L == 18) || (L == 14 && (G == 4 || G == 8))` that stood here before.
// k_vm: the (2G, 9) form under the small-batch rule; a (4,18) modulus = -1 (mod 2^29) -- in practice the multiple M = c n of
// neg1_twin -- runs the instance without the quotient multiply
inline Instance vm_instance(const Instance& m, const Policy& p, uint64_t count) {
  const bool lat = small_batch(m, p, count);
  const int G = lat ? 2 * m.G : m.G, L = lat ? 9 : m.L;
  return {G, L, m.W, has_vm(G, L, m.W, true) && m.neg1};
}
// k_pvm: which instance a launch of `count` items of modulus m takes
inline Instance pvm_instance(const Instance& m, const Policy& p, uint64_t count) {
  int G = m.G, L = m.L;
  if (small_batch(m, p, count) && (m.G == 1 || m.G == 2 || m.G == 4)) { G = 2 * m.G; L = 9; }   // (2,9): the 512-bit primes of 1024-bit keys (BASELINE configs[0])
  return {G, L, m.W, m.neg1 && has_pvm(G, L, true, false, false)};
}

// ---- the twins ---------------------------------------------------------------------------------------------------------------------
// The small-batch pair twin ((16,5) for a (4,18) modulus, (8,5) for a (2,18) one, (4,5) for a (1,18) one) when this batch should run
// on it, else null.  Automatic policy: the (2G, 9) launch would still leave at least half of the SIMDs without a wave.
inline const Config* latency_pair_config(const Instance& m, int nbits, int nwords, const Policy& p, uint64_t count) {
  if (p.latency_mode == 0) return nullptr;
  if (m.W != 29 || m.L != 18 || (m.G != 1 && m.G != 2 && m.G != 4)) return nullptr;
  const Config* cfg = (m.G == 4) ? &kLatencyPair16 : (m.G == 2 ? &kLatencyPair8 : &kLatencyPair4);
  const uint64_t per_wave = 64 / (2 * m.G), waves = (count + per_wave - 1) / per_wave;
  if (p.latency_mode == 1 && waves > (uint64_t)p.num_cu * 2 / (uint64_t)p.chip_share) return nullptr;
  return fits(*cfg, nbits, nwords, true) ? cfg : nullptr;
}
// Is the multiple M = c n, c = -n^-1 mod 2^29, worth building for this modulus?  Its configuration has a NEG1 pair kernel, n is not
// = -1 already, and the 8 guard bits are left whatever c is (M has at most 29 more bits than n).  M itself must then pass
// fits(.., whole words) in the same configuration: a 1587-bit modulus on (4,14) gave an M of 51 words for 1624 limb bits.
inline bool neg1_candidate(const Instance& m, int nbits) {
  return m.W == 29 && has_pvm(m.G, m.L, true, false, false) && !m.neg1 && nbits + 29 + 8 <= m.W * m.G * m.L;
}
// The single-modulus interpreter runs modulo M only as k_vm<4,18,29,true>, and not under the small-batch rule.
inline bool neg1_vm_allowed(const Instance& m, const Policy& p, uint64_t count) {
  return m.W == 29 && m.L == 18 && m.G == 4 && !small_batch(m, p, count);
}
// The one-lane twin exists for moduli of another limb width whose residue arrays (and the raw chunks a wide operand is read in) fit
// below R = 2^(28 * 37): at most 32 words.
inline bool onelane_eligible(const Instance& m, int nbits, int nwords) { return m.W != kOneLane.W && fits(kOneLane, nbits, nwords, true); }

// ---- the one-lane comparison -----------------------------------------------------------------------------------------------------
// Both forms run in rounds of their resident waves: 2 waves per SIMD, 64 numbers per one-lane wave and 32 per two-lane wave.  What a
// batch costs in either form is a sum of full rounds plus one partial round, and a partial round that leaves every SIMD at most one
// wave costs about half -- how much exactly depends on the part, so the round times are measured per device (sc_lib.hip:
// onelane_calibrate); the defaults are round 3's constants, fitted on one box (0.6 / 0.27 / 0.38 of a one-lane round).
struct OneLaneCal { bool ok = false; double one_full = 1.0, one_half = 0.5, two_full = 0.6, two_half = 0.27, two_only_half = 0.38; int simds = 0; };
struct OneLaneCost { double one, two; };
// Rounds are counted on this context's share of the chip (sc_ctx_set_chip_share): the idle SIMDs of an under-filled launch are taken
// by the other contexts' kernels.
inline OneLaneCost onelane_cost(const OneLaneCal& c, uint64_t count, int chip_share, int num_cu) {
  const double share = (double)chip_share / ((double)num_cu * 4 * 2 * 64);
  const double r1 = (double)count * share, r2 = 2.0 * r1;
  const double f1 = r1 - std::floor(r1), f2 = r2 - std::floor(r2);
  const double one = c.one_full * std::floor(r1) + (f1 <= 0.0 ? 0.0 : (f1 <= 0.5 ? c.one_half : c.one_full));
  const double two = c.two_full * std::floor(r2) + (f2 <= 0.0 ? 0.0 : (f2 <= 0.5 ? (r2 < 1.0 ? c.two_only_half : c.two_half) : c.two_full));
  return {one, two};
}
// a tie keeps the two-lane form
inline bool onelane_faster(const OneLaneCal& c, uint64_t count, int chip_share, int num_cu) {
  const OneLaneCost k = onelane_cost(c, count, chip_share, num_cu);
  return !(k.one >= k.two);
}

// ---- the rules against the list -------------------------------------------------------------------------------------------------
// A configuration that a rule above can pick and no part compiles does not build.
constexpr bool every_own_configuration_has_its_vm() {
  for (const Config& c : kConfigs)
    if (c.primary && !has_vm(c.G, c.L, c.W, false)) return false;
  return has_vm(kOneLane.G, kOneLane.L, kOneLane.W, false);
}
constexpr bool every_small_batch_form_has_its_vm() {
  for (const Config& c : kConfigs)
    if (c.L == 18 && c.W == 29 && c.G <= 8 && !has_vm(2 * c.G, 9, c.W, false)) return false;
  return true;
}
constexpr bool pair_kernel_where_capable(const Config& c) { return !pair_capable(c.G, c.L, c.W) || has_pvm(c.G, c.L, false, false, false); }
constexpr bool every_pair_configuration_has_its_pvm() {
  for (const Config& c : kConfigs)
    if (!pair_kernel_where_capable(c)) return false;
  return pair_kernel_where_capable(kLatencyPair16) && pair_kernel_where_capable(kLatencyPair8) && pair_kernel_where_capable(kLatencyPair4);
}
static_assert(every_own_configuration_has_its_vm(), "a configuration of kConfigs, or kOneLane, has no k_vm instance");
static_assert(every_small_batch_form_has_its_vm(), "an L = 18, G <= 8 configuration has no (2G, 9) k_vm instance");
static_assert(every_pair_configuration_has_its_pvm(), "a pair_capable configuration has no plain k_pvm instance");
static_assert(has_pvm(2, 9, false, false, false) && has_pvm(4, 9, false, false, false) && has_pvm(8, 9, false, false, false),
              "the small-batch form (2G, 9) of G = 1, 2 or 4 has no k_pvm instance");

}  // namespace sc_host

// Host logic that the product along an axis (sc_modprod_axis) and the running product (sc_modscan_axis, 8k) share: the chunk
// rule, the two level plans and the part of the argument check that needs no context.  No HIP and no sc_ctx in here, so that a
// stand-alone host program can include this file alone and run it under a sanitizer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sc_host {

// Chunk length as in modinv_rec: a chain is sequential, so a level's latency is its chunk length while the work (one product per
// member, plus one per partial) hardly depends on it.  The shortest chunks of at least 4 and at most 32 members that still fill every
// resident group slot of the chip at a level of `total` members; `forced` (sc_ctx_set_reduce_chunk, 2 .. 32) overrides that at every
// level.  protocols/secure_comparison_amd/aggregate.py::_axis_chunk mirrors this for the tests.
static inline uint64_t axis_chunk(uint64_t total, uint64_t resident_groups, int forced) {
  return forced ? (uint64_t)forced : std::min<uint64_t>(32, std::max<uint64_t>(4, (total + resident_groups - 1) / resident_groups));
}

// One level of the reduction tree: K members per output in chains of `chunk` (the last one of an output may be shorter),
// nch = ceil(K / chunk) partials.  A level never cuts finer than its K.
struct ReduceLevel { uint64_t K; uint32_t chunk; uint64_t nch; };
static inline std::vector<ReduceLevel> reduce_plan(uint64_t outer, uint64_t K, uint64_t inner, uint64_t resident_groups, int forced) {
  std::vector<ReduceLevel> lv;
  for (;;) {
    const uint64_t c = std::min(axis_chunk(outer * K * inner, resident_groups, forced), K);
    const uint64_t nch = (K + c - 1) / c;
    lv.push_back(ReduceLevel{K, (uint32_t)c, nch});
    if (nch == 1) return lv;
    K = nch;
  }
}

// One level of the blocked scan: K members per scan in chunks of `chunk`, nch = ceil(K / chunk) of them; `members` original members
// stand behind one member of this level (1 at the top), which therefore carries the drift R^-(members - 1).  A blocked level hands the
// totals of its nch - 1 full chunks to the next level; the last level is direct: one chain per scan, no seed.
struct ScanLevel { uint64_t K; uint64_t chunk; uint64_t nch; uint64_t members; bool blocked; };
// Direct when the outer * inner scans fill every resident group slot by themselves, or K is no longer than one chunk; blocked
// otherwise.  A forced chunk length blocks every level longer than itself.
static inline std::vector<ScanLevel> scan_plan(uint64_t outer, uint64_t K, uint64_t inner, uint64_t resident_groups, int forced) {
  std::vector<ScanLevel> lv;
  uint64_t members = 1;
  for (;;) {
    const uint64_t c = axis_chunk(outer * K * inner, resident_groups, forced);
    if ((!forced && outer * inner >= resident_groups) || K <= c) {
      lv.push_back(ScanLevel{K, K, 1, members, false});
      return lv;
    }
    const uint64_t nch = (K + c - 1) / c;
    lv.push_back(ScanLevel{K, c, nch, members, true});
    members *= c;
    K = nch - 1;
  }
}

// What the geometry and the two arrays of a call allow, tested in this order: K >= 1; outer * K * inner * nwords <= 2^40 words, factor
// by factor so that no product wraps; an empty array; `out` (out_rows numbers, read only once the bound holds) must not overlap `x`.
enum AxisVerdict { AXIS_RUN = 0, AXIS_EMPTY, AXIS_NO_MEMBER, AXIS_TOO_LARGE, AXIS_OVERLAP };
static inline AxisVerdict axis_verdict(uint64_t nwords, uint64_t outer, uint64_t K, uint64_t inner, uint64_t out_rows, uintptr_t x, uintptr_t out) {
  if (K < 1) return AXIS_NO_MEMBER;
  const uint64_t LIM = 1ull << 40;
  uint64_t words = nwords;
  for (uint64_t f : {K, outer, inner}) {
    if (f != 0 && words > LIM / f) return AXIS_TOO_LARGE;
    words *= f;
  }
  if (outer == 0 || inner == 0) return AXIS_EMPTY;
  const uint64_t xbytes = words * 4, obytes = out_rows * nwords * 4;
  return (x < out + obytes && out < x + xbytes) ? AXIS_OVERLAP : AXIS_RUN;
}

}  // namespace sc_host

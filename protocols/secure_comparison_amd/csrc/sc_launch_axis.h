// What sc_launch_reduce.hip and sc_launch_scan.hip share: the list of their instances and the launcher of one of them.  Each unit keeps
// its kernel, its argument struct and its dispatch over the list.
#pragma once
#include "sc_internal.h"

// every multi-lane configuration with 29-bit limbs a modulus can have as its own (kConfigs): the instances of k_prod_axis and k_scan_axis
#define SC_AXIS_INSTANCES(X) X(2, 18) X(2, 27) X(4, 14) X(4, 18) X(4, 27) X(8, 14) X(8, 18) X(8, 27) X(16, 14) X(16, 18)

namespace sc_host {

constexpr bool axis_instances_are_the_multi_lane_configs() {
#define SC_AXIS_PAIR(GG, LL) {GG, LL},
  constexpr int axis[][2] = {SC_AXIS_INSTANCES(SC_AXIS_PAIR)};
#undef SC_AXIS_PAIR
  constexpr size_t n = sizeof axis / sizeof *axis;
  size_t i = 0;
  for (const Config& c : kConfigs) {
    if (!c.primary || c.G == 1 || c.W != 29) continue;
    if (i == n || axis[i][0] != c.G || axis[i][1] != c.L) return false;
    i++;
  }
  return i == n;
}
static_assert(axis_instances_are_the_multi_lane_configs(), "SC_AXIS_INSTANCES is not the multi-lane primary rows of kConfigs");

// One wave per workgroup, NG chains per wave, grid-stride over min(nchains / NG, num_cu * occupancy) resident waves on the context's
// stream.  KEY is the instance's key in sc_ctx::launch_counts (reduce_launch_key / scan_launch_key / lin_launch_key).
template <uint32_t KEY, typename Args>
int launch_axis(sc_ctx* ctx, void (*kernel)(Args), int NG, uint64_t nchains, const Args& a) {
  return launch_waves(ctx, KEY, kernel, (nchains + NG - 1) / NG, true, a, [](uint32_t, Args&) { return (int)SC_OK; });
}

}  // namespace sc_host

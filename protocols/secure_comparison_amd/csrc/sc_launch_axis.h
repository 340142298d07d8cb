// What sc_launch_reduce.hip and sc_launch_scan.hip share: the list of their instances and the launcher of one of them.  Each unit keeps
// its kernel, its argument struct and its dispatch over the list.
#pragma once
#include "sc_internal.h"

// every multi-lane configuration with 29-bit limbs a modulus can have as its own (kConfigs): the instances of k_prod_axis and k_scan_axis
#define SC_AXIS_INSTANCES(X) X(2, 18) X(2, 27) X(4, 14) X(4, 18) X(4, 27) X(8, 14) X(8, 18) X(8, 27) X(16, 14) X(16, 18)

namespace {

// One wave per workgroup, NG chains per wave, grid-stride over min(nchains / NG, num_cu * occupancy) resident waves on the context's
// stream.  KEY is the instance's key in sc_ctx::launch_counts (reduce_launch_key / scan_launch_key: bit 28 or 29 set) and in
// occ_cache as well, which the interpreters share: their keys there (10000 G + 10 L + 1000000 W + 0/1 in sc_launch_vm.hip, below
// 1000000 in sc_launch_pvm.hip) stay below 3e7 < 2^28.
template <uint32_t KEY, typename Args>
int launch_axis(sc_ctx* ctx, void (*kernel)(Args), int NG, uint64_t nchains, const Args& a) {
  const int key = (int)KEY;
  int& occ = ctx->occ_cache[key];                  // 0: not asked yet
  if (!occ) {
    int nb = 0;
    HIPCHK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64, 0));
    occ = std::max(1, std::min(nb, 16));
  }
  const uint64_t need = (nchains + NG - 1) / NG, maxb = (uint64_t)ctx->num_cu * occ;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min(need, maxb));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, ctx->stream, a);
  ctx->launch_counts[KEY]++;
  HIPCHK(ctx, hipGetLastError());
  return SC_OK;
}

}  // namespace

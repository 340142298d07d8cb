// k_divmod_words (gfx950) and its launcher: per row, a number of nw words divided by the row's own 64-bit divisor (sc_plain_divmod,
// include/sc_amd_dev.h).  Compiled by sc_launch_misc.hip, which includes this file; the digit loop is
// sc_divmod_words.h.  One thread per row like the other plain-word kernels: the division of a row is a chain (every step needs the
// remainder of the one before), so a row cannot be spread over lanes.  A lane walks its row from the top word down; across a wave the
// loads are nw words apart, each lane in a cache line of its own that its next 31 steps hit again, and the stores of q follow the same
// pattern -- HBM sees every line once.  The kernel is small beside the decryption it follows (section 8r has the figures).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sc_divmod_words.h"

namespace sc {

// q [count][nw] = x div d, rem [count] = x mod d for x [count][nw] and d [count].  q may be x itself (no __restrict__ on the two).  A
// row whose divisor is zero sets *bad, and its q and rem are zero: nothing is divided, nothing faults.
__global__ void k_divmod_words(const uint32_t* x, int nw, const uint64_t* __restrict__ d, uint64_t count, uint32_t* q,
                               uint64_t* __restrict__ rem, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t dv = d[i];
  uint32_t* qi = q + i * nw;
  if (dv == 0) {
    *bad = 1u;
    for (int k = 0; k < nw; k++) qi[k] = 0u;
    rem[i] = 0ull;
    return;
  }
  rem[i] = divmod_row(x + i * nw, nw, dv, qi, nullptr);
}

}  // namespace sc

int sc_host::launch_divmod_words(hipStream_t stream, const uint32_t* x, int nw, const uint64_t* d, uint64_t count, uint32_t* q, uint64_t* rem,
                                 uint32_t* bad) {
  hipLaunchKernelGGL(sc::k_divmod_words, blocks256(count), dim3(256), 0, stream, x, nw, d, count, q, rem, bad);
  return launched();
}

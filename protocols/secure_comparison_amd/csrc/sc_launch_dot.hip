// The plain-word kernels of the secure inner product (k_dot_prep / k_dot_split, sc_kernel_plain.h) behind plain launch functions
// (sc_internal.h) -- a unit of their own beside sc_launch_misc.hip and sc_launch_mul.hip.
#define SC_DOT_UNIT
#include "sc_internal.h"
#include "sc_kernel_plain.h"

using namespace sc;

namespace {
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

int sc_host::launch_dot_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const DotLayout& lay, int nw, int ew,
                             uint64_t count, uint32_t* e, uint32_t* R, uint32_t* S) {
  hipLaunchKernelGGL(k_dot_prep, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, ra, aw, rb, bw, lay, nw, ew, count, e, R, S);
  return launched();
}
int sc_host::launch_dot_split(hipStream_t stream, const uint32_t* p, int nw, const DotLayout& lay, uint64_t count, uint32_t* D, uint32_t* bad) {
  hipLaunchKernelGGL(k_dot_split, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, p, nw, lay, count, D, bad);
  return launched();
}

// The plain-word kernels of the secure multiplication (k_mul_prep / k_mul_split, sc_kernel_plain.h) behind plain launch functions
// (sc_internal.h) -- a unit of their own beside sc_launch_misc.hip.
#define SC_MUL_UNIT
#include "sc_internal.h"
#include "sc_kernel_plain.h"

using namespace sc;

namespace {
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

int sc_host::launch_mul_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const MulLayout& lay, int nw, int ew,
                             uint64_t count, uint32_t* R, uint32_t* e, uint32_t* rab) {
  hipLaunchKernelGGL(k_mul_prep, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, ra, aw, rb, bw, lay, nw, ew, count, R, e, rab);
  return launched();
}
int sc_host::launch_mul_split(hipStream_t stream, const uint32_t* p, int nw, const MulLayout& lay, uint64_t count, uint32_t* prod, uint32_t* bad) {
  hipLaunchKernelGGL(k_mul_split, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, p, nw, lay, count, prod, bad);
  return launched();
}

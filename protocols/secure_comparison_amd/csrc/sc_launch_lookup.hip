// The plain-word kernels of the secure one-hot encoding (k_onehot_prep / k_onehot_split / k_onehot_rotate, sc_kernel_plain.h) behind
// plain launch functions (sc_internal.h) -- a unit of their own beside sc_launch_misc.hip, sc_launch_mul.hip and sc_launch_dot.hip.
#define SC_LOOKUP_UNIT
#include "sc_internal.h"
#include "sc_kernel_plain.h"

using namespace sc;

namespace {
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
// one wave per row, four waves per block
inline dim3 wave_rows(uint64_t rows) { return dim3((unsigned)((rows + 3) / 4)); }
}  // namespace

int sc_host::launch_onehot_prep(hipStream_t stream, const uint32_t* r, int rw, const OnehotLayout& lay, int nw, uint64_t count, uint32_t* R,
                                int32_t* rot) {
  const uint64_t items = (uint64_t)lay.M * count;
  hipLaunchKernelGGL(k_onehot_prep, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, r, rw, lay, nw, count, R, rot);
  return launched();
}
int sc_host::launch_onehot_split(hipStream_t stream, const uint32_t* p, int nw, const OnehotLayout& lay, uint64_t count, uint32_t* prod,
                                 uint32_t* bad) {
  hipLaunchKernelGGL(k_onehot_split, wave_rows((uint64_t)lay.m * lay.k * count), dim3(256), 0, stream, p, nw, lay, count, prod, bad);
  return launched();
}
int sc_host::launch_onehot_rotate(hipStream_t stream, const uint32_t* E, const int32_t* rot, int k, int m, int w2, uint64_t count,
                                  uint32_t* out) {
  hipLaunchKernelGGL(k_onehot_rotate, wave_rows((uint64_t)m * k * count), dim3(256), 0, stream, E, rot, k, m, w2, count, out);
  return launched();
}

// The plain-word kernels of the secure one-hot encoding (k_onehot_prep / k_onehot_split / k_onehot_rotate) and their plain launch
// functions (sc_internal.h) -- a unit of their own beside sc_launch_misc.hip, sc_launch_mul.hip and sc_launch_dot.hip.
#include "sc_internal.h"
#include "sc_plain_words.h"

namespace sc {

// ---------------------------------------------------------------------------------------------
// Secure one-hot encoding (sc_onehot_prep / sc_onehot_split / sc_onehot_rotate, include/sc_amd_dev.h).  A row has m
// indices; index q is blinded to the field d_q = i_q + r_q of f = ib + kappa + 1 bits and lives in message q div g at position
// q mod g, bits [(q mod g) f, (q mod g + 1) f).  Message mm holds n_mm = min(g, m - mm g) fields and ends at bit n_mm f.  The key holder
// marks j_q = d_q mod k among k plaintext rows, the initiator turns the k ciphertext rows back by rot_q = r_q mod k.
// ---------------------------------------------------------------------------------------------
// (OnehotLayout, ONEHOT_FIELD_WORDS: sc_vm.h)

// v mod k for 1 <= k <= 1024 over ALL the words of v, sixteen bits at a time from the top: the running remainder stays below 2^26
__device__ __forceinline__ uint32_t onehot_mod(const uint32_t (&v)[ONEHOT_FIELD_WORDS], uint32_t k) {
  uint32_t rem = 0;
#pragma unroll
  for (int w = ONEHOT_FIELD_WORDS - 1; w >= 0; w--) {
    rem = ((rem << 16) | (v[w] >> 16)) % k;
    rem = ((rem << 16) | (v[w] & 0xffffu)) % k;
  }
  return rem;
}

// The initiator's plaintext values of a one-hot from her draws r [m][count][rw] (< 2^(ib + kappa)): R [M][count][nw], the masks of a
// message at the bit offsets 0, f, 2f, .. (a mask has f - 1 bits: the top bit of a field is the carry of i + r), and
// rot [m][count] = r mod k.  One thread per message.
__global__ void k_onehot_prep(const uint32_t* __restrict__ r, int rw, OnehotLayout lay, int nw, uint64_t count, uint32_t* __restrict__ R,
                              int32_t* __restrict__ rot) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)lay.M * count) return;
  const int mm = (int)(i / count);
  const uint64_t b = i % count;
  const int n_m = lay.m - mm * lay.g < lay.g ? lay.m - mm * lay.g : lay.g;
  uint32_t* const row = R + i * nw;
  BitStream packed = {row, 0, 0};
  for (int j = 0; j < n_m; j++) {
    const uint64_t item = (uint64_t)(mm * lay.g + j) * count + b;
    uint32_t v[ONEHOT_FIELD_WORDS];
#pragma unroll
    for (int w = 0; w < ONEHOT_FIELD_WORDS; w++) v[w] = w < rw ? r[item * rw + w] : 0u;
    rot[item] = (int32_t)onehot_mod(v, (uint32_t)lay.k);
    stream_push(packed, v, lay.f);
  }
  stream_finish(packed, row + nw);                     // n_m f <= g f < bits(N) - 1 <= 32 nw: the fields end inside the row
}

// The key holder's half: from the decrypted P [M][count][nw], the plaintext rows prod [m][k][count][nw] with prod[q][t][b] =
// [t == d_q mod k] (word 0; the other words 0).  One wave per output row, its lanes across the row's words.  A message with a bit at or
// above its own end n_mm f sets *bad (the wave of its first field's row t = 0 looks); the rows are still written.
__global__ void k_onehot_split(const uint32_t* __restrict__ p, int nw, OnehotLayout lay, uint64_t count, uint32_t* __restrict__ prod,
                               uint32_t* __restrict__ bad) {
  const uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (uint64_t)lay.m * lay.k * count) return;
  const uint64_t b = row % count, qt = row / count;
  const int t = (int)(qt % lay.k), q = (int)(qt / lay.k);
  const int mm = q / lay.g, pos = q % lay.g;
  const uint32_t* x = p + ((uint64_t)mm * count + b) * nw;
  uint32_t d[ONEHOT_FIELD_WORDS];
#pragma unroll
  for (int w = 0; w < ONEHOT_FIELD_WORDS; w++) d[w] = field_word(x, nw, pos * lay.f, lay.f, w);
  const uint32_t hot = onehot_mod(d, (uint32_t)lay.k) == (uint32_t)t ? 1u : 0u;
  if (t == 0 && pos == 0) {
    const int n_m = lay.m - mm * lay.g < lay.g ? lay.m - mm * lay.g : lay.g;
    if (bits_from(x, nw, n_m * lay.f, lane, 64)) *bad = 1u;
  }
  uint32_t* o = prod + row * nw;
  for (int w = lane; w < nw; w += 64) o[w] = w == 0 ? hot : 0u;
}

// The initiator's last step: out[q][t][b] = E[q][(t + rot[q][b]) mod k][b], rows of w2 words, E and out [m][k][count][w2].  One wave per
// output row: the source row is wave-uniform, the lanes read and write consecutive words.  rot is reduced modulo k here, so no value of
// it reads outside E.
__global__ void k_onehot_rotate(const uint32_t* __restrict__ E, const int32_t* __restrict__ rot, int k, int m, int w2, uint64_t count,
                                uint32_t* __restrict__ out) {
  const uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (uint64_t)m * k * count) return;
  const uint64_t b = row % count, qt = row / count;
  const uint32_t t = (uint32_t)(qt % k);
  const uint64_t q = qt / k;
  const uint32_t s = (t + (uint32_t)rot[q * count + b] % (uint32_t)k) % (uint32_t)k;
  const uint32_t* src = E + ((q * k + s) * count + b) * w2;
  uint32_t* dst = out + row * w2;
  for (int w = lane; w < w2; w += 64) dst[w] = src[w];
}

}  // namespace sc

using namespace sc;

namespace {
// one wave per row, four waves per block
inline dim3 wave_rows(uint64_t rows) { return dim3((unsigned)((rows + 3) / 4)); }
}  // namespace

int sc_host::launch_onehot_prep(hipStream_t stream, const uint32_t* r, int rw, const OnehotLayout& lay, int nw, uint64_t count, uint32_t* R,
                                int32_t* rot) {
  hipLaunchKernelGGL(k_onehot_prep, blocks256((uint64_t)lay.M * count), dim3(256), 0, stream, r, rw, lay, nw, count, R, rot);
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

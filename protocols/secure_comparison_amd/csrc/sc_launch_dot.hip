// The plain-word kernels of the secure inner product (k_dot_prep / k_dot_split) and their plain launch functions (sc_internal.h) -- a
// unit of their own beside sc_launch_misc.hip and sc_launch_mul.hip.
#include "sc_internal.h"
#include "sc_plain_words.h"

namespace sc {

// ---------------------------------------------------------------------------------------------
// Secure inner product (sc_dot_prep / sc_dot_split, include/sc_amd_dev.h).  A row has k pairs (A_j, B_j), A_j = x_j + a_j
// of sa bits and B_j = y_j + b_j of sb bits, pb = sa + sb bits per pair (square mode: the one field A_j, pb = sa).  Pair j lives in
// message j mod M at position t = j div M: A in bits [t pb, t pb + sa), B in [t pb + sa, (t + 1) pb).  Message m holds the
// n_m = |{j < k : j mod M = m}| <= g pairs j = m, m + M, .. and ends at bit n_m pb.  One thread per row, one pass over the pairs with two
// field buffers and one accumulator, every one of them indexed by constants only so that they stay in registers.
// ---------------------------------------------------------------------------------------------
// (DotLayout, DOT_ACC_WORDS: sc_vm.h)

// acc += a * b: schoolbook by columns with a 96-bit column sum that also takes acc's own word, so the carry of the running sum
// travels through every word of acc, not only through the words of this one product
__device__ __forceinline__ void dot_mac(const uint32_t (&a)[MUL_FIELD_WORDS], const uint32_t (&b)[MUL_FIELD_WORDS], uint32_t (&acc)[DOT_ACC_WORDS]) {
  uint64_t col = 0;
  uint32_t top = 0;
#pragma unroll
  for (int k = 0; k < DOT_ACC_WORDS; k++) {
#pragma unroll
    for (int i = 0; i < MUL_FIELD_WORDS; i++) {
      if (k - i >= 0 && k - i < MUL_FIELD_WORDS) {
        const uint64_t p = (uint64_t)a[i] * b[k - i];
        col += p;
        top += col < p ? 1u : 0u;
      }
    }
    col += acc[k];
    top += col < acc[k] ? 1u : 0u;
    acc[k] = (uint32_t)col;
    col = (col >> 32) | ((uint64_t)top << 32);
    top = 0;
  }
}
// row[0 .. w) = acc, zero-extended (or cut: the fit rule keeps the sum below N, so the words past w are zero)
__device__ __forceinline__ void dot_store_acc(const uint32_t (&acc)[DOT_ACC_WORDS], uint32_t* row, int w) {
#pragma unroll
  for (int k = 0; k < DOT_ACC_WORDS; k++) if (k < w) row[k] = acc[k];
  for (int k = DOT_ACC_WORDS; k < w; k++) row[k] = 0u;
}

// The initiator's plaintext values of an inner product from her draws r_a [k][count][aw] (< 2^(wx + kappa)) and r_b [k][count][bw]
// (< 2^(wy + kappa)), every field with a mask of its own.  With a_j = r_a_j + ox, b_j = r_b_j + oy (ox = 2^(wx - 1), oy = 2^(wy - 1)
// for signed operands, else 0):
//   e [2k][count][ew]: planes 0 .. k-1 the exponents of x_j (b_j), planes k .. 2k-1 the exponents of y_j (a_j);
//   R [M][count][nw]: the packed masks of message m;  S [count][nw] = sum_j a_j b_j.
// Square mode (r_b unused): e [k][count][ew] = 2 a_j, R packs the a_j alone, S = sum_j a_j^2.
__global__ void k_dot_prep(const uint32_t* __restrict__ ra, int aw, const uint32_t* __restrict__ rb, int bw, DotLayout lay, int nw, int ew,
                           uint64_t count, uint32_t* __restrict__ e, uint32_t* __restrict__ R, uint32_t* __restrict__ S) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t a[MUL_FIELD_WORDS], b[MUL_FIELD_WORDS], acc[DOT_ACC_WORDS];
#pragma unroll
  for (int k = 0; k < DOT_ACC_WORDS; k++) acc[k] = 0u;
  const int oa = lay.is_signed ? lay.wx - 1 : -1, ob = lay.is_signed ? lay.wy - 1 : -1;
  for (int m = 0; m < lay.M; m++) {
    uint32_t* const row = R + ((uint64_t)m * count + i) * nw;
    BitStream packed = {row, 0, 0};
    for (int j = m; j < lay.k; j += lay.M) {
      const uint64_t item = (uint64_t)j * count + i;
      add_bit(ra + item * aw, aw, oa, a);
      stream_push(packed, a, lay.sa);
      if (lay.square) {
        uint32_t* ej = e + item * ew;                  // 2 a_j < 2^(sa + 1) <= 2^(32 MUL_FIELD_WORDS)
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) if (k < ew) ej[k] = (a[k] << 1) | (k ? a[k - 1] >> 31 : 0u);
        for (int k = MUL_FIELD_WORDS; k < ew; k++) ej[k] = 0u;
        dot_mac(a, a, acc);
      } else {
        add_bit(rb + item * bw, bw, ob, b);
        stream_push(packed, b, lay.sb);
        uint32_t* ex = e + item * ew;                  // the exponent of x_j is b_j
        uint32_t* ey = e + ((uint64_t)(lay.k + j) * count + i) * ew;
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) if (k < ew) { ex[k] = b[k]; ey[k] = a[k]; }
        for (int k = MUL_FIELD_WORDS; k < ew; k++) { ex[k] = 0u; ey[k] = 0u; }
        dot_mac(a, b, acc);
      }
    }
    stream_finish(packed, row + nw);                   // n_m pb <= g pb < bits(N) - 1 <= 32 nw: the fields end inside the row
  }
  dot_store_acc(acc, S + i * nw, nw);
}

// The key holder's half: from the decrypted P [M][count][nw], D [count][nw] = sum_j A_j B_j (square mode: sum_j A_j^2) over the fields of
// the row's M messages.  A message with a bit at or above its own end n_m pb sets *bad (the players disagree on the layout); D is still
// written.
__global__ void k_dot_split(const uint32_t* __restrict__ p, int nw, DotLayout lay, uint64_t count, uint32_t* __restrict__ D,
                            uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t a[MUL_FIELD_WORDS], b[MUL_FIELD_WORDS], acc[DOT_ACC_WORDS];
#pragma unroll
  for (int k = 0; k < DOT_ACC_WORDS; k++) acc[k] = 0u;
  uint32_t over = 0;
  for (int m = 0; m < lay.M; m++) {
    const uint32_t* x = p + ((uint64_t)m * count + i) * nw;
    const int n_m = (lay.k - m + lay.M - 1) / lay.M, end = n_m * lay.pb;      // the partial last position: end differs between messages
    over |= bits_from(x, nw, end, 0, 1);
    for (int t = 0; t < n_m; t++) {
#pragma unroll
      for (int k = 0; k < MUL_FIELD_WORDS; k++) a[k] = field_word(x, nw, t * lay.pb, lay.sa, k);
      if (lay.square) {
        dot_mac(a, a, acc);
      } else {
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) b[k] = field_word(x, nw, t * lay.pb + lay.sa, lay.sb, k);
        dot_mac(a, b, acc);
      }
    }
  }
  if (over) *bad = 1u;
  dot_store_acc(acc, D + i * nw, nw);
}

}  // namespace sc

using namespace sc;

int sc_host::launch_dot_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const DotLayout& lay, int nw, int ew,
                             uint64_t count, uint32_t* e, uint32_t* R, uint32_t* S) {
  hipLaunchKernelGGL(k_dot_prep, blocks256(count), dim3(256), 0, stream, ra, aw, rb, bw, lay, nw, ew, count, e, R, S);
  return launched();
}
int sc_host::launch_dot_split(hipStream_t stream, const uint32_t* p, int nw, const DotLayout& lay, uint64_t count, uint32_t* D, uint32_t* bad) {
  hipLaunchKernelGGL(k_dot_split, blocks256(count), dim3(256), 0, stream, p, nw, lay, count, D, bad);
  return launched();
}

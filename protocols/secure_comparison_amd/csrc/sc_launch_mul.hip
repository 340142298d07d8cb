// The plain-word kernels of the secure multiplication (k_mul_prep / k_mul_split) and their plain launch functions (sc_internal.h) -- a
// unit of their own beside sc_launch_misc.hip.
#include "sc_internal.h"
#include "sc_plain_words.h"

namespace sc {

// ---------------------------------------------------------------------------------------------
// Secure multiplication (sc_mul_prep / sc_mul_split, include/sc_amd_dev.h).  Layout of the packed plaintext of P, low
// bits first: A = x + e_y in bits [0, s), s = wx + kappa + 1, then field j = B_j = y_j + e_x_j in bits [off[j], off[j] + fbits[j]),
// fbits[j] = wy[j] + kappa + 1, off[0] = s, off[j + 1] = off[j] + fbits[j]; everything below the modulus (the host checks).  Every
// field may span several words (s and fbits reach 255 + 62 + 1 = 318 bits), so both kernels multiply multi-word by multi-word.
// ---------------------------------------------------------------------------------------------
// (MulLayout, MUL_FIELD_WORDS: sc_vm.h)

// The initiator's plaintext values of a multiplication from her draws r_a [count][aw] (< 2^(wx + kappa)) and r_b [nf][count][bw]
// (column j < 2^(wy[j] + kappa)), with ox = 2^(wx - 1), oy_j = 2^(wy[j] - 1) for signed operands and 0 otherwise:
//   e_y = r_a + ox and e_x_j = r_b_j + oy_j as e [nf + 1][count][ew] (planes e_x_0 .. e_x_(nf-1), then e_y),
//   R = e_y + sum_j 2^off[j] e_x_j ([count][nw]), rab_j = e_x_j e_y ([nf][count][nw]).
__global__ void k_mul_prep(const uint32_t* __restrict__ ra, int aw, const uint32_t* __restrict__ rb, int bw, MulLayout lay, int nw, int ew,
                           uint64_t count, uint32_t* __restrict__ R, uint32_t* __restrict__ e, uint32_t* __restrict__ rab) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t ey[MUL_FIELD_WORDS], ex[SEL_MAX_FIELDS][MUL_FIELD_WORDS];
  add_bit(ra + i * aw, aw, lay.is_signed ? lay.wx - 1 : -1, ey);
  uint32_t* eo = e + ((uint64_t)lay.nf * count + i) * ew;
  for (int k = 0; k < ew; k++) eo[k] = k < MUL_FIELD_WORDS ? ey[k] : 0u;
  for (int j = 0; j < lay.nf; j++) {
    add_bit(rb + ((uint64_t)j * count + i) * bw, bw, lay.is_signed ? lay.wy[j] - 1 : -1, ex[j]);
    uint32_t* ej = e + ((uint64_t)j * count + i) * ew;
    for (int k = 0; k < ew; k++) ej[k] = k < MUL_FIELD_WORDS ? ex[j][k] : 0u;
    mul_words(ex[j], MUL_FIELD_WORDS, ey, MUL_FIELD_WORDS, rab + ((uint64_t)j * count + i) * nw, nw);
  }
  for (int k = 0; k < nw; k++) {
    uint32_t v = k < MUL_FIELD_WORDS ? ey[k] : 0u;
    for (int j = 0; j < lay.nf; j++) v |= shl_word(ex[j], MUL_FIELD_WORDS, lay.off[j], k);
    R[i * nw + k] = v;
  }
}

// The key holder's half: from the decrypted P [count][nw], prod_j = A * B_j ([nf][count][nw]) with A and B_j the fields of P.
// A P with a bit at or above lay.end sets *bad (the players disagree on kappa or on the widths); its products are still written.
__global__ void k_mul_split(const uint32_t* __restrict__ p, int nw, MulLayout lay, uint64_t count, uint32_t* __restrict__ prod,
                            uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* x = p + i * nw;
  if (bits_from(x, nw, lay.end, 0, 1)) *bad = 1u;
  uint32_t a[MUL_FIELD_WORDS], b[MUL_FIELD_WORDS];
  for (int k = 0; k < MUL_FIELD_WORDS; k++) a[k] = field_word(x, nw, 0, lay.s, k);
  for (int j = 0; j < lay.nf; j++) {
    for (int k = 0; k < MUL_FIELD_WORDS; k++) b[k] = field_word(x, nw, lay.off[j], lay.fbits[j], k);
    mul_words(a, MUL_FIELD_WORDS, b, MUL_FIELD_WORDS, prod + ((uint64_t)j * count + i) * nw, nw);
  }
}

}  // namespace sc

using namespace sc;

int sc_host::launch_mul_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const MulLayout& lay, int nw, int ew,
                             uint64_t count, uint32_t* R, uint32_t* e, uint32_t* rab) {
  hipLaunchKernelGGL(k_mul_prep, blocks256(count), dim3(256), 0, stream, ra, aw, rb, bw, lay, nw, ew, count, R, e, rab);
  return launched();
}
int sc_host::launch_mul_split(hipStream_t stream, const uint32_t* p, int nw, const MulLayout& lay, uint64_t count, uint32_t* prod, uint32_t* bad) {
  hipLaunchKernelGGL(k_mul_split, blocks256(count), dim3(256), 0, stream, p, nw, lay, count, prod, bad);
  return launched();
}

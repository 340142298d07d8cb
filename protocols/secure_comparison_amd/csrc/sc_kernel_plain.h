// Plain-word helper kernels of the protocol steps (gfx950): the comparison's two and the secure selection's two, compiled and launched
// by sc_launch_misc.hip.  The kernels of the multiplication, the inner product and the one-hot encoding stand in the units that launch
// them (sc_launch_mul.hip, sc_launch_dot.hip, sc_launch_lookup.hip); the bit-field helpers all of them share are sc_plain_words.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sc_plain_words.h"
#include "sc_vm.h"

namespace sc {

// ---------------------------------------------------------------------------------------------
// Plain-integer helper kernels on canonical 32-bit words (HBM-bound, one thread per item).
// ---------------------------------------------------------------------------------------------
// 64-bit word j of a number held as nw little-endian 32-bit words (0 past its end)
__device__ __forceinline__ uint64_t word64(const uint32_t* x, int nw, int j) {
  const int k = 2 * j;
  return (k < nw ? (uint64_t)x[k] : 0ull) | ((k + 1 < nw) ? ((uint64_t)x[k + 1] << 32) : 0ull);
}

// Flag rows (include/sc_amd.h): alpha, alpha_tilde and beta are LW = ceil(l / 64) little-endian u64 words per item, [count][LW];
// LW = 1 is the [count] array of l <= 64.  The launch picks the instance from l, so 64 (LW - 1) < l <= 64 LW.

// Alice's plaintext-side values derived from r (SC/initiator.py:250-256, :270, :289, :373, :558-562):
//   m1 = 2^l + r (as nw+1 words), alpha = r mod 2^l, alpha_tilde = (r - N) mod 2^l (the borrow carried across the flag words),
//   rsmall = [r < (N-1)/2], rshift = r >> l.
template <int LW>
__global__ void k_plain_alice(const uint32_t* __restrict__ r, const uint32_t* __restrict__ nmod,
                              const uint32_t* __restrict__ halfn /* (N-1)/2 */, int nw, int l, uint64_t count,
                              uint32_t* __restrict__ m1, uint64_t* __restrict__ alpha,
                              uint64_t* __restrict__ alpha_tilde, uint64_t* __restrict__ rsmall,
                              uint32_t* __restrict__ rshift) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* ri = r + i * nw;
  const int top = l - 64 * (LW - 1);   // bits of the top flag word, 1 .. 64
  const uint64_t tmask = (top >= 64) ? ~0ull : ((1ull << top) - 1);
  uint64_t borrow = 0;
#pragma unroll
  for (int j = 0; j < LW; j++) {
    const uint64_t rw = word64(ri, nw, j), nwd = word64(nmod, nw, j);
    const uint64_t mask = (j == LW - 1) ? tmask : ~0ull;
    const uint64_t diff = rw - nwd - borrow;
    borrow = (rw < nwd || rw - nwd < borrow) ? 1ull : 0ull;
    alpha[i * LW + j] = rw & mask;
    alpha_tilde[i * LW + j] = diff & mask;
  }
  int cmp = 0;  // r ? halfn
  for (int k = nw - 1; k >= 0 && cmp == 0; k--) cmp = (ri[k] > halfn[k]) ? 1 : ((ri[k] < halfn[k]) ? -1 : 0);
  rsmall[i] = (cmp < 0) ? 1ull : 0ull;
  // m1 = r + 2^l  (nw + 1 words)
  uint64_t carry = 0;
  for (int k = 0; k <= nw; k++) {
    uint64_t v = (k < nw ? (uint64_t)ri[k] : 0ull) + carry + ((k == (l >> 5)) ? (1ull << (l & 31)) : 0ull);
    m1[i * (nw + 1) + k] = (uint32_t)v;
    carry = v >> 32;
  }
  // rshift = r >> l
  const int ws = l >> 5, bs = l & 31;
  for (int k = 0; k < nw; k++) {
    const uint64_t lo = (k + ws < nw) ? ri[k + ws] : 0u, hi = (k + ws + 1 < nw) ? ri[k + ws + 1] : 0u;
    rshift[i * nw + k] = (uint32_t)(((hi << 32) | lo) >> bs);
  }
}

// Bob's plaintext-side values derived from z (SC/keyholder.py:196, :213, :274-282):
//   beta = z mod 2^l (LW words), dbit = [z < (N-1)/2], zeta1 = z >> l, zeta2 = (z + N) >> l if dbit else z >> l.
//   bits (nullable): the plaintext bits of steps 4a / 4b as bytes, bit-major [l+1][count]: plane 0 = d, plane 1 + i = bit i of beta
//   (SC/keyholder.py:213, 230-233) -- what the g^bit selection of the DGK encryption launch reads.
template <int LW>
__global__ void k_plain_bob(const uint32_t* __restrict__ z, const uint32_t* __restrict__ nmod,
                            const uint32_t* __restrict__ halfn, int nw, int l, uint64_t count,
                            uint64_t* __restrict__ beta, uint64_t* __restrict__ dbit, uint32_t* __restrict__ zeta1,
                            uint32_t* __restrict__ zeta2, uint8_t* __restrict__ bits) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* zi = z + i * nw;
  const int tb = l - 64 * (LW - 1);   // bits of the top flag word, 1 .. 64
  const uint64_t tmask = (tb >= 64) ? ~0ull : ((1ull << tb) - 1);
  uint64_t bw[LW];
#pragma unroll
  for (int j = 0; j < LW; j++) {
    bw[j] = word64(zi, nw, j) & ((j == LW - 1) ? tmask : ~0ull);
    beta[i * LW + j] = bw[j];
  }
  int cmp = 0;
  for (int k = nw - 1; k >= 0 && cmp == 0; k--) cmp = (zi[k] > halfn[k]) ? 1 : ((zi[k] < halfn[k]) ? -1 : 0);
  const bool d = cmp < 0;
  dbit[i] = d ? 1ull : 0ull;
  if (bits) {
    bits[i] = d ? 1 : 0;
#pragma unroll
    for (int j = 0; j < LW; j++) {
      const int nb = (j == LW - 1) ? tb : 64;
      for (int k = 0; k < nb; k++) bits[(uint64_t)(64 * j + k + 1) * count + i] = (uint8_t)((bw[j] >> k) & 1);
    }
  }
  const int ws = l >> 5, bs = l & 31;
  // zeta2: first the sum z + (d ? N : 0) (nw words + a carry word), then an in-place
  // ascending funnel shift (word o only reads words >= o).
  uint32_t* z2 = zeta2 + i * nw;
  uint64_t carry = 0;
  for (int k = 0; k < nw; k++) {
    const uint64_t v = (uint64_t)zi[k] + (d ? nmod[k] : 0u) + carry;
    z2[k] = (uint32_t)v;
    carry = v >> 32;
  }
  const uint32_t top = (uint32_t)carry;  // word nw of the sum (z + N may exceed nw words)
  for (int k = 0; k < nw; k++) {
    const int a = k + ws, b = k + ws + 1;
    const uint64_t lo = (a < nw) ? z2[a] : ((a == nw) ? top : 0u), hi = (b < nw) ? z2[b] : ((b == nw) ? top : 0u);
    z2[k] = (uint32_t)(((hi << 32) | lo) >> bs);
  }
  for (int k = 0; k < nw; k++) {
    const uint64_t lo = (k + ws < nw) ? zi[k + ws] : 0u, hi = (k + ws + 1 < nw) ? zi[k + ws + 1] : 0u;
    zeta1[i * nw + k] = (uint32_t)(((hi << 32) | lo) >> bs);
  }
}


// ---------------------------------------------------------------------------------------------
// Secure selection (sc_select_prep / sc_select_split, include/sc_amd_dev.h).  Layout of the packed plaintext of P, low bits first:
// the field a = delta + r_a in bits [0, s), s = kappa + 1, then field j = d_j + r_b_j in bits [off[j], off[j] + fbits[j]),
// fbits[j] = width[j] + kappa + 2, off[0] = s, off[j + 1] = off[j] + fbits[j]; everything below the modulus (the host checks).
// ---------------------------------------------------------------------------------------------
// (SelLayout: sc_vm.h)

// The initiator's plaintext values of a selection from her draws r_a [count][aw] (< 2^kappa) and r_b [nf][count][bw]:
//   R = r_a + sum_j 2^off[j] r_b_j ([count][nw]), e_j = r_b_j + 2^width[j] ([nf][count][ew]), rab_j = r_a r_b_j ([nf][count][nw]).
__global__ void k_select_prep(const uint32_t* __restrict__ ra, int aw, const uint32_t* __restrict__ rb, int bw, SelLayout lay, int nw,
                              int ew, uint64_t count, uint32_t* __restrict__ R, uint32_t* __restrict__ e, uint32_t* __restrict__ rab) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* a = ra + i * aw;
  const uint64_t av = (uint64_t)a[0] | (aw > 1 ? (uint64_t)a[1] << 32 : 0u);
  for (int k = 0; k < nw; k++) {
    uint32_t v = k < aw ? a[k] : 0u;
    for (int j = 0; j < lay.nf; j++) v |= shl_word(rb + ((uint64_t)j * count + i) * bw, bw, lay.off[j], k);
    R[i * nw + k] = v;
  }
  for (int j = 0; j < lay.nf; j++) {
    const uint32_t* b = rb + ((uint64_t)j * count + i) * bw;
    uint32_t* ej = e + ((uint64_t)j * count + i) * ew;
    uint32_t carry = 0;
    for (int k = 0; k < ew; k++) {
      const uint64_t t = (uint64_t)(k < bw ? b[k] : 0u) + carry + ((k == (lay.width[j] >> 5)) ? (1u << (lay.width[j] & 31)) : 0u);
      ej[k] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    mul64_words(av, [=](int k) { return k < bw ? b[k] : 0u; }, rab + ((uint64_t)j * count + i) * nw, nw);
  }
}

// The key holder's half: from the decrypted P [count][nw], prod_j = a * b_j ([nf][count][nw]) with a and b_j the fields of P.
// A P with a bit at or above lay.end sets *bad (the players disagree on kappa or on the widths); its products are still written.
__global__ void k_select_split(const uint32_t* __restrict__ p, int nw, SelLayout lay, uint64_t count, uint32_t* __restrict__ prod,
                               uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* x = p + i * nw;
  const uint64_t a = (uint64_t)field_word(x, nw, 0, lay.s, 0) | ((uint64_t)field_word(x, nw, 0, lay.s, 1) << 32);
  if (bits_from(x, nw, lay.end, 0, 1)) *bad = 1u;
  for (int j = 0; j < lay.nf; j++) {         // the field goes into the product word by word: it may be wider than any buffer
    const int off = lay.off[j], fbits = lay.fbits[j];
    mul64_words(a, [=](int k) { return field_word(x, nw, off, fbits, k); }, prod + ((uint64_t)j * count + i) * nw, nw);
  }
}

}  // namespace sc

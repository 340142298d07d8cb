// Plain-word helper kernels of the protocol steps (gfx950).  Included by sc_launch_misc.hip and, for the multiplication's two, by
// sc_launch_mul.hip; for the inner product's two, by sc_launch_dot.hip; for the one-hot's three, by sc_launch_lookup.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// word k of (x >> bitpos) masked to `bits` bits; x has nw words (0 past its end)
__device__ __forceinline__ uint32_t sel_field_word(const uint32_t* x, int nw, int bitpos, int bits, int k) {
  const int b = bitpos + 32 * k, q = b >> 5, sh = b & 31;
  if (32 * k >= bits) return 0u;
  uint32_t v = (q < nw) ? (x[q] >> sh) : 0u;
  if (sh && q + 1 < nw) v |= x[q + 1] << (32 - sh);
  const int left = bits - 32 * k;
  return left >= 32 ? v : (v & ((1u << left) - 1u));
}
// word k of (x << bitpos); x has xw words
__device__ __forceinline__ uint32_t sel_shl_word(const uint32_t* x, int xw, int bitpos, int k) {
  const int q = k - (bitpos >> 5), sh = bitpos & 31;
  uint32_t v = (q >= 0 && q < xw) ? (x[q] << sh) : 0u;
  if (sh && q - 1 >= 0 && q - 1 < xw) v |= x[q - 1] >> (32 - sh);
  return v;
}
// out[0 .. nw) = a * b mod 2^(32 nw), a < 2^64, b of bw words
__device__ __forceinline__ void sel_mul64(uint64_t a, const uint32_t* b, int bw, uint32_t* out, int nw) {
  const uint64_t alo = a & 0xffffffffu, ahi = a >> 32;
  uint64_t carry = 0;
  for (int k = 0; k < nw; k++) {
    const uint64_t p1 = (k < bw) ? (uint64_t)b[k] * alo : 0u;
    const uint64_t p2 = (k >= 1 && k - 1 < bw) ? (uint64_t)b[k - 1] * ahi : 0u;
    const uint64_t lo = (p1 & 0xffffffffu) + (p2 & 0xffffffffu) + (carry & 0xffffffffu);
    carry = (p1 >> 32) + (p2 >> 32) + (carry >> 32) + (lo >> 32);
    out[k] = (uint32_t)lo;
  }
}

#if !defined(SC_MUL_UNIT) && !defined(SC_DOT_UNIT) && !defined(SC_LOOKUP_UNIT)   // the other units take the helpers above and their own kernels below, not these two
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
    for (int j = 0; j < lay.nf; j++) v |= sel_shl_word(rb + ((uint64_t)j * count + i) * bw, bw, lay.off[j], k);
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
    sel_mul64(av, b, bw, rab + ((uint64_t)j * count + i) * nw, nw);
  }
}

// The key holder's half: from the decrypted P [count][nw], prod_j = a * b_j ([nf][count][nw]) with a and b_j the fields of P.
// A P with a bit at or above lay.end sets *bad (the players disagree on kappa or on the widths); its products are still written.
__global__ void k_select_split(const uint32_t* __restrict__ p, int nw, SelLayout lay, uint64_t count, uint32_t* __restrict__ prod,
                               uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t* x = p + i * nw;
  const uint64_t a = (uint64_t)sel_field_word(x, nw, 0, lay.s, 0) | ((uint64_t)sel_field_word(x, nw, 0, lay.s, 1) << 32);
  uint32_t over = 0;
  for (int k = lay.end >> 5; k < nw; k++) over |= (k == (lay.end >> 5)) ? (x[k] >> (lay.end & 31)) : x[k];
  if (over) *bad = 1u;
  for (int j = 0; j < lay.nf; j++) {
    uint32_t* o = prod + ((uint64_t)j * count + i) * nw;
    const int fw = (lay.fbits[j] + 31) >> 5;
    uint64_t carry = 0;
    const uint64_t alo = a & 0xffffffffu, ahi = a >> 32;
    uint32_t prev = 0;
    for (int k = 0; k < nw; k++) {          // sel_mul64 with b = the field, extracted on the fly
      const uint32_t bk = k < fw ? sel_field_word(x, nw, lay.off[j], lay.fbits[j], k) : 0u;
      const uint64_t p1 = (uint64_t)bk * alo, p2 = (uint64_t)prev * ahi;
      const uint64_t lo = (p1 & 0xffffffffu) + (p2 & 0xffffffffu) + (carry & 0xffffffffu);
      carry = (p1 >> 32) + (p2 >> 32) + (carry >> 32) + (lo >> 32);
      o[k] = (uint32_t)lo;
      prev = bk;
    }
  }
}

#endif  // !SC_MUL_UNIT && !SC_DOT_UNIT && !SC_LOOKUP_UNIT

// ---------------------------------------------------------------------------------------------
// Secure multiplication (sc_mul_prep / sc_mul_split, include/sc_amd_dev.h).  Layout of the packed plaintext of P, low
// bits first: A = x + e_y in bits [0, s), s = wx + kappa + 1, then field j = B_j = y_j + e_x_j in bits [off[j], off[j] + fbits[j]),
// fbits[j] = wy[j] + kappa + 1, off[0] = s, off[j + 1] = off[j] + fbits[j]; everything below the modulus (the host checks).  Every
// field may span several words (s and fbits reach 255 + 62 + 1 = 318 bits), so both kernels multiply multi-word by multi-word.
// ---------------------------------------------------------------------------------------------
// (MulLayout, MUL_FIELD_WORDS: sc_vm.h)  Compiled and launched by sc_launch_mul.hip alone (SC_MUL_UNIT).
#ifdef SC_MUL_UNIT

// out[0 .. nw) = a * b mod 2^(32 nw), a of aw words, b of bw words: schoolbook by columns, a 96-bit accumulator per column
__device__ __forceinline__ void mul_words(const uint32_t* a, int aw, const uint32_t* b, int bw, uint32_t* out, int nw) {
  uint64_t acc = 0;
  uint32_t top = 0;
  for (int k = 0; k < nw; k++) {
    const int lo = k - bw + 1 > 0 ? k - bw + 1 : 0, hi = k < aw - 1 ? k : aw - 1;
    for (int i = lo; i <= hi; i++) {
      const uint64_t p = (uint64_t)a[i] * b[k - i];
      acc += p;
      top += acc < p ? 1u : 0u;
    }
    out[k] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)top << 32);
    top = 0;
  }
}
// v[0 .. MUL_FIELD_WORDS) = x (xw words, 0 past its end) + 2^(bit) when bit >= 0
__device__ __forceinline__ void mul_add_offset(const uint32_t* x, int xw, int bit, uint32_t* v) {
  uint32_t carry = 0;
  for (int k = 0; k < MUL_FIELD_WORDS; k++) {
    const uint64_t t = (uint64_t)(k < xw ? x[k] : 0u) + carry + ((bit >= 0 && k == (bit >> 5)) ? (1u << (bit & 31)) : 0u);
    v[k] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}

// The initiator's plaintext values of a multiplication from her draws r_a [count][aw] (< 2^(wx + kappa)) and r_b [nf][count][bw]
// (column j < 2^(wy[j] + kappa)), with ox = 2^(wx - 1), oy_j = 2^(wy[j] - 1) for signed operands and 0 otherwise:
//   e_y = r_a + ox and e_x_j = r_b_j + oy_j as e [nf + 1][count][ew] (planes e_x_0 .. e_x_(nf-1), then e_y),
//   R = e_y + sum_j 2^off[j] e_x_j ([count][nw]), rab_j = e_x_j e_y ([nf][count][nw]).
__global__ void k_mul_prep(const uint32_t* __restrict__ ra, int aw, const uint32_t* __restrict__ rb, int bw, MulLayout lay, int nw, int ew,
                           uint64_t count, uint32_t* __restrict__ R, uint32_t* __restrict__ e, uint32_t* __restrict__ rab) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t ey[MUL_FIELD_WORDS], ex[SEL_MAX_FIELDS][MUL_FIELD_WORDS];
  mul_add_offset(ra + i * aw, aw, lay.is_signed ? lay.wx - 1 : -1, ey);
  uint32_t* eo = e + ((uint64_t)lay.nf * count + i) * ew;
  for (int k = 0; k < ew; k++) eo[k] = k < MUL_FIELD_WORDS ? ey[k] : 0u;
  for (int j = 0; j < lay.nf; j++) {
    mul_add_offset(rb + ((uint64_t)j * count + i) * bw, bw, lay.is_signed ? lay.wy[j] - 1 : -1, ex[j]);
    uint32_t* ej = e + ((uint64_t)j * count + i) * ew;
    for (int k = 0; k < ew; k++) ej[k] = k < MUL_FIELD_WORDS ? ex[j][k] : 0u;
    mul_words(ex[j], MUL_FIELD_WORDS, ey, MUL_FIELD_WORDS, rab + ((uint64_t)j * count + i) * nw, nw);
  }
  for (int k = 0; k < nw; k++) {
    uint32_t v = k < MUL_FIELD_WORDS ? ey[k] : 0u;
    for (int j = 0; j < lay.nf; j++) v |= sel_shl_word(ex[j], MUL_FIELD_WORDS, lay.off[j], k);
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
  uint32_t over = 0;
  for (int k = lay.end >> 5; k < nw; k++) over |= (k == (lay.end >> 5)) ? (x[k] >> (lay.end & 31)) : x[k];
  if (over) *bad = 1u;
  uint32_t a[MUL_FIELD_WORDS], b[MUL_FIELD_WORDS];
  for (int k = 0; k < MUL_FIELD_WORDS; k++) a[k] = sel_field_word(x, nw, 0, lay.s, k);
  for (int j = 0; j < lay.nf; j++) {
    for (int k = 0; k < MUL_FIELD_WORDS; k++) b[k] = sel_field_word(x, nw, lay.off[j], lay.fbits[j], k);
    mul_words(a, MUL_FIELD_WORDS, b, MUL_FIELD_WORDS, prod + ((uint64_t)j * count + i) * nw, nw);
  }
}
#endif  // SC_MUL_UNIT

// ---------------------------------------------------------------------------------------------
// Secure inner product (sc_dot_prep / sc_dot_split, include/sc_amd_dev.h).  A row has k pairs (A_j, B_j), A_j = x_j + a_j
// of sa bits and B_j = y_j + b_j of sb bits, pb = sa + sb bits per pair (square mode: the one field A_j, pb = sa).  Pair j lives in
// message j mod M at position t = j div M: A in bits [t pb, t pb + sa), B in [t pb + sa, (t + 1) pb).  Message m holds the
// n_m = |{j < k : j mod M = m}| <= g pairs j = m, m + M, .. and ends at bit n_m pb.  One thread per row, one pass over the pairs with two
// field buffers and one accumulator, every one of them indexed by constants only so that they stay in registers.
// ---------------------------------------------------------------------------------------------
// (DotLayout, DOT_ACC_WORDS: sc_vm.h)  Compiled and launched by sc_launch_dot.hip alone (SC_DOT_UNIT).
#ifdef SC_DOT_UNIT

// v = x (xw words, 0 past its end) + 2^bit when bit >= 0
__device__ __forceinline__ void dot_load_field(const uint32_t* x, int xw, int bit, uint32_t (&v)[MUL_FIELD_WORDS]) {
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < MUL_FIELD_WORDS; k++) {
    const uint64_t t = (uint64_t)(k < xw ? x[k] : 0u) + carry + ((bit >= 0 && k == (bit >> 5)) ? (1u << (bit & 31)) : 0u);
    v[k] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}
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
// the low `bits` bits of v appended to a little-endian bit stream: buf holds `fill` < 32 pending bits, whole words go to *out.  v has no
// bit at or above `bits` (the draws' widths); the number of words written depends on the widths alone, never on the values
__device__ __forceinline__ void dot_push(const uint32_t (&v)[MUL_FIELD_WORDS], int bits, uint64_t& buf, int& fill, uint32_t*& out) {
#pragma unroll
  for (int w = 0; w < MUL_FIELD_WORDS; w++) {
    const int nb = bits - 32 * w;
    if (nb > 0) {
      buf |= (uint64_t)v[w] << fill;
      fill += nb < 32 ? nb : 32;
      if (fill >= 32) { *out++ = (uint32_t)buf; buf >>= 32; fill -= 32; }
    }
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
    uint32_t* out = row;
    uint64_t buf = 0;
    int fill = 0;
    for (int j = m; j < lay.k; j += lay.M) {
      const uint64_t item = (uint64_t)j * count + i;
      dot_load_field(ra + item * aw, aw, oa, a);
      dot_push(a, lay.sa, buf, fill, out);
      if (lay.square) {
        uint32_t* ej = e + item * ew;                  // 2 a_j < 2^(sa + 1) <= 2^(32 MUL_FIELD_WORDS)
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) if (k < ew) ej[k] = (a[k] << 1) | (k ? a[k - 1] >> 31 : 0u);
        for (int k = MUL_FIELD_WORDS; k < ew; k++) ej[k] = 0u;
        dot_mac(a, a, acc);
      } else {
        dot_load_field(rb + item * bw, bw, ob, b);
        dot_push(b, lay.sb, buf, fill, out);
        uint32_t* ex = e + item * ew;                  // the exponent of x_j is b_j
        uint32_t* ey = e + ((uint64_t)(lay.k + j) * count + i) * ew;
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) if (k < ew) { ex[k] = b[k]; ey[k] = a[k]; }
        for (int k = MUL_FIELD_WORDS; k < ew; k++) { ex[k] = 0u; ey[k] = 0u; }
        dot_mac(a, b, acc);
      }
    }
    if (fill) *out++ = (uint32_t)buf;
    while (out < row + nw) *out++ = 0u;                // n_m pb <= g pb < bits(N) - 1 <= 32 nw: the fields end inside the row
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
    for (int k = end >> 5; k < nw; k++) over |= (k == (end >> 5)) ? (x[k] >> (end & 31)) : x[k];
    for (int t = 0; t < n_m; t++) {
#pragma unroll
      for (int k = 0; k < MUL_FIELD_WORDS; k++) a[k] = sel_field_word(x, nw, t * lay.pb, lay.sa, k);
      if (lay.square) {
        dot_mac(a, a, acc);
      } else {
#pragma unroll
        for (int k = 0; k < MUL_FIELD_WORDS; k++) b[k] = sel_field_word(x, nw, t * lay.pb + lay.sa, lay.sb, k);
        dot_mac(a, b, acc);
      }
    }
  }
  if (over) *bad = 1u;
  dot_store_acc(acc, D + i * nw, nw);
}
#endif  // SC_DOT_UNIT

// ---------------------------------------------------------------------------------------------
// Secure one-hot encoding (sc_onehot_prep / sc_onehot_split / sc_onehot_rotate, include/sc_amd_dev.h).  A row has m
// indices; index q is blinded to the field d_q = i_q + r_q of f = ib + kappa + 1 bits and lives in message q div g at position
// q mod g, bits [(q mod g) f, (q mod g + 1) f).  Message mm holds n_mm = min(g, m - mm g) fields and ends at bit n_mm f.  The key holder
// marks j_q = d_q mod k among k plaintext rows, the initiator turns the k ciphertext rows back by rot_q = r_q mod k.
// ---------------------------------------------------------------------------------------------
// (OnehotLayout, ONEHOT_FIELD_WORDS: sc_vm.h)  Compiled and launched by sc_launch_lookup.hip alone (SC_LOOKUP_UNIT).
#ifdef SC_LOOKUP_UNIT

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
  uint32_t* out = row;
  uint64_t buf = 0;
  int fill = 0;
  for (int j = 0; j < n_m; j++) {
    const uint64_t item = (uint64_t)(mm * lay.g + j) * count + b;
    uint32_t v[ONEHOT_FIELD_WORDS];
#pragma unroll
    for (int w = 0; w < ONEHOT_FIELD_WORDS; w++) v[w] = w < rw ? r[item * rw + w] : 0u;
    rot[item] = (int32_t)onehot_mod(v, (uint32_t)lay.k);
#pragma unroll
    for (int w = 0; w < ONEHOT_FIELD_WORDS; w++) {     // append the f bits of the field to the row's bit stream (fill < 32 pending bits)
      const int nb = lay.f - 32 * w;
      if (nb > 0) {
        buf |= (uint64_t)v[w] << fill;
        fill += nb < 32 ? nb : 32;
        if (fill >= 32) { *out++ = (uint32_t)buf; buf >>= 32; fill -= 32; }
      }
    }
  }
  if (fill) *out++ = (uint32_t)buf;
  while (out < row + nw) *out++ = 0u;                  // n_m f <= g f < bits(N) - 1 <= 32 nw: the fields end inside the row
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
  for (int w = 0; w < ONEHOT_FIELD_WORDS; w++) d[w] = sel_field_word(x, nw, pos * lay.f, lay.f, w);
  const uint32_t hot = onehot_mod(d, (uint32_t)lay.k) == (uint32_t)t ? 1u : 0u;
  if (t == 0 && pos == 0) {
    const int n_m = lay.m - mm * lay.g < lay.g ? lay.m - mm * lay.g : lay.g, end = n_m * lay.f;
    uint32_t over = 0;
    for (int w = (end >> 5) + lane; w < nw; w += 64) over |= (w == (end >> 5)) ? (x[w] >> (end & 31)) : x[w];
    if (over) *bad = 1u;
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
#endif  // SC_LOOKUP_UNIT

}  // namespace sc

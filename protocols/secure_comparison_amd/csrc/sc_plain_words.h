// Bit-field and multi-word helpers of the plain-word kernels (sc_kernel_plain.h, sc_launch_mul.hip, sc_launch_dot.hip,
// sc_launch_lookup.hip), each stated once.  Numbers are little-endian arrays of 32-bit words.  Plain C++: the header compiles without
// the GPU runtime, which is how tests/test_plain_words_cpu.py asks it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SC_WORDS_FN __host__ __device__ __forceinline__
#define SC_WORDS_UNROLL _Pragma("unroll")   // a fixed-size array stays in registers only where every index into it is a constant
#else
#define SC_WORDS_FN inline
#define SC_WORDS_UNROLL
#endif

namespace sc {

// word k of (x >> bitpos) masked to `bits` bits; x has nw words (0 past its end)
SC_WORDS_FN uint32_t field_word(const uint32_t* x, int nw, int bitpos, int bits, int k) {
  const int b = bitpos + 32 * k, q = b >> 5, sh = b & 31;
  if (32 * k >= bits) return 0u;
  uint32_t v = (q < nw) ? (x[q] >> sh) : 0u;
  if (sh && q + 1 < nw) v |= x[q + 1] << (32 - sh);
  const int left = bits - 32 * k;
  return left >= 32 ? v : (v & ((1u << left) - 1u));
}
// word k of (x << bitpos); x has xw words
SC_WORDS_FN uint32_t shl_word(const uint32_t* x, int xw, int bitpos, int k) {
  const int q = k - (bitpos >> 5), sh = bitpos & 31;
  uint32_t v = (q >= 0 && q < xw) ? (x[q] << sh) : 0u;
  if (sh && q - 1 >= 0 && q - 1 < xw) v |= x[q - 1] >> (32 - sh);
  return v;
}

// v = x (xw words, 0 past its end) + 2^bit when bit >= 0, cut to the N words of v
template <int N>
SC_WORDS_FN void add_bit(const uint32_t* x, int xw, int bit, uint32_t (&v)[N]) {
  uint32_t carry = 0;
  SC_WORDS_UNROLL
  for (int k = 0; k < N; k++) {
    const uint64_t t = (uint64_t)(k < xw ? x[k] : 0u) + carry + ((bit >= 0 && k == (bit >> 5)) ? (1u << (bit & 31)) : 0u);
    v[k] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}

// A little-endian bit stream written into a row of words: buf holds `fill` < 32 pending bits, whole words go to *out.
struct BitStream {
  uint32_t* out;
  uint64_t buf;
  int fill;
};
// the low `bits` bits of v appended to the stream.  v has no bit at or above `bits`; the number of words written depends on the widths
// alone, never on the values
template <int N>
SC_WORDS_FN void stream_push(BitStream& s, const uint32_t (&v)[N], int bits) {
  SC_WORDS_UNROLL
  for (int w = 0; w < N; w++) {
    const int nb = bits - 32 * w;
    if (nb > 0) {
      s.buf |= (uint64_t)v[w] << s.fill;
      s.fill += nb < 32 ? nb : 32;
      if (s.fill >= 32) { *s.out++ = (uint32_t)s.buf; s.buf >>= 32; s.fill -= 32; }
    }
  }
}
// the pending bits flushed and the rest of the row, up to `end`, filled with zeros (the caller's fields end inside the row)
SC_WORDS_FN void stream_finish(BitStream& s, uint32_t* end) {
  if (s.fill) *s.out++ = (uint32_t)s.buf;
  while (s.out < end) *s.out++ = 0u;
}

// Nonzero iff one of the words w, w + step, .. of x (nw words), w = (end >> 5) + first, has a bit at or above bit `end` of x: a thread
// that looks alone asks with (first, step) = (0, 1), the lanes of a wave that share the look with (lane, 64)
SC_WORDS_FN uint32_t bits_from(const uint32_t* x, int nw, int end, int first, int step) {
  uint32_t over = 0;
  for (int k = (end >> 5) + first; k < nw; k += step) over |= (k == (end >> 5)) ? (x[k] >> (end & 31)) : x[k];
  return over;
}

// out[0 .. nw) = a * b mod 2^(32 nw), a of aw words, b of bw words: schoolbook by columns, a 96-bit accumulator per column
SC_WORDS_FN void mul_words(const uint32_t* a, int aw, const uint32_t* b, int bw, uint32_t* out, int nw) {
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
// out[0 .. nw) = a * b mod 2^(32 nw), a < 2^64, b the number whose word k is word(k): asked once per k, in ascending order, so b need
// not be held anywhere
template <typename Word>
SC_WORDS_FN void mul64_words(uint64_t a, Word word, uint32_t* out, int nw) {
  const uint64_t alo = a & 0xffffffffu, ahi = a >> 32;
  uint64_t carry = 0;
  uint32_t prev = 0;
  for (int k = 0; k < nw; k++) {
    const uint32_t bk = word(k);
    const uint64_t p1 = (uint64_t)bk * alo, p2 = (uint64_t)prev * ahi;
    const uint64_t lo = (p1 & 0xffffffffu) + (p2 & 0xffffffffu) + (carry & 0xffffffffu);
    carry = (p1 >> 32) + (p2 >> 32) + (carry >> 32) + (lo >> 32);
    out[k] = (uint32_t)lo;
    prev = bk;
  }
}

}  // namespace sc

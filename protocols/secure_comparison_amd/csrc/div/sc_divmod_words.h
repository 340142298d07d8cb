// The digit loop of k_divmod_words (sc_kernel_divmod.h): a number of nw little-endian 32-bit words divided by a 64-bit divisor, floor
// quotient and remainder.  Plain C++: the header compiles without the GPU runtime, which is how tests/test_division_cpu.py asks it, so
// the CPU tier runs the very code the kernel runs.
//
// Knuth's algorithm D (TAOCP 4.3.1) with 32-bit digits and a TWO-digit divisor, for every divisor: d is shifted left by its leading
// zeros s = clz64(d), 0 .. 63, so v = d 2^s = (v1, v0) has its top bit set whatever the size of d -- a divisor below 2^32 takes the
// same path with s >= 32 and v0 = 0, there is no one-digit branch.  The dividend is shifted by the same s on the fly (digit k of
// x 2^s is made of words k - s/32 and k - s/32 - 1 of x) and walked from the top; the quotient is unchanged by the shift and the
// remainder comes out as R >> s.  x 2^s has nw + 2 digits; its top two are below 2^s <= v, so they are the first partial remainder and
// exactly nw quotient digits follow.
//
// One step takes the partial remainder R = (r1, r0) < v and the next digit u to q = floor((R b + u) / v), b = 2^32, and the next R:
//   estimate   qhat = floor(R / v1), rhat = R mod v1; where r1 == v1 that quotient would be b or b + 1, and qhat = b - 1,
//              rhat = r0 + v1 is taken instead (DIV_SATURATED)
//   correct    while rhat < b and qhat v0 > rhat b + u: qhat -= 1, rhat += v1 -- at most twice (DIV_FIRST, DIV_SECOND): the estimate
//              exceeds q by at most 2 for a normalised divisor (Knuth's theorem B)
// With a two-digit divisor the test qhat v0 > rhat b + u IS qhat v > R b + u (rhat = R - qhat v1), so after the corrections qhat = q
// and algorithm D's add-back step never happens; where rhat >= b the test cannot hold (qhat v0 < b^2) and is skipped.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SC_DIV_FN __host__ __device__ __forceinline__
#else
#define SC_DIV_FN inline
#endif

namespace sc {

// the branches of one step, as indices of an optional tally (tests; the kernel passes none)
enum DivBranch { DIV_SATURATED = 0, DIV_FIRST = 1, DIV_SECOND = 2, DIV_BRANCHES = 3 };

// One quotient digit: R < v = (v1, v0), v1 >= 2^31; returns q and leaves R = (R b + u) - q v < v.
SC_DIV_FN uint32_t div_digit(uint64_t& R, uint32_t u, uint32_t v1, uint32_t v0, uint32_t* tally) {
  const uint32_t r1 = (uint32_t)(R >> 32), r0 = (uint32_t)R;
  uint64_t qhat, rhat;
  if (r1 == v1) {
    qhat = 0xffffffffull; rhat = (uint64_t)r0 + v1;
    if (tally) tally[DIV_SATURATED]++;
  } else {                                   // r1 < v1: the quotient fits a digit
    qhat = R / v1; rhat = R - qhat * v1;
  }
  if ((rhat >> 32) == 0 && qhat * v0 > ((rhat << 32) | u)) {
    qhat--; rhat += v1;
    if (tally) tally[DIV_FIRST]++;
    if ((rhat >> 32) == 0 && qhat * v0 > ((rhat << 32) | u)) {
      qhat--; rhat += v1;
      if (tally) tally[DIV_SECOND]++;
    }
  }
  R = (rhat << 32) + u - qhat * v0;          // below v < 2^64, so exact modulo 2^64 also where rhat >= b
  return (uint32_t)qhat;
}

// q[0 .. nw) = x div d and the return value x mod d, for x of nw >= 1 words and d != 0.  q may be x itself: step k reads words k - s/32
// and below of x before it writes word k of q, and no later step reads word k or above.
SC_DIV_FN uint64_t divmod_row(const uint32_t* x, int nw, uint64_t d, uint32_t* q, uint32_t* tally) {
  const int s = __builtin_clzll(d), ws = s >> 5, bs = s & 31;
  const uint64_t v = d << s;
  const uint32_t v1 = (uint32_t)(v >> 32), v0 = (uint32_t)v;
  // digit k of x 2^s is (hi << bs) | (lo >> (32 - bs)) with hi = word k - ws and lo = word k - ws - 1 of x (0 outside the row; ws is 0
  // or 1, so word nw + 1 - ws, the high half of digit nw + 1, is always outside)
  uint32_t hi = ws ? x[nw - 1] : 0u;                              // word nw - ws
  uint32_t lo = (nw - ws - 1 >= 0) ? x[nw - ws - 1] : 0u;
  const uint32_t d1 = bs ? (hi >> (32 - bs)) : 0u, d0 = bs ? ((hi << bs) | (lo >> (32 - bs))) : hi;
  uint64_t R = ((uint64_t)d1 << 32) | d0;
  for (int k = nw - 1; k >= 0; k--) {
    hi = lo;
    lo = (k - ws - 1 >= 0) ? x[k - ws - 1] : 0u;
    const uint32_t u = bs ? ((hi << bs) | (lo >> (32 - bs))) : hi;
    q[k] = div_digit(R, u, v1, v0, tally);
  }
  return R >> s;
}

}  // namespace sc

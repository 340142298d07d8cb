// The set-up-time integers of the host library: little-endian uint32 word vectors and the few operations that derive every key object,
// Montgomery constant and fixed-base table from them (never on a hot path).  HIP-free and context-free, like sc_route.h, sc_axis_plan.h,
// sc_pack_plan.h and sc_plain_words.h: only host units include it, and tests/test_bigint_cpu.py compiles it alone and compares every
// helper with Python integers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sc_host {

typedef std::vector<uint32_t> Big;

inline int big_bits(const Big& a) {
  for (int i = (int)a.size() - 1; i >= 0; i--)
    if (a[i]) return 32 * i + (32 - __builtin_clz(a[i]));
  return 0;
}
inline int big_cmp(const Big& a, const Big& b) {  // same length
  for (int i = (int)a.size() - 1; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i] ? 1 : -1;
  return 0;
}
inline void big_sub(Big& a, const Big& b) {  // a -= b, same length
  uint64_t borrow = 0;
  for (size_t i = 0; i < a.size(); i++) {
    uint64_t v = (uint64_t)a[i] - b[i] - borrow;
    a[i] = (uint32_t)v;
    borrow = (v >> 32) & 1;
  }
}
// a = 2a mod n  (a < n, a and n have the same length with one spare top word)
inline void big_dbl_mod(Big& a, const Big& n) {
  uint32_t carry = 0;
  for (size_t i = 0; i < a.size(); i++) {
    uint32_t nc = a[i] >> 31;
    a[i] = (a[i] << 1) | carry;
    carry = nc;
  }
  if (big_cmp(a, n) >= 0) big_sub(a, n);
}
// x * 2^k mod n
inline Big big_shl_mod(const Big& x, const Big& n, int k) {
  Big nn = n; nn.push_back(0);
  Big v = x; v.resize(nn.size(), 0);
  while (big_cmp(v, nn) >= 0) big_sub(v, nn);
  for (int i = 0; i < k; i++) big_dbl_mod(v, nn);
  v.resize(n.size());
  return v;
}
inline Big big_trimmed(Big a) { while (a.size() > 1 && a.back() == 0) a.pop_back(); return a; }
inline Big big_fit(Big a, size_t words) { a.resize(words, 0); return a; }
inline bool big_is_zero(const Big& a) { for (uint32_t w : a) if (w) return false; return true; }
inline bool big_is_one(const Big& a) { if (a.empty() || a[0] != 1) return false; for (size_t i = 1; i < a.size(); i++) if (a[i]) return false; return true; }
inline Big big_mul(const Big& a, const Big& b) {  // schoolbook product (set-up time only)
  Big r(a.size() + b.size(), 0);
  for (size_t i = 0; i < a.size(); i++) {
    uint64_t carry = 0;
    for (size_t j = 0; j < b.size(); j++) {
      uint64_t v = (uint64_t)a[i] * b[j] + r[i + j] + carry;
      r[i + j] = (uint32_t)v;
      carry = v >> 32;
    }
    r[i + b.size()] = (uint32_t)carry;
  }
  return r;
}
// x = q * m + rem by restoring division, bit by bit (set-up time only); q has x.size() words, rem m.size() words
inline void big_divmod(const Big& x, const Big& m, Big* q, Big* rem) {
  Big r(m.size() + 1, 0), mm = m; mm.push_back(0);
  q->assign(x.size(), 0);
  for (int bit = 32 * (int)x.size() - 1; bit >= 0; bit--) {
    uint32_t carry = (x[bit >> 5] >> (bit & 31)) & 1;
    for (size_t i = 0; i < r.size(); i++) { uint32_t nc = r[i] >> 31; r[i] = (r[i] << 1) | carry; carry = nc; }
    if (big_cmp(r, mm) >= 0) { big_sub(r, mm); (*q)[bit >> 5] |= 1u << (bit & 31); }
  }
  r.resize(m.size());
  *rem = r;
}
inline Big big_mod(const Big& x, const Big& m) { Big q, r; big_divmod(x, m, &q, &r); return r; }       // m.size() words
inline Big big_mulmod(const Big& a, const Big& b, const Big& m) { return big_mod(big_mul(a, b), m); }
// base^e mod m, set-up time only (square and multiply over the bits of e; m.size() words)
inline Big big_powmod(const Big& base, const Big& e, const Big& m) {
  Big r(m.size(), 0); r[0] = 1;
  r = big_mod(r, m);
  const Big b = big_mod(base, m);
  for (int i = big_bits(e) - 1; i >= 0; i--) {
    r = big_mulmod(r, r, m);
    if ((e[i >> 5] >> (i & 31)) & 1) r = big_mulmod(r, b, m);
  }
  return r;
}
inline Big big_sub_small(Big a, uint32_t k) { Big b(a.size(), 0); b[0] = k; big_sub(a, b); return a; }
inline void big_add_inplace(Big& a, const Big& b) {   // same length; the carry out is dropped (callers keep a spare top word)
  uint64_t c = 0;
  for (size_t i = 0; i < a.size(); i++) { c += (uint64_t)a[i] + b[i]; a[i] = (uint32_t)c; c >>= 32; }
}
inline void big_shr1(Big& a) { for (size_t i = 0; i < a.size(); i++) a[i] = (a[i] >> 1) | ((i + 1 < a.size()) ? (a[i + 1] << 31) : 0u); }
// a^-1 mod m for odd m (binary extended Euclid, HAC 14.61 shape); empty when gcd(a, m) != 1.  Result has m.size() words.
inline Big big_modinv_odd(const Big& a_in, const Big& m_in) {
  const size_t W = m_in.size() + 1;                         // one spare word: x + m never overflows
  const Big m = big_fit(m_in, W);
  Big u = big_fit(big_mod(a_in, m_in), W), v = m, x1(W, 0), x2(W, 0);
  x1[0] = 1;
  if (big_is_zero(u)) return Big();
  auto halve = [&](Big& x) { if (x[0] & 1) big_add_inplace(x, m); big_shr1(x); };
  while (!big_is_one(u) && !big_is_one(v)) {
    while (!(u[0] & 1)) { big_shr1(u); halve(x1); }
    while (!(v[0] & 1)) { big_shr1(v); halve(x2); }
    if (big_cmp(u, v) >= 0) { big_sub(u, v); if (big_cmp(x1, x2) < 0) big_add_inplace(x1, m); big_sub(x1, x2); }
    else { big_sub(v, u); if (big_cmp(x2, x1) < 0) big_add_inplace(x2, m); big_sub(x2, x1); }
    if (big_is_zero(u) || big_is_zero(v)) return Big();     // a common factor was subtracted away
  }
  Big r = big_is_one(u) ? x1 : x2;
  while (big_cmp(r, m) >= 0) big_sub(r, m);
  r.resize(m_in.size());
  return r;
}
// the limbs of x: S of them, W bits each (W < 32), low limb first; bits past the end of x read as 0
inline std::vector<uint32_t> to_limbs(const Big& x, int S, int W) {
  std::vector<uint32_t> out(S, 0);
  const uint32_t mask = (1u << W) - 1;
  for (int i = 0; i < S; i++) {
    int bit = W * i, w0 = bit >> 5, sh = bit & 31;
    uint64_t v = (w0 < (int)x.size()) ? x[w0] : 0;
    if (w0 + 1 < (int)x.size()) v |= (uint64_t)x[w0 + 1] << 32;
    out[i] = (uint32_t)(v >> sh) & mask;
  }
  return out;
}

}  // namespace sc_host

// Host logic of the pack step that the selection, the multiplication, the inner product and the one-hot encoding share: which
// rows make up each field of a message, how wide it is and how many messages carry it.  No HIP and no sc_ctx in here, so that a
// stand-alone host program can include this file alone and run it under a sanitizer.
#pragma once
#include <cstdint>
#include <vector>

namespace sc_host {

// One field of the messages, listed from the low end: its ciphertext rows [held][2 nw], its width in bits -- the shift of the field above
// it -- and the rows it holds, a prefix of the rows of the field below it.  Field 0 is held by every message.
struct PackField { const uint32_t* rows; int bits; uint64_t held; };

// Selection and multiplication: x in the low s bits, then column j of fbits[j] bits, so column j starts at off[j]; one message per row.
// `col` is the words of one plane, count * 2 nw.
static inline std::vector<PackField> column_fields(const uint32_t* x, const uint32_t* cols, int nf, int s, const int* fbits, uint64_t count, uint64_t col) {
  std::vector<PackField> fld{{x, s, count}};
  for (int j = 0; j < nf; j++) fld.push_back({cols + j * col, fbits[j], count});
  return fld;
}

// Inner product: pair j in message j mod M at position j div M, A at t pb and B at t pb + sa (a square has no B: y is not read and
// pb = sa).  The planes of one position are contiguous in x / y [k][count][2 nw]; the top position holds k - (npos - 1) M messages.
static inline std::vector<PackField> dot_fields(const uint32_t* x, const uint32_t* y, bool square, int k, int M, int sa, int sb, uint64_t count, uint64_t col) {
  const int npos = (k + M - 1) / M, n_top = k - (npos - 1) * M;
  std::vector<PackField> fld;
  for (int t = 0; t < npos; t++) {
    const uint64_t held = (uint64_t)(t == npos - 1 ? n_top : M) * count;
    fld.push_back({x + t * M * col, sa, held});
    if (!square) fld.push_back({y + t * M * col, sb, held});
  }
  return fld;
}

// One-hot encoding: index q in message q div g at position q mod g, f bits each.  `planes` holds the planes position by position: the
// indices themselves for M = 1, a gathered copy otherwise.  The last message has m - (M - 1) g fields; M - 1 messages hold the others.
static inline std::vector<PackField> onehot_fields(const uint32_t* planes, int m, int g, int M, int f, uint64_t count, uint64_t col) {
  const int F = M > 1 ? g : m, n_last = m - (M - 1) * g;
  std::vector<PackField> fld;
  for (int pos = 0; pos < F; pos++) {
    const uint64_t n = pos < n_last ? M : M - 1;
    fld.push_back({planes, f, n * count});
    planes += n * col;
  }
  return fld;
}

}  // namespace sc_host

// Stand-alone host check of csrc/sc_pack_plan.h: for every family the cumulative shift of each field equals the layout's bit
// offset, `held` equals the number of messages that carry the field, and every row a field names lies inside the array it came from.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/pack_plan_check.cpp -o pack_plan_check && ./pack_plan_check
#include "../protocols/secure_comparison_amd/csrc/sc_pack_plan.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

using namespace sc_host;

#define CHECK(c) do { if (!(c)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t COUNT = 3;
static const size_t W2 = 4, COL = COUNT * W2;      // words of a row and of a plane
static volatile uint32_t sink;

// bit offset of field f; reads the first and the last word the field holds, so that a row outside its array trips the sanitizer
static int shift_of(const std::vector<PackField>& fld, size_t f) {
  int s = 0;
  for (size_t i = 0; i < f; i++) s += fld[i].bits;
  CHECK(fld[f].held >= 1 && fld[f].held <= fld[0].held && (f == 0 || fld[f].held <= fld[f - 1].held));
  sink = fld[f].rows[0] + fld[f].rows[fld[f].held * W2 - 1];
  return s;
}

static void check_columns(int nf) {
  const int s = 41, fbits[4] = {50, 43, 77, 42};
  std::vector<uint32_t> x(COL), cols(nf * COL);
  const auto fld = column_fields(x.data(), cols.data(), nf, s, fbits, COUNT, COL);
  CHECK((int)fld.size() == nf + 1 && fld[0].rows == x.data() && shift_of(fld, 0) == 0 && fld[0].held == COUNT);
  for (int j = 0, off = s; j < nf; off += fbits[j++])            // off[j] as pack_fields (sc_families.hip) lays the columns out
    CHECK(shift_of(fld, j + 1) == off && fld[j + 1].rows == cols.data() + j * COL && fld[j + 1].held == COUNT);
}

static void check_dot(int k, int g, bool square) {
  const int sa = 50, sb = square ? 0 : 45, pb = sa + sb, fp = square ? 1 : 2, M = (k + g - 1) / g;
  std::vector<uint32_t> x(k * COL), y(square ? 0 : k * COL);
  const auto fld = dot_fields(x.data(), square ? nullptr : y.data(), square, k, M, sa, sb, COUNT, COL);
  const int npos = (int)fld.size() / fp;
  CHECK((int)fld.size() == fp * npos && npos <= g && fld[0].held == M * COUNT);
  std::vector<uint64_t> carried(npos, 0);
  for (int j = 0; j < k; j++) {                                  // pair j: message j mod M, position j div M
    const int msg = j % M, t = j / M;
    CHECK(t < npos);
    carried[t]++;
    CHECK(shift_of(fld, fp * t) == t * pb && fld[fp * t].rows + msg * COL == x.data() + j * COL && msg * COUNT < fld[fp * t].held);
    if (!square) CHECK(shift_of(fld, fp * t + 1) == t * pb + sa && fld[fp * t + 1].rows + msg * COL == y.data() + j * COL);
  }
  for (int f = 0; f < fp * npos; f++) CHECK(fld[f].held == carried[f / fp] * COUNT);
}

static void check_onehot(int m, int g) {
  const int f = 51, M = (m + g - 1) / g;
  std::vector<uint32_t> planes(m * COL);                         // index_enc (M = 1) or the gathered copy: m planes either way
  const auto fld = onehot_fields(planes.data(), m, g, M, f, COUNT, COL);
  CHECK((int)fld.size() == (M > 1 ? g : m) && fld[0].held == M * COUNT);
  std::vector<uint64_t> carried(fld.size(), 0);
  for (int q = 0; q < m; q++) {                                  // index q: message q div g, position q mod g
    const int msg = q / g, pos = q % g;
    CHECK(pos < (int)fld.size());
    carried[pos]++;
    CHECK(shift_of(fld, pos) == pos * f && msg * COUNT < fld[pos].held);
    if (M == 1) CHECK(fld[pos].rows == planes.data() + q * COL);
  }
  const uint32_t* next = planes.data();                          // the positions' planes follow each other without a gap
  for (size_t pos = 0; pos < fld.size(); next += carried[pos++] * COL) CHECK(fld[pos].rows == next && fld[pos].held == carried[pos] * COUNT);
  CHECK(next == planes.data() + planes.size());
}

int main() {
  for (int nf : {1, 4}) check_columns(nf);
  for (auto kg : {std::pair<int, int>{1, 7}, {7, 7}, {8, 7}, {17, 7}, {3, 1}}) check_dot(kg.first, kg.second, false);
  for (auto kg : {std::pair<int, int>{1, 14}, {14, 14}, {15, 14}}) check_dot(kg.first, kg.second, true);
  for (auto mg : {std::pair<int, int>{1, 20}, {20, 20}, {21, 20}, {11, 10}, {23, 10}}) check_onehot(mg.first, mg.second);
  std::printf("pack plan ok\n");
  return 0;
}

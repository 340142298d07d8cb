// The truncated sorting network of a secure top-m for a C host: sc_topk_network.  Host code only, no context and no
// device work.  Python derives the same network on its own (sorting.topk_network); the two are compared field by field in
// tests/test_topk_cpu.py, so a host that iterates these layers sends the key holder exactly the sub-batches he expects.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/sc_amd.h"

namespace {

constexpr int TK_MAX_K = 1024;   // sorting.MAX_K

struct TkCmp { int i, j; bool keep_i, keep_j; };

int tk_pow2_at_least(int x) { int n = 1; while (n < x) n <<= 1; return n; }

// Batcher's odd-even merge sort for n = 2^ceil(log2 k) without the comparators that touch an index >= k, shifted by `at`; with
// layer_end, the running comparator count after every layer that is not empty
void tk_batcher(int k, int at, std::vector<TkCmp>& seq, std::vector<int>* layer_end) {
  const int n = tk_pow2_at_least(k);
  for (int p = 1; p < n; p *= 2)
    for (int q = p; q >= 1; q /= 2) {
      const size_t before = seq.size();
      for (int j = q % p; j < n - q; j += 2 * q)
        for (int i = 0; i < std::min(q, n - j - q); ++i) {
          const int a = i + j, b = a + q;
          if (a / (2 * p) == b / (2 * p) && b < k) seq.push_back({at + a, at + b, true, true});
        }
      if (layer_end && seq.size() > before) layer_end->push_back((int)seq.size());
    }
}

// candidate (A): sorted blocks of mp = 2^ceil(log2 m), then per stride a half-cleaner and a bitonic merger that leave the mp smallest
// of blocks a and a + stride sorted in block a; false when one block spans the padded row
bool tk_truncated_merges(int k, int m, std::vector<TkCmp>& seq) {
  const int mp = tk_pow2_at_least(m);
  if (mp >= tk_pow2_at_least(k)) return false;
  std::vector<TkCmp> all;
  for (int a = 0; a < k; a += mp) tk_batcher(mp, a, all, nullptr);
  for (int stride = mp; stride < k; stride *= 2)
    for (int a = 0; a + stride < k; a += 2 * stride) {          // a block b at or past k is all +inf: nothing to merge
      const int b = a + stride;
      for (int i = 0; i < mp; ++i) all.push_back({a + i, b + mp - 1 - i, true, true});
      for (int q = mp / 2; q >= 1; q /= 2)
        for (int i = 0; i < mp; ++i)
          if ((i / q) % 2 == 0) all.push_back({a + i, a + i + q, true, true});
    }
  for (const TkCmp& c : all)
    if (c.j < k) seq.push_back(c);
  return true;
}

// backwards from the live outputs: drop what nothing reads, flag which output of the rest is read again
std::vector<TkCmp> tk_prune(const std::vector<TkCmp>& seq, int k, int m, bool only_last) {
  std::vector<char> live(k, 0);
  if (only_last) live[m - 1] = 1;
  else std::fill(live.begin(), live.begin() + m, 1);
  std::vector<TkCmp> out;
  for (size_t t = seq.size(); t-- > 0;) {
    const TkCmp& c = seq[t];
    if (!live[c.i] && !live[c.j]) continue;
    out.push_back({c.i, c.j, live[c.i] != 0, live[c.j] != 0});
    live[c.i] = live[c.j] = 1;
  }
  std::reverse(out.begin(), out.end());
  return out;
}

// every comparator into the earliest layer after the previous comparators of both positions; a layer keeps the sequential order
void tk_relayer(const std::vector<TkCmp>& seq, int k, std::vector<TkCmp>& out, std::vector<int>& layer_end) {
  std::vector<int> depth(k, 0), layer(seq.size());
  int layers = 0;
  for (size_t t = 0; t < seq.size(); ++t) {
    const int d = std::max(depth[seq[t].i], depth[seq[t].j]);
    layer[t] = d;
    depth[seq[t].i] = depth[seq[t].j] = d + 1;
    layers = std::max(layers, d + 1);
  }
  std::vector<int> start(layers + 1, 0);
  for (int d : layer) ++start[d + 1];
  for (int d = 0; d < layers; ++d) start[d + 1] += start[d];
  layer_end.assign(start.begin() + 1, start.end());
  out.resize(seq.size());
  for (size_t t = 0; t < seq.size(); ++t) out[start[layer[t]]++] = seq[t];
}

}  // namespace

extern "C" int sc_topk_network(int k, int m, int only_last, int cap, int32_t* ij_out, uint8_t* keep_out, int32_t* layer_end_out,
                               int* n_comparators, int* n_layers) {
  if (k < 1 || k > TK_MAX_K || m < 1 || m > k || (only_last != 0 && only_last != 1) || cap < 0 || !n_comparators || !n_layers)
    return SC_ERR_ARG;
  std::vector<TkCmp> net;
  std::vector<int> layer_end;
  if (m == k && !only_last) {
    tk_batcher(k, 0, net, &layer_end);                            // nothing to prune: Batcher's own layers
  } else {
    std::vector<TkCmp> full, merges;
    tk_batcher(k, 0, full, nullptr);
    std::vector<TkCmp> best = tk_prune(full, k, m, only_last != 0);
    if (tk_truncated_merges(k, m, merges)) {
      std::vector<TkCmp> cand = tk_prune(merges, k, m, only_last != 0);
      if (cand.size() < best.size()) best.swap(cand);             // the full sort's on a tie
    }
    tk_relayer(best, k, net, layer_end);
  }
  *n_comparators = (int)net.size();
  *n_layers = (int)layer_end.size();
  if (cap == 0) return SC_OK;                                     // the size query
  if ((size_t)cap < net.size() || !ij_out || !keep_out || !layer_end_out) return SC_ERR_ARG;
  for (size_t t = 0; t < net.size(); ++t) {
    ij_out[2 * t] = net[t].i; ij_out[2 * t + 1] = net[t].j;
    keep_out[2 * t] = net[t].keep_i; keep_out[2 * t + 1] = net[t].keep_j;
  }
  for (size_t t = 0; t < layer_end.size(); ++t) layer_end_out[t] = layer_end[t];
  return SC_OK;
}

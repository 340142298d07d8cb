// k_prod_axis: the product of residues along one axis of an array (the sum of Paillier ciphertexts), its instances and its launcher.
// A unit of its own, outside the interpreters: a chain of runtime length with an (outer, K, inner) geometry would cost every k_vm
// instance the registers of its index arithmetic, and the interpreter objects stay exactly what they were.
#include "sc_internal.h"
#include "sc_device.h"
#include "sc_launch_axis.h"

using namespace sc;

namespace sc {

// One level of the reduction tree.  The level's input is [outer][K][inner] numbers, its output [outer][nch][inner] with
// nch = ceil(K / chunk): chain t = (o * nch + ch) * inner + i multiplies the members j = ch * chunk .. of (o, i).
//   in_words: the members are canonical 32-bit words (the caller's array); otherwise lazily reduced limbs (partials)
//   final:    nch == 1 and the result leaves as canonical words after the product with `fin`; otherwise as limbs, lazily reduced
struct ReduceArgs {
  const uint32_t* modctx;   // n | R^2 | R in limb form
  const uint32_t* fin;      // the last level's closing factor R^K0 mod n in limb form, K0 the K of the whole call (else any S limbs)
  const uint32_t* src;
  uint32_t* dst;
  uint64_t K, inner, nch, nchains;
  uint32_t n0inv, chunk, nwords, in_words, final;
};

// One group of G lanes owns one chain, one wave per workgroup, grid-stride over the chains.  No operand is converted to Montgomery
// form and no product is followed by a reduction pass: the accumulator starts as the chain's first member as it is, every further
// member -- word form or partial -- is exactly one product acc * x / R with the accumulator staged in LDS and the member in this lane's
// limbs, and every such product leaves one factor 1 / R behind.  A tree over K0 members holds K0 - 1 products whatever its shape, so
// the root is prod x / R^(K0 - 1) and the last level's product with R^K0 (then / R) gives prod x exactly.  A group whose
// chain lies past the end of the level, and a member past the end of a short last chunk, still run every LDS and DPP step of their
// wave: the chain index is clamped and its store skipped, the missing member reads as R (acc * R / R = acc: no drift).
template <int G, int L>
__global__ void __launch_bounds__(64, 2) k_prod_axis(const ReduceArgs a) {
  using GT = Grp<G, L, 29>;
  constexpr int S = GT::S, NG = GT::NG, SP = GT::SP, WP = GT::WP;
  __shared__ uint32_t s_a[NG * SP];   // per group: the staged accumulator
  __shared__ uint32_t s_w[NG * SP];   // per group: word scratch of the format conversions
  __shared__ uint32_t s_c[2 * SP];    // the closing factor, R
  static_assert(WP <= SP, "word scratch must fit its area");

  GT gp;
  gp.init(a.modctx, a.n0inv);
  uint32_t* const my_a = s_a + gp.g * SP;
  uint32_t* const my_w = s_w + gp.g * SP;
  for (int t = threadIdx.x; t < S; t += 64) { s_c[t] = a.fin[t]; s_c[SP + t] = a.modctx[2 * S + t]; }
  SC_WAVE_SYNC();
  const uint32_t* const s_one = s_c + SP;
  const uint32_t in_stride = a.in_words ? a.nwords : (uint32_t)S;

  for (uint64_t base = (uint64_t)blockIdx.x * NG; base < a.nchains; base += (uint64_t)gridDim.x * NG) {
    const bool live = base + gp.g < a.nchains;
    const uint64_t t = live ? base + gp.g : a.nchains - 1;
    const uint64_t i = t % a.inner, och = t / a.inner;
    const uint64_t ch = och % a.nch, o = och / a.nch;
    const uint64_t j0 = ch * a.chunk;
    const uint32_t cnt = (uint32_t)((a.K - j0 < a.chunk) ? a.K - j0 : a.chunk);   // members of this chain, >= 1
    const uint32_t* const first = a.src + ((o * a.K + j0) * a.inner + i) * in_stride;
    const uint64_t step = a.inner * in_stride;

    uint32_t acc[L];
    if (a.in_words) gp.load_words(acc, first, (int)a.nwords, my_w); else gp.load_limbs(acc, first);
#pragma unroll 1
    for (uint32_t m = 1; m < a.chunk; m++) {
      const bool ok = m < cnt;
      const uint32_t* const p = first + (uint64_t)(ok ? m : cnt - 1) * step;
      uint32_t x[L];
      if (a.in_words) gp.load_words(x, p, (int)a.nwords, my_w); else gp.load_limbs(x, p);
#pragma unroll
      for (int l = 0; l < L; l++) x[l] = ok ? x[l] : s_one[gp.j * L + l];
      SC_WAVE_SYNC();
      gp.stage(my_a, acc);
      SC_WAVE_SYNC();
      uint32_t r[L];
      gp.mul(r, my_a, x);
#pragma unroll
      for (int l = 0; l < L; l++) acc[l] = r[l];
    }
    if (a.final) {
      uint32_t r[L];
      gp.mul(r, s_c, acc);          // acc R^K0 / R
      gp.canonical(r);
      gp.store_words(a.dst + t * a.nwords, (int)a.nwords, r, my_a, live);
    } else if (live) {
      gp.store_limbs(a.dst + t * S, acc);
    }
  }
}

}  // namespace sc

int sc_host::launch_prod_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* fin, const uint32_t* src, uint32_t* dst,
                              uint64_t K, uint64_t inner, uint32_t chunk, uint64_t nch, uint64_t nchains, int nwords, bool in_words, bool final) {
  ReduceArgs a;
  a.modctx = modctx; a.fin = fin; a.src = src; a.dst = dst; a.K = K; a.inner = inner; a.nch = nch; a.nchains = nchains;
  a.n0inv = n0inv; a.chunk = chunk; a.nwords = (uint32_t)nwords; a.in_words = in_words ? 1u : 0u; a.final = final ? 1u : 0u;
#define SC_REDUCE_CASE(GG, LL) if (W == 29 && G == GG && L == LL) return launch_axis<reduce_launch_key(GG, LL)>(ctx, k_prod_axis<GG, LL>, 64 / GG, nchains, a);
  SC_AXIS_INSTANCES(SC_REDUCE_CASE)
#undef SC_REDUCE_CASE
  return SC_ERR_UNSUPPORTED;
}

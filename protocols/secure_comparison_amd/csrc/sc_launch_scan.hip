// k_scan_axis: the running product of residues along one axis of an array (the running sum of Paillier ciphertexts), its instances and
// its launcher.  A unit of its own for the reason k_prod_axis is one: the interpreter objects, and sc_launch_reduce's, stay
// exactly what they were.
#include "sc_internal.h"
#include "sc_device.h"
#include "sc_launch_axis.h"

using namespace sc;

namespace sc {

// One launch of the blocked scan.  The level's input is [outer][K][inner] numbers, cut into nch = ceil(K / chunk) chunks along K: chain
// t = (o * nch + ch) * inner + i owns the members j = ch * chunk .. of (o, i) and writes, at every member's own position of `dst`
// ([outer][K][inner] canonical words), the product of its seed and of the members up to and including that one.
//   in_words: the members are canonical 32-bit words (the caller's array); otherwise lazily reduced limbs that carry a known power of
//             1 / R (the totals a k_prod_axis level left behind)
//   seed:     [outer][nch - 1][inner] canonical words, chunk ch > 0 starts from seed[o][ch - 1][i]; chunk 0, and every chunk of a
//             launch without seeds (seed == nullptr, nch == 1), starts from 1
//   lift:     the level's constant R^(e + 2) mod n in limb form, R^-e the drift of a member (e = 0, lift = R^2, for word form)
struct ScanArgs {
  const uint32_t* modctx;   // n | R^2 | R in limb form
  const uint32_t* lift;
  const uint32_t* src;
  const uint32_t* seed;
  uint32_t* dst;
  uint64_t K, inner, nch, nchains, chunk;   // (a direct launch's chunk is its K: 64 bits)
  uint32_t n0inv, nwords, in_words;
};

// One group of G lanes owns one chain, one wave per workgroup, grid-stride over the chains.  Every prefix is an output, so no drift may
// be left in it: the running prefix p is kept as the canonical residue that was just stored, and a member x R^-e costs two products,
//   q = p * lift / R = p R^(e + 1),    p' = q * (x R^-e) / R = p x,
// the second one canonical and stored.  The seed enters as p, a missing one as 1, so a launch is two products per member and nothing
// else: no conversion before, no reduction after.  A group whose chain lies past the end of the level, and a member past the end of a
// short last chunk, still run every LDS and DPP step of their wave: the chain index is clamped, the member re-reads the chunk's last
// one and the stores are skipped.
template <int G, int L>
__global__ void __launch_bounds__(64, 2) k_scan_axis(const ScanArgs a) {
  using GT = Grp<G, L, 29>;
  constexpr int S = GT::S, NG = GT::NG, SP = GT::SP, WP = GT::WP;
  __shared__ uint32_t s_a[NG * SP];   // per group: the staged q, then the limbs of the prefix on their way to words
  __shared__ uint32_t s_w[NG * SP];   // per group: word scratch of the format conversions
  __shared__ uint32_t s_f[SP];        // the level's constant
  static_assert(WP <= SP, "word scratch must fit its area");

  GT gp;
  gp.init(a.modctx, a.n0inv);
  uint32_t* const my_a = s_a + gp.g * SP;
  uint32_t* const my_w = s_w + gp.g * SP;
  for (int t = threadIdx.x; t < S; t += 64) s_f[t] = a.lift[t];
  SC_WAVE_SYNC();
  const uint32_t in_stride = a.in_words ? a.nwords : (uint32_t)S;

  for (uint64_t base = (uint64_t)blockIdx.x * NG; base < a.nchains; base += (uint64_t)gridDim.x * NG) {
    const bool live = base + gp.g < a.nchains;
    const uint64_t t = live ? base + gp.g : a.nchains - 1;
    const uint64_t i = t % a.inner, och = t / a.inner;
    const uint64_t ch = och % a.nch, o = och / a.nch;
    const uint64_t j0 = ch * a.chunk;
    const uint64_t cnt = (a.K - j0 < a.chunk) ? a.K - j0 : a.chunk;   // members of this chain, >= 1
    const uint64_t at = (o * a.K + j0) * a.inner + i;                              // the chain's first member, in numbers
    const uint32_t* const first = a.src + at * in_stride;
    uint32_t* const out = a.dst + at * a.nwords;
    const uint64_t step = a.inner * in_stride, ostep = a.inner * a.nwords;

    uint32_t p[L];
#pragma unroll
    for (int l = 0; l < L; l++) p[l] = (gp.j == 0 && l == 0) ? 1u : 0u;
    if (a.seed) {                                                                  // (the same way for the whole launch)
      const bool seeded = ch > 0;
      const uint32_t* const sp = a.seed + ((o * (a.nch - 1) + (seeded ? ch - 1 : 0)) * a.inner + i) * a.nwords;
      uint32_t s[L];
      gp.load_words(s, sp, (int)a.nwords, my_w);
#pragma unroll
      for (int l = 0; l < L; l++) p[l] = seeded ? s[l] : p[l];
    }
#pragma unroll 1
    for (uint64_t m = 0; m < a.chunk; m++) {
      const bool ok = m < cnt;
      const uint64_t at_m = ok ? m : cnt - 1;
      uint32_t x[L];
      if (a.in_words) gp.load_words(x, first + at_m * step, (int)a.nwords, my_w); else gp.load_limbs(x, first + at_m * step);
      uint32_t q[L];
      gp.mul(q, s_f, p);             // p R^(e + 1)
      SC_WAVE_SYNC();
      gp.stage(my_a, q);
      SC_WAVE_SYNC();
      gp.mul(p, my_a, x);            // p x
      gp.canonical(p);
      gp.store_words(out + at_m * ostep, (int)a.nwords, p, my_a, live && ok);
    }
  }
}

}  // namespace sc

int sc_host::launch_scan_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* lift, const uint32_t* src,
                              const uint32_t* seed, uint32_t* dst, uint64_t K, uint64_t inner, uint64_t chunk, uint64_t nch, uint64_t nchains, int nwords,
                              bool in_words) {
  ScanArgs a;
  a.modctx = modctx; a.lift = lift; a.src = src; a.seed = seed; a.dst = dst; a.K = K; a.inner = inner; a.nch = nch; a.nchains = nchains;
  a.n0inv = n0inv; a.chunk = chunk; a.nwords = (uint32_t)nwords; a.in_words = in_words ? 1u : 0u;
#define SC_SCAN_CASE(GG, LL) if (W == 29 && G == GG && L == LL) return launch_axis<scan_launch_key(GG, LL)>(ctx, k_scan_axis<GG, LL>, 64 / GG, nchains, a);
  SC_AXIS_INSTANCES(SC_SCAN_CASE)
#undef SC_SCAN_CASE
  return SC_ERR_UNSUPPORTED;
}

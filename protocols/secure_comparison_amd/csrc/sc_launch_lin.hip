// k_lin_axis: linear maps with public weights along one axis of an array of residues (a public weight matrix applied to Paillier
// ciphertexts), its lifting launch k_lin_lift, their instances and their launchers.  A unit of its own for the reason k_prod_axis and
// k_scan_axis are: the objects of the other units stay exactly what they were.
#include "sc_internal.h"
#include "sc_device.h"
#include "sc_launch_axis.h"

using namespace sc;

namespace sc {

// The lifting launch: every member of x ([count] canonical words) once into Montgomery form, one product with R^2, left as lazily
// reduced limbs in `dst` ([count][S]).
struct LinLiftArgs {
  const uint32_t* modctx;   // n | R^2 | R in limb form
  const uint32_t* src;
  uint32_t* dst;
  uint64_t count;
  uint32_t n0inv, nwords;
};

// One group of G lanes owns one member, one wave per workgroup, grid-stride over the members.  A group past the end re-reads the last
// member and skips its store.
template <int G, int L>
__global__ void __launch_bounds__(64, 2) k_lin_lift(const LinLiftArgs a) {
  using GT = Grp<G, L, 29>;
  constexpr int S = GT::S, NG = GT::NG, SP = GT::SP, WP = GT::WP;
  __shared__ uint32_t s_w[NG * SP];   // per group: word scratch of the format conversion
  __shared__ uint32_t s_r2[SP];       // R^2
  static_assert(WP <= SP, "word scratch must fit its area");

  GT gp;
  gp.init(a.modctx, a.n0inv);
  uint32_t* const my_w = s_w + gp.g * SP;
  for (int t = threadIdx.x; t < S; t += 64) s_r2[t] = a.modctx[S + t];
  SC_WAVE_SYNC();

  for (uint64_t base = (uint64_t)blockIdx.x * NG; base < a.count; base += (uint64_t)gridDim.x * NG) {
    const bool live = base + gp.g < a.count;
    const uint64_t t = live ? base + gp.g : a.count - 1;
    uint32_t x[L], r[L];
    gp.load_words(x, a.src + t * a.nwords, (int)a.nwords, my_w);
    gp.mul(r, s_r2, x);               // x R
    if (live) gp.store_limbs(a.dst + t * S, r);
  }
}

// One launch of the linear map.  The members are [outer][K][inner][S] lifted limbs (x R, lazily reduced), the weights w[J][K] 64-bit
// words with rowbits[j] the bit length of the largest weight of row j; out[o][j][i] = prod_k x[o][k][i]^w[j][k] mod n leaves as
// canonical words, [outer][J][inner][nwords].
struct LinArgs {
  const uint32_t* modctx;   // n | R^2 | R in limb form
  const uint32_t* lifted;
  const uint64_t* w;
  const uint32_t* rowbits;
  uint32_t* dst;
  uint64_t K, J, inner, npairs, nblocks, nwaves;   // npairs = outer * inner, nblocks = ceil(npairs / NG), nwaves = J * nblocks
  uint32_t n0inv, nwords;
};

// One group of G lanes owns one output, one wave per workgroup, grid-stride over the waves' work items (j, block): every group of a
// wave works on the same weight row j and on NG consecutive (o, i) pairs of `block`.  The weight bits are therefore the same in every
// lane: they are read with uniform addresses and steer a branch the whole wave takes or skips, so every LDS, DPP and barrier step is
// run by the whole wave.  The chain is the interleaved square and multiply over the K bases (Straus): from the Montgomery one, for
// every bit t = rowbits[j] - 1 .. 0 one squaring -- none while the accumulator is still R -- and one product with the lifted member
// k for every k whose weight has bit t set; then one reduction pass (the product by 1) takes the factor R off, and the canonical
// residue is stored.  Nothing drifts: every operand carries exactly one R.  The last block of every j is padded: a group past the
// last pair clamps its pair index and skips its store.
template <int G, int L>
__global__ void __launch_bounds__(64, 2) k_lin_axis(const LinArgs a) {
  using GT = Grp<G, L, 29>;
  constexpr int S = GT::S, NG = GT::NG, SP = GT::SP;
  __shared__ uint32_t s_a[NG * SP];    // per group: the staged accumulator, then the limbs of the result on their way to words
  __shared__ uint32_t s_a2[NG * SP];   // per group: the staged accumulator doubled (squarings)
  __shared__ uint32_t s_one[SP];       // R

  GT gp;
  gp.init(a.modctx, a.n0inv);
  uint32_t* const my_a = s_a + gp.g * SP;
  uint32_t* const my_a2 = s_a2 + gp.g * SP;
  for (int t = threadIdx.x; t < S; t += 64) s_one[t] = a.modctx[2 * S + t];
  SC_WAVE_SYNC();

  for (uint64_t v = blockIdx.x; v < a.nwaves; v += gridDim.x) {
    const uint64_t j = v / a.nblocks, blk = v - j * a.nblocks;
    const uint64_t pair = blk * NG + gp.g;
    const bool live = pair < a.npairs;
    const uint64_t p = live ? pair : a.npairs - 1;
    const uint64_t o = p / a.inner, i = p - o * a.inner;
    const uint32_t* const first = a.lifted + (o * a.K * a.inner + i) * S;   // member k at first + k * step
    const uint64_t step = a.inner * S;
    const uint64_t* const wrow = a.w + j * a.K;
    const int bits = (int)a.rowbits[j];

    uint32_t acc[L];
#pragma unroll
    for (int l = 0; l < L; l++) acc[l] = s_one[gp.j * L + l];
    bool fresh = true;                 // the accumulator is still R (the same in every lane: it depends on the weights alone)
#pragma unroll 1
    for (int t = bits - 1; t >= 0; t--) {
      if (!fresh) {
        uint32_t r[L];
        SC_WAVE_SYNC();
        gp.stage(my_a, acc);
        gp.stage_doubled(my_a2, acc);
        SC_WAVE_SYNC();
        gp.sqr(r, my_a, my_a2, acc);
#pragma unroll
        for (int l = 0; l < L; l++) acc[l] = r[l];
      }
#pragma unroll 1
      for (uint64_t k = 0; k < a.K; k++) {
        if (!((wrow[k] >> t) & 1ull)) continue;
        uint32_t x[L], r[L];
        gp.load_limbs(x, first + k * step);
        SC_WAVE_SYNC();
        gp.stage(my_a, acc);
        SC_WAVE_SYNC();
        gp.mul(r, my_a, x);
#pragma unroll
        for (int l = 0; l < L; l++) acc[l] = r[l];
        fresh = false;
      }
    }
    uint32_t r[L];
    gp.redc(r, acc);                   // the product by 1: acc / R
    gp.canonical(r);
    gp.store_words(a.dst + ((o * a.J + j) * a.inner + i) * a.nwords, (int)a.nwords, r, my_a, live);
  }
}

}  // namespace sc

int sc_host::launch_lin_lift(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* src, uint32_t* dst, uint64_t count,
                             int nwords) {
  LinLiftArgs a;
  a.modctx = modctx; a.src = src; a.dst = dst; a.count = count; a.n0inv = n0inv; a.nwords = (uint32_t)nwords;
#define SC_LIFT_CASE(GG, LL) if (W == 29 && G == GG && L == LL) return launch_axis<lin_launch_key(GG, LL, true)>(ctx, k_lin_lift<GG, LL>, 64 / GG, count, a);
  SC_AXIS_INSTANCES(SC_LIFT_CASE)
#undef SC_LIFT_CASE
  return SC_ERR_UNSUPPORTED;
}

int sc_host::launch_lin_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* lifted, const uint64_t* w,
                             const uint32_t* rowbits, uint32_t* dst, uint64_t outer, uint64_t K, uint64_t inner, uint64_t J, int nwords) {
  const uint64_t NG = 64 / (uint64_t)G;
  LinArgs a;
  a.modctx = modctx; a.lifted = lifted; a.w = w; a.rowbits = rowbits; a.dst = dst; a.K = K; a.J = J; a.inner = inner;
  a.npairs = outer * inner; a.nblocks = (a.npairs + NG - 1) / NG; a.nwaves = J * a.nblocks;
  a.n0inv = n0inv; a.nwords = (uint32_t)nwords;
  // launch_axis sizes its grid by chains of NG per wave: nwaves * NG of them are the nwaves work items of this kernel
#define SC_LIN_CASE(GG, LL) if (W == 29 && G == GG && L == LL) return launch_axis<lin_launch_key(GG, LL, false)>(ctx, k_lin_axis<GG, LL>, 64 / GG, a.nwaves * NG, a);
  SC_AXIS_INSTANCES(SC_LIN_CASE)
#undef SC_LIN_CASE
  return SC_ERR_UNSUPPORTED;
}

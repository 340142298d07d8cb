// What every translation unit of libsc_amd.so shares: the registered objects of a context (moduli, exponents, constants, tables,
// programs), the context itself, the one launch body of the one-wave-per-workgroup kernels (launch_waves) and what the kernel
// translation units export: one look-up of its instances per part of the two interpreters, a launch entry point per kernel elsewhere.
// The kernels are instantiated in sc_launch_vm.hip / sc_launch_pvm.hip (three parts each, compiled in parallel),
// sc_launch_misc.hip (with sc_kernel_plain.h), sc_launch_mul.hip, sc_launch_dot.hip, sc_launch_lookup.hip (each family's plain-word kernels
// in its own unit, the helpers they share in sc_plain_words.h), sc_launch_reduce.hip, sc_launch_scan.hip and
// sc_launch_lin.hip (the last three share their instance list and launcher, sc_launch_axis.h).  The host units (sc_lib.hip, sc_families.hip,
// sc_schemes.hip, sc_topk.hip) hold no device code; what they share among
// themselves is declared in sc_host.h, their set-up-time integers are sc_bigint.h, and a change of host logic rebuilds the units it
// touches, in seconds each.  Everything here has a name with linkage -- no unnamed namespace -- so that sc_ctx is one type in every unit.
// sc_route.h, included here, is the HIP-free list of the interpreters' instances, with their launch keys, and the policy that picks the
// instance of a launch: configurations, fit rule, twins.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/sc_amd_dev.h"
#include "sc_vm.h"
#include "sc_route.h"

#ifndef SC_INV_TOP
#define SC_INV_TOP 2048
#define SC_MAX_L 255      // widest comparison: l + 1 <= 256 bit planes (byte permutations, 8-bit flag fields; include/sc_amd.h)
#endif
#ifndef SC_PVM_WAVES
#define SC_PVM_WAVES 2    // waves per SIMD the pair interpreter is compiled for (sc_kernel_pvm.h)
#endif

namespace sc_host {

struct Mod {
  int G = 0, L = 0, W = 29, S = 0, nwords = 0, nbits = 0;
  std::vector<uint32_t> n;     // little-endian words (sc_bigint.h: Big)
  uint32_t n0inv = 0;
  uint32_t small_c = 0, small_cinv = 0;   // a modulus multiple M = c n (neg1_twin): c and c^-1 mod 2^W, else 0
  uint32_t* d_ctx = nullptr;  // n | R^2 | R  limb form
};
struct Exp { std::vector<uint32_t> e; int bits = 0; };
struct Const { int mod = -1; uint32_t* d_limbs = nullptr; };
// the rows of a fixed-base table are shared between contexts (sc_fbt_import): freed when the last table that uses them goes
struct FbtRows {
  int device = 0; uint32_t* d = nullptr; size_t bytes = 0;
  ~FbtRows() { if (d) { (void)hipSetDevice(device); (void)hipFree(d); } }
};
struct Fbt { int mod = -1, window = 0, nwin = 0, exp_bits = 0; uint32_t* d_rows = nullptr; std::shared_ptr<FbtRows> rows; };
struct Prog {
  uint32_t nops = 0, nscratch = 1, nconst = 0;
  sc::VmOp* d_ops = nullptr;
  uint32_t* d_consts = nullptr;
  double muls_per_item = 0;   // Montgomery products (full) per item
  double redcs_per_item = 0;  // reduction-only passes per item
  double sqrs_per_item = 0;   // squarings (a*a part costs L(L+1)/2 per block instead of L^2)
  std::shared_ptr<std::vector<sc::VmOp>> host_ops;   // the micro-ops on the host (pair programs: cut into segments on demand)
  uint32_t pair_sqrs = 0, pair_muls = 0;         // pair programs: pair squarings / pair products per item (the hold-time model)
  bool pair_dig = false;                         // pair programs with PV_MULTDIG: run on the k_pvm<.., DIG> instances
};

}  // namespace sc_host

struct sc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t switch_event = nullptr;   // orders the work of the previous stream before the next one (sc_ctx_set_stream)
  int num_cu = 256;
  std::string err;
  int64_t last_bad_index = -1;                              // the element named by the last SC_ERR_NOT_INVERTIBLE (sc_last_bad_index)
  std::vector<sc_host::Mod> mods;
  std::vector<sc_host::Exp> exps;
  std::vector<sc_host::Const> consts;
  std::vector<sc_host::Fbt> fbts;
  std::map<std::string, sc_host::Prog> progs;
  std::map<std::string, std::vector<sc_host::Prog>> seg_progs;   // pair programs cut into segments (sc_modexp_shared_sq)
  uint32_t* scratch = nullptr;
  size_t scratch_bytes = 0;
  std::vector<void*> owned;
  double mac_counter = 0;
  std::map<uint32_t, int> occ_cache;  // launch key of a kernel instance -> resident waves per CU (kernel_occupancy)
  std::map<int, std::pair<void*, size_t>> tmp;          // grow-only temporaries, reused across calls (same stream => ordered)
  std::map<std::vector<uint32_t>, uint32_t*> nwords_cache;  // device copy of {n, (n-1)/2} for the plain-word kernels
  std::map<int, int> kred_cache;                            // mod -> constant id of 2^(32 nwords) (wide-operand reduction)
  std::map<std::pair<int, std::vector<uint32_t>>, int> const_by_value;  // (mod, residue) -> constant id
  int latency_mode = 1;                                     // sc_ctx_set_latency_mode: 0 never, 1 automatic, 2 whenever available
  int onelane_mode = 1;                                     // sc_ctx_set_onelane_mode: 0 never, 1 automatic, 2 whenever available
  bool slot_per_item = false;                               // pair launches: a table slot per item instead of per resident wave (segments)
  // Segment policy of long pair launches on a shared chip (sc_modexp_shared_sq, sc_ctx_set_pair_policy): a resident wave should not
  // hold its slot for much longer than pair_hold_ms; launches of more than pair_max_rounds rounds are left whole
  double pair_hold_ms = 5.0, pair_max_rounds = 2.5;
  uint64_t stat_segmented_launches = 0, stat_segments = 0, stat_pair_calibrations = 0;   // sc_ctx_stats
  std::map<uint32_t, uint64_t> launch_counts;                // sc_ctx_launch_counts: launches per interpreter instance (launch_key)
  int chip_share = 1;                                       // sc_ctx_set_chip_share: contexts working on this GPU at the same time
  void* comm = nullptr;                                     // RCCL communicator of this rank (sc_comm_init), one context per GPU
  int comm_rank = 0, comm_nranks = 0;
  std::map<std::pair<int, int>, int> twins;                 // (twin kind, mod) -> its twin context, -1 where it has none (sc_lib.hip: twin_of)
  std::map<int, uint32_t*> pair_consts;                     // mod -> 4 limb arrays: pair(R^2), pair(B R) for the pair arithmetic
  uint32_t* d_one = nullptr;                                // the word 1 (a broadcast operand: the table entry x^0 of sc_modexp_var_sq)
  sc::RngKey rng_key;                                           // ChaCha20 key of the context's generator (sc_rng_seed)
  // fork / join inside one library call (AuxFork): independent halves of a small batch -- the p- and q-side of the key holder's CRT
  // -- run on a second stream of the context with its own scratch arena and temporaries
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  uint32_t* scratch_aux = nullptr;
  size_t scratch_aux_bytes = 0;
  bool in_aux = false;
  // verdict words of the inversion kernel: pinned host memory the kernel writes directly (one buffer per stream of the context), so
  // the host reads them after a stream synchronisation with no copy in between -- a device-to-host copy of a few words from pageable
  // memory is a runtime blit kernel (__amd_rocclr_copyBuffer) that queues behind other contexts' chip-filling launches
  int* status_host[2] = {nullptr, nullptr};
  size_t status_cap[2] = {0, 0};
  int fork_mode = 1;                                        // sc_ctx_set_fork_mode: 0 never fork inside a call, 1 automatic (small batches), 2 always
  void* scheme_keys = nullptr;                              // Paillier / DGK key objects of the scheme-level entry points (sc_schemes.hip)
  bool rng_seeded = false;
  std::atomic<uint64_t> rng_call{0};                        // generator calls since seeding: part of every keystream's nonce (atomic: two
                                                            // host threads that ever share a context must never draw one (key, call) twice)
  std::mutex rng_seed_mutex;                                // the lazy first seeding happens once
  uint64_t* stamps = nullptr;                               // sc_clock_probe: the next (4,18,neg1) pair launch runs its stamping twin
  uint32_t stamp_grid = 0;                                  // ... and reports its grid size here
  int reduce_chunk = 0;                                     // sc_ctx_set_reduce_chunk: 0 automatic, 2 .. 32 the chunk length of every level
  // (mod, e) -> limbs of R^e mod n (mont_power_limbs): the device copy and the pinned host buffer it is filled from (bounded)
  std::map<std::pair<int, uint64_t>, std::pair<uint32_t*, uint32_t*>> reduce_consts;
  // sc_modlin_axis: the pinned host buffer its weights are copied to the device from (grow-only), and the event of the last such copy
  void* lin_host = nullptr;
  size_t lin_host_bytes = 0;
  hipEvent_t lin_copied = nullptr;
};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sc_host::fail(ctx, SC_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

// ---- what the other translation units provide --------------------------------------------------------------------------------
namespace sc_host {
// sc_lib.hip
int fail(sc_ctx* ctx, int code, const char* fmt, ...);
int ensure_scratch(sc_ctx* ctx, size_t bytes, uint32_t** out);
// sc_launch_vm.hip / sc_launch_pvm.hip, parts 0 .. 2: the row of the interpreter instance with that launch_key, or null when the part
// does not compile it (each part holds its rows of the list in sc_route.h).  `launch` runs the instance on the context's stream (grid,
// scratch arena and launch count handled there); `occupancy` is its resident waves per CU (asked once per context), <= 0 when the
// query failed.
struct KernelRow { uint32_t key; int (*launch)(sc_ctx* ctx, const sc::VmArgs& a); int (*occupancy)(sc_ctx* ctx); };
const KernelRow* vm_part0(uint32_t key);
const KernelRow* vm_part1(uint32_t key);
const KernelRow* vm_part2(uint32_t key);
const KernelRow* pvm_part0(uint32_t key);
const KernelRow* pvm_part1(uint32_t key);
const KernelRow* pvm_part2(uint32_t key);

// Resident waves per CU of a one-wave-per-workgroup kernel: the runtime's occupancy answer held to 1 .. 16, cached in the context
// under the instance's launch key; 0 when the query failed.
template <typename Kernel>
int kernel_occupancy(sc_ctx* ctx, uint32_t key, Kernel kernel) {
  int& occ = ctx->occ_cache[key];                  // 0: not asked yet
  if (!occ) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64, 0) != hipSuccess) return 0;
    occ = std::max(1, std::min(nb, 16));
  }
  return occ;
}
// One launch of such a kernel on the context's stream, counted under `key`: `need` waves of work run as a grid-stride loop of at most
// num_cu * occupancy resident waves, or (grid_stride false) as a wave each.  `prepare(grid, args)` fills in what depends on the grid
// before the launch and may refuse it with an error code.
template <typename Args, typename Prepare>
int launch_waves(sc_ctx* ctx, uint32_t key, void (*kernel)(Args), uint64_t need, bool grid_stride, Args args, Prepare prepare) {
  const int occ = kernel_occupancy(ctx, key, kernel);
  if (occ <= 0) return fail(ctx, SC_ERR_HIP, "occupancy query failed for kernel instance %#x", key);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, grid_stride ? std::min<uint64_t>(need, (uint64_t)ctx->num_cu * occ) : need);
  const int rc = prepare(grid, args);
  if (rc) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, ctx->stream, args);
  ctx->launch_counts[key]++;
  HIPCHK(ctx, hipGetLastError());
  return SC_OK;
}
// What the launch entry points below share: their answer, 0 on success and a negative number when the launch itself failed, and the
// grid of a kernel that runs `count` items in blocks of 256 threads.
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
inline dim3 blocks256(uint64_t count) { return dim3((unsigned)((count + 255) / 256)); }
// sc_launch_misc.hip
int launch_xgcd(hipStream_t stream, const uint32_t* x, uint32_t* out, const uint32_t* d_n, int nw, uint64_t count, int* d_status);
int launch_plain_alice(hipStream_t stream, const uint32_t* r, const uint32_t* nmod, const uint32_t* halfn, int nw, int l, uint64_t count, uint32_t* m1,
                       uint64_t* alpha, uint64_t* alpha_tilde, uint64_t* rsmall, uint32_t* rshift);
int launch_plain_bob(hipStream_t stream, const uint32_t* z, const uint32_t* nmod, const uint32_t* halfn, int nw, int l, uint64_t count, uint64_t* beta,
                     uint64_t* dbit, uint32_t* zeta1, uint32_t* zeta2, uint8_t* bits);
int launch_select_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const sc::SelLayout& lay, int nw, int ew,
                       uint64_t count, uint32_t* R, uint32_t* e, uint32_t* rab);
int launch_select_split(hipStream_t stream, const uint32_t* p, int nw, const sc::SelLayout& lay, uint64_t count, uint32_t* prod, uint32_t* bad);
// sc_launch_mul.hip
int launch_mul_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const sc::MulLayout& lay, int nw, int ew,
                    uint64_t count, uint32_t* R, uint32_t* e, uint32_t* rab);
int launch_mul_split(hipStream_t stream, const uint32_t* p, int nw, const sc::MulLayout& lay, uint64_t count, uint32_t* prod, uint32_t* bad);
// sc_launch_dot.hip
int launch_dot_prep(hipStream_t stream, const uint32_t* ra, int aw, const uint32_t* rb, int bw, const sc::DotLayout& lay, int nw, int ew,
                    uint64_t count, uint32_t* e, uint32_t* R, uint32_t* S);
int launch_dot_split(hipStream_t stream, const uint32_t* p, int nw, const sc::DotLayout& lay, uint64_t count, uint32_t* D, uint32_t* bad);
// sc_launch_lookup.hip
int launch_onehot_prep(hipStream_t stream, const uint32_t* r, int rw, const sc::OnehotLayout& lay, int nw, uint64_t count, uint32_t* R, int32_t* rot);
int launch_onehot_split(hipStream_t stream, const uint32_t* p, int nw, const sc::OnehotLayout& lay, uint64_t count, uint32_t* prod, uint32_t* bad);
int launch_onehot_rotate(hipStream_t stream, const uint32_t* E, const int32_t* rot, int k, int m, int w2, uint64_t count, uint32_t* out);
// sc_launch_reduce.hip: one level of the product along an axis (k_prod_axis) on the context's stream; SC_ERR_UNSUPPORTED when
// (G, L, W) has no instance
int launch_prod_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* fin, const uint32_t* src, uint32_t* dst, uint64_t K,
                     uint64_t inner, uint32_t chunk, uint64_t nch, uint64_t nchains, int nwords, bool in_words, bool final);
// sc_launch_scan.hip: one launch of the running product along an axis (k_scan_axis) on the context's stream; `seed` may be null;
// SC_ERR_UNSUPPORTED when (G, L, W) has no instance
int launch_scan_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* lift, const uint32_t* src, const uint32_t* seed,
                     uint32_t* dst, uint64_t K, uint64_t inner, uint64_t chunk, uint64_t nch, uint64_t nchains, int nwords, bool in_words);
// sc_launch_lin.hip: the lifting launch (k_lin_lift: `count` members, words -> limbs of x R) and the linear map itself (k_lin_axis: w
// and rowbits on the device) on the context's stream; SC_ERR_UNSUPPORTED when (G, L, W) has no instance
int launch_lin_lift(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* src, uint32_t* dst, uint64_t count, int nwords);
int launch_lin_axis(sc_ctx* ctx, int G, int L, int W, const uint32_t* modctx, uint32_t n0inv, const uint32_t* lifted, const uint64_t* w, const uint32_t* rowbits,
                    uint32_t* dst, uint64_t outer, uint64_t K, uint64_t inner, uint64_t J, int nwords);
// sc_launch_misc.hip again
int launch_rng_bits(hipStream_t stream, const sc::RngKey& key, uint64_t call, int bits, int nw, uint32_t* out, uint64_t count);
int launch_rng_below(hipStream_t stream, const sc::RngKey& key, uint64_t call, const uint32_t* d_n, int nbits, int nw, int nonzero, uint32_t* out, uint64_t count);
int launch_rng_coins(hipStream_t stream, const sc::RngKey& key, uint64_t call, uint64_t* out, uint64_t count);
int launch_rng_perm(hipStream_t stream, const sc::RngKey& key, uint64_t call, int k, int64_t* out, uint64_t count);
int launch_peak_probe(hipStream_t stream, int grid, uint32_t* out, uint32_t a0, uint32_t b0, int iters);
// div/sc_kernel_divmod.h, compiled by sc_launch_misc.hip: q [count][nw] = x div d, rem = x mod d per row (k_divmod_words); q may be x
int launch_divmod_words(hipStream_t stream, const uint32_t* x, int nw, const uint64_t* d, uint64_t count, uint32_t* q, uint64_t* rem, uint32_t* bad);
}  // namespace sc_host

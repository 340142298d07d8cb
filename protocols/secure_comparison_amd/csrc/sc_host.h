// What the host units of libsc_amd.so share among themselves (sc_lib.hip, sc_families.hip, sc_schemes.hip): every helper that crosses a unit boundary is declared here once, under the unit that defines it, so
// no unit forward-declares a function and what one unit may use of another is what this file says.  Templates, the RAII helpers and the
// two program builders are defined here; everything else has its one definition in the named unit.  The kernel units never include this
// file (they see sc_internal.h only), and it holds no device code.
#pragma once
#include "sc_internal.h"
#include "sc_bigint.h"
#include "sc_axis_plan.h"
#include "sc_pack_plan.h"

#include <functional>
#include <type_traits>

namespace sc_host {
using namespace sc;

// ================================================================================================
// sc_lib.hip: memory of a context
// ================================================================================================
// every allocation selects the context's device first: the caller may have switched the thread's current device
int dev_alloc(sc_ctx* ctx, size_t bytes, void** out);
int upload(sc_ctx* ctx, const void* h, size_t bytes, void** out);
// Temporary device buffer `slot`, at least `bytes` large.  Buffers are reused by later calls: every kernel of a context
// runs on one stream, so a later call cannot overtake an earlier one that still reads the buffer.
int tmp_buf(sc_ctx* ctx, int slot, size_t bytes, void** out);
template <typename T>
int tmp_words(sc_ctx* ctx, int slot, uint64_t elems, T** out) { return tmp_buf(ctx, slot, (size_t)elems * sizeof(T), (void**)out); }
// Fork / join inside one library call.  begin(): everything queued so far on the context's stream happens before the forked work;
// until suspend() the context launches on its second stream (own scratch arena, own temporaries); after suspend() it is back on
// its own stream, whose later launches run BESIDE the forked work; join(): the context's stream waits for the forked work.
// (The forked half is queued first: an event recorded after the other half's launches would wait for them.)
// Used for the q-side of the key holder's CRT when a launch of the batch leaves most of the chip idle.
struct AuxFork {
  sc_ctx* ctx = nullptr;
  hipStream_t main = nullptr;
  bool active = false, pending = false;
  int begin(sc_ctx* c) {
    ctx = c;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->aux_stream) {
      HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
      HIPCHK(c, hipEventCreateWithFlags(&c->aux_fork, hipEventDisableTiming));
      HIPCHK(c, hipEventCreateWithFlags(&c->aux_join, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->aux_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->aux_stream, c->aux_fork, 0));
    main = c->stream;
    c->stream = c->aux_stream;
    c->in_aux = true;
    active = true;
    return SC_OK;
  }
  int suspend() {
    if (!active) return SC_OK;
    active = false;
    sc_ctx* c = ctx;
    const hipError_t e1 = hipEventRecord(c->aux_join, c->aux_stream);
    c->stream = main;
    c->in_aux = false;
    if (e1 != hipSuccess) return fail(c, SC_ERR_HIP, "hipEventRecord: %s", hipGetErrorString(e1));
    pending = true;
    return SC_OK;
  }
  int join() {
    int rc = suspend();
    if (rc) return rc;
    if (pending) { pending = false; HIPCHK(ctx, hipStreamWaitEvent(main, ctx->aux_join, 0)); }
    return SC_OK;
  }
  ~AuxFork() { (void)join(); }      // error paths: never leave the context on its second stream, nor forked work unordered
};
// Times work enqueued on the context's stream between two events (created on first use); they are destroyed on every path.
struct LaunchTimer {
  sc_ctx* ctx;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit LaunchTimer(sc_ctx* c) : ctx(c) {}
  // *ms = the time of what `enqueue` queues (it returns SC_OK or an error code, which is passed on), waited for
  template <class F> int time(F&& enqueue, float* ms) {
    if (!e0) HIPCHK(ctx, hipEventCreate(&e0));
    if (!e1) HIPCHK(ctx, hipEventCreate(&e1));
    HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
    int rc = enqueue(); if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(e1));
    HIPCHK(ctx, hipEventElapsedTime(ms, e0, e1));
    return SC_OK;
  }
  ~LaunchTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
// A measurement runs under a launch policy of its own and stays out of the MAC counter: the context's settings are restored on every
// exit path.
struct PolicyOverride {
  sc_ctx* ctx;
  const int latency_mode, onelane_mode, chip_share;
  const double mac_counter;
  explicit PolicyOverride(sc_ctx* c)
      : ctx(c), latency_mode(c->latency_mode), onelane_mode(c->onelane_mode), chip_share(c->chip_share), mac_counter(c->mac_counter) {}
  ~PolicyOverride() {
    ctx->latency_mode = latency_mode; ctx->onelane_mode = onelane_mode; ctx->chip_share = chip_share; ctx->mac_counter = mac_counter;
  }
};
// a device buffer of a measurement, freed on every exit path
template <class T> struct DevBuf {
  T* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
// Should the two CRT halves of a call run side by side on two streams?  Small batches: when a second, independent launch fits
// beside the first (a wave per SIMD for both: half of the chip's 4 x CUs SIMDs each; off with latency mode 0).  Large ones: when
// this context has the chip to itself.
inline bool small_enough_to_fork(const sc_ctx* ctx, const Mod& m, uint64_t count) {
  if (ctx->fork_mode == 0 || ctx->in_aux) return false;
  if (ctx->fork_mode == 2) return true;                     // always: the two halves' launches beside each other whatever the batch size
  // a context that has the chip to itself: the halves' launches side by side pack their partial rounds (three launches of 1.5
  // rounds each are 2 rounds long one after the other) -- single-stream step 381.1 -> 377.2 ms at B = 65536; with concurrent
  // shards the other shard's launches fill those rounds already and forking costs 1 % (profiles/r04_fork_modes.txt)
  if (ctx->chip_share == 1 && ctx->latency_mode != 2) {
    const uint64_t per_wave_full = std::max(1, 64 / m.G);
    if ((count + per_wave_full - 1) / per_wave_full > (uint64_t)ctx->num_cu * 4) return true;
  }
  if (ctx->latency_mode == 0) return false;
  if (ctx->latency_mode == 2) return true;
  const uint64_t per_wave = std::max(1, 64 / (2 * m.G));     // in the small-batch configuration this batch would take
  return (count + per_wave - 1) / per_wave <= (uint64_t)ctx->num_cu * 4 / (uint64_t)ctx->chip_share;
}

enum TmpSlot { TMP_PARK = 1, TMP_ANYFLAG = 2, TMP_CRT = 3, TMP_PAIR = 4, TMP_INV_MEMBERS = 5, TMP_REDUCE = 6, TMP_SCAN = 7, TMP_LIN = 8, TMP_INV_BASE = 16 /* + 2*depth, + 2*depth+1 */ };

// A u64 accumulator array of the context that is ZERO whenever no step is using it: cleared when it is (re)allocated, reset by its
// reader afterwards (OP_TAKEFLAG).  The zero tests of step 4j OR their verdicts into it; no clearing launch inside a step.
int zero_kept_flags(sc_ctx* ctx, uint64_t count, uint64_t** out);
void drop_zero_kept_flags(sc_ctx* ctx);      // forget the accumulator: the next use allocates and clears a new one

// `count` verdict words in pinned, device-visible host memory (grow-only, per stream of the context)
int status_words(sc_ctx* ctx, size_t count, int** out);

// device copy of n | (n-1)/2 as canonical words (plain-word kernels)
int device_n_half(sc_ctx* ctx, const uint32_t* n_hptr, int nw, uint32_t** out);

// Limb-form constant pairs of a modulus m for the pair arithmetic: pair(R^2) embeds an integer (u,0) -> u; pair(B R) is
// the radix B = 2^(32 nwords) of the operand chunks.  Each pair (c0, c1) satisfies c0 + c1 m = value (mod m^2), c0, c1 < m.
int get_pair_consts(sc_ctx* ctx, int mod, uint32_t** out);

// ------------------------------------------------------------------------------------------------
// program builders: every micro-op is emitted, and its cost counted, by one of these
// ------------------------------------------------------------------------------------------------
// k_vm programs.  Constants: LDS 0 = R^2, 1 = R, 2.. = the extra constants of use_const.
struct Builder {
  std::vector<VmOp> ops;
  std::vector<int> consts;  // extra constant ids (LDS index = 2 + position)
  int use_const(int cid) {
    for (size_t i = 0; i < consts.size(); i++) if (consts[i] == cid) return 2 + (int)i;
    consts.push_back(cid);
    return 2 + (int)consts.size() - 1;
  }
  void mul_const(int lds_idx) { emit(OP_MUL, AK_CONST, 0, lds_idx); muls++; }
  // times LDS constant lds0 where the item's byte in ext is 0, else lds1
  void mul_constsel(int ext, int lds0, int lds1) { emit(OP_MUL, AK_CONSTSEL, 0, ext, (uint32_t)lds0 | ((uint32_t)lds1 << 8)); muls++; }
  void sqr() {   // consecutive squarings merge into one micro-op with a repeat count (imm, 16 bits)
    sqrs++;
    if (!ops.empty()) {
      VmOp& last = ops.back();
      const uint32_t imm = last.w0 >> 16;
      if ((last.w0 & 0xffff) == (OP_MUL | (AK_ACC << 8)) && imm >= 1 && imm < 0xffff) { last.w0 += 1u << 16; return; }
    }
    emit(OP_MUL, AK_ACC, 1);
  }
  void mul_tbl(uint32_t e) { touch(e); emit(OP_MUL, AK_TBL, 0, e); muls++; }
  void mul_tblsel(int extA, int bitA, int extB, int bitB, uint32_t e00, uint32_t e01, uint32_t e10, uint32_t e11) {
    touch(std::max(std::max(e00, e01), std::max(e10, e11)));
    emit(OP_MUL, AK_TBLSEL, 0, extA | (bitA << 4) | (extB << 12) | (bitB << 16), e00 | (e01 << 8) | (e10 << 16) | (e11 << 24));
    muls++;
  }
  void mul_tbldig(int ext, uint32_t bitpos, uint32_t width, uint32_t base) {
    touch(base + (1u << width) - 1);
    emit(OP_MUL, AK_TBLDIG, 0, ext | (bitpos << 4) | (width << 24), base); muls++;
  }
  void mul_fbt(int ext, uint32_t bitpos, uint32_t width, uint32_t win) { emit(OP_MUL, AK_FBT, 0, ext | (bitpos << 4) | (width << 24), win); muls++; }
  void mul_extw(int ext, uint32_t off = 0) { emit(OP_MUL, AK_EXTW, 0, ext, off); muls++; }
  void mul_extl(int ext, uint32_t off = 0) { emit(OP_MUL, AK_EXTL, 0, ext, off); muls++; }
  void loadw(int ext, uint32_t off = 0, uint32_t woff = 0, uint32_t nw = 0) { emit(OP_LOADW, 0, 0, ext, off, (woff << 16) | nw); }
  // ext_set where bit `bit` (0 .. 255) of the item's flag row (ext flag_ext) is set, else ext_clear (sc_vm.h)
  void loadw_sel(int ext_set, int ext_clear, int flag_ext, int bit, uint32_t off = 0) { emit(OP_LOADW, 0, 1, ext_set | (ext_clear << 4) | (flag_ext << 8) | (bit << 12), off); }
  void add1() { emit(OP_ADD1); }
  void add_flag(int flag_ext, int bit, bool invert) { emit(OP_ADD1, 0, 1, flag_ext | (bit << 4) | ((invert ? 1 : 0) << 12)); }
  void sub1() { emit(OP_SUB1); }
  void neg() { emit(OP_NEG); }
  void quot() { emit(OP_QUOT); redcs++; }
  void addw(int ext, uint32_t off = 0, uint32_t woff = 0, uint32_t nw = 0) { emit(OP_ADDW, 0, 0, ext, off, (woff << 16) | nw); }
  void loadt_const(int lds_idx) { emit(OP_LOADT, AK_CONST, 0, lds_idx); }
  void loadt_tbl(uint32_t e) { touch(e); emit(OP_LOADT, AK_TBL, 0, e); }
  void loadt_tbldig(int ext, uint32_t bitpos, uint32_t width, uint32_t base) {
    touch(base + (1u << width) - 1);
    emit(OP_LOADT, AK_TBLDIG, 0, ext | (bitpos << 4) | (width << 24), base);
  }
  void loadt_tblsel(int extA, int bitA, int extB, int bitB, uint32_t e00, uint32_t e01, uint32_t e10, uint32_t e11) {
    touch(std::max(std::max(e00, e01), std::max(e10, e11)));
    emit(OP_LOADT, AK_TBLSEL, 0, extA | (bitA << 4) | (extB << 12) | (bitB << 16), e00 | (e01 << 8) | (e10 << 16) | (e11 << 24));
  }
  void loadt_fbt(int ext, uint32_t bitpos, uint32_t width, uint32_t win) { emit(OP_LOADT, AK_FBT, 0, ext | (bitpos << 4) | (width << 24), win); }
  void loadt_extl(int ext, uint32_t off = 0) { emit(OP_LOADT, AK_EXTL, 0, ext, off); }
  // ACC = the u64 accumulator ext_acc[item], which is reset to 0; the value also goes to ext_copy[item] (sc_vm.h)
  void takeflag(int ext_acc, int ext_copy) { emit(OP_TAKEFLAG, 0, 0, ext_acc, ext_copy); }
  void stt(uint32_t e) { touch(e); emit(OP_STT, 0, e); }
  void addt(uint32_t e) { touch(e); emit(OP_ADDT, 0, e); }
  void redc(bool times_c = false) { emit(OP_REDC, 0, times_c ? 1 : 0); redcs++; }     // times_c / over_c: leaving a modulus-multiple context (sc_vm.h)
  void storew(int ext, uint32_t off = 0, bool over_c = false) { emit(OP_STOREW, 0, over_c ? 1 : 0, ext, off); }
  void storew_at(int ext, int ext_index, bool over_c = false, bool by_perm = false) {   // row = ext_index[item] (u64), or from a batch of permutations (sc_vm.h)
    emit(OP_STOREW, 0, (over_c ? 1 : 0) | (by_perm ? 2 : 0), ext, 0, 1 + ext_index);
  }
  void storel(int ext, uint32_t off = 0) { emit(OP_STOREL, 0, 0, ext, off); }
  // or_group: OR the verdict into the item's group flag (u64) instead of storing a byte
  void storeflag(int ext, uint32_t off, int lds_const, bool or_group = false) { emit(OP_STOREFLAG, 0, or_group ? 1 : 0, ext, off, lds_const); }
  // ends the program and uploads it with its constants for modulus `mod`
  int finalize(sc_ctx* ctx, int mod, Prog* out) {
    emit(OP_END);
    if (consts.size() + 2 > VM_MAX_CONST) return fail(ctx, SC_ERR_ARG, "too many constants in program");
    const Mod& m = ctx->mods[mod];
    Prog p;
    p.nops = (uint32_t)ops.size();
    p.nscratch = nscratch;
    p.nconst = (uint32_t)consts.size();
    p.muls_per_item = muls;
    p.redcs_per_item = redcs;
    p.sqrs_per_item = sqrs;
    int rc = upload(ctx, ops.data(), ops.size() * sizeof(VmOp), (void**)&p.d_ops);
    if (rc) return rc;
    if (p.nconst) {
      rc = dev_alloc(ctx, (size_t)p.nconst * m.S * 4, (void**)&p.d_consts);
      if (rc) return rc;
      for (uint32_t i = 0; i < p.nconst; i++)
        HIPCHK(ctx, hipMemcpyAsync(p.d_consts + (size_t)i * m.S, ctx->consts[consts[i]].d_limbs, (size_t)m.S * 4,
                                   hipMemcpyDeviceToDevice, ctx->stream));   // stream-ordered before the program's first launch
    }
    *out = p;
    return SC_OK;
  }

 private:
  uint32_t nscratch = 1;
  double muls = 0, redcs = 0, sqrs = 0;
  void touch(uint32_t e) { nscratch = std::max(nscratch, e + 1); }
  void emit(uint32_t opc, uint32_t ak = 0, uint32_t imm = 0, uint32_t w1 = 0, uint32_t w2 = 0, uint32_t w3 = 0) {
    ops.push_back(VmOp{opc | (ak << 8) | (imm << 16), w1, w2, w3});
  }
};

// the encoding of one k_pvm micro-op (PairBuilder, and the segment cutter of sc_modexp_shared_sq)
inline VmOp pv_op(uint32_t opc, uint32_t w1 = 0, uint32_t w2 = 0, uint32_t w3 = 0) { return VmOp{opc, w1, w2, w3}; }

// k_pvm programs.  Constants: LDS 2,3 = pair(R^2), 4,5 = pair(B R) (get_pair_consts).  Pair entry e of the table is limb-form
// entries 2e and 2e + 1.  Costs: muls_per_item carries the exact multiply-adds per item -- a pair squaring is (a*a part) + 3 S^2,
// a pair product 5 S^2 with the two-row pass, 6 S^2 in the one-lane form (three single passes over one staging area).
struct PairBuilder {
  std::vector<VmOp> ops;
  explicit PairBuilder(const Mod& m)
      : one_lane(m.G == 1), S2((double)m.S * m.S), SQ(S2 + (double)m.G * m.G * m.L * (m.L + 1) / 2.0 + 2.0 * S2),
        MU((m.G == 1 ? 6.0 : 5.0) * S2) {}
  // ACC0 = words ext[ext] (row `row` of a [rows][count] operand, word offset woff, nw words), ACC1 = 0
  void loadu(int ext, uint32_t woff, uint32_t nw, uint32_t row = 0) { ops.push_back(pv_op(PV_LOADU, ext, row, (woff << 16) | nw)); }
  void mul_const(uint32_t lds_idx) { ops.push_back(pv_op(PV_MULC, lds_idx)); macs += MU; muls++; }
  void sqr() { ops.push_back(pv_op(PV_SQR)); macs += SQ; sqrs++; }
  void mul_tbl(uint32_t e) { touch(e); ops.push_back(pv_op(PV_MULT, e)); macs += MU; muls++; }
  // pair *= entry base + digit, the digit `width` bits at `bitpos` of the item's row in ext (k_pvm<.., DIG> instances only)
  void mul_tbl_digit(int ext, uint32_t bitpos, uint32_t width, uint32_t base) {
    touch(base + (1u << width) - 1); dig = true;
    ops.push_back(pv_op(PV_MULTDIG, ext | (bitpos << 4) | (width << 24), base)); macs += MU; muls++;
  }
  void loadt_tbl(uint32_t e) { touch(e); ops.push_back(pv_op(PV_LOADT, e)); }
  void stt(uint32_t e) { touch(e); ops.push_back(pv_op(PV_STT, e)); }
  void addt(uint32_t e) { touch(e); ops.push_back(pv_op(PV_ADDT, e)); }
  void out(int ext0, int ext1) { ops.push_back(pv_op(PV_OUT, ext0, ext1)); macs += 2.0 * S2; }
  // ends the program and uploads it; the host copy of the ops stays with it (segments are cut from it on demand)
  int finalize(sc_ctx* ctx, int mod, Prog* out) {
    ops.push_back(pv_op(PV_END));
    Prog p;
    // one-lane pair products park an intermediate in a spare row (the last one) of the slot's table
    p.nops = (uint32_t)ops.size(); p.nscratch = nscratch + (one_lane ? 1 : 0); p.nconst = 4; p.muls_per_item = macs;
    p.pair_sqrs = sqrs; p.pair_muls = muls; p.pair_dig = dig;
    p.host_ops = std::make_shared<std::vector<VmOp>>(ops);
    int rc = upload(ctx, ops.data(), ops.size() * sizeof(VmOp), (void**)&p.d_ops); if (rc) return rc;
    rc = get_pair_consts(ctx, mod, &p.d_consts); if (rc) return rc;
    *out = p;
    return SC_OK;
  }

 private:
  bool one_lane;
  double S2, SQ, MU, macs = 0;
  uint32_t nscratch = 2, sqrs = 0, muls = 0;
  bool dig = false;
  void touch(uint32_t e) { nscratch = std::max(nscratch, 2 * e + 2); }
};

// The program cached under `key` in the context, or the one `build` emits into `bd`, finalized for modulus `mod` and cached.
// `build` may return an error code, which is passed on (nothing is cached then).
template <class F, class B = Builder>
int cached_prog(sc_ctx* ctx, const std::string& key, int mod, F&& build, const Prog** out, B bd = B()) {
  auto it = ctx->progs.find(key);
  if (it == ctx->progs.end()) {
    if constexpr (std::is_void_v<decltype(build(bd))>) build(bd);
    else { int rc = build(bd); if (rc) return rc; }
    Prog p; int rc = bd.finalize(ctx, mod, &p); if (rc) return rc;
    it = ctx->progs.emplace(key, p).first;
  }
  *out = &it->second;
  return SC_OK;
}

// what the instance policy (sc_route.h) is asked with: the switches of the context, and a modulus as it sees one
inline Policy policy_of(const sc_ctx* ctx) { return {ctx->latency_mode, ctx->onelane_mode, ctx->chip_share, ctx->num_cu}; }
inline Instance shape_of(const Mod& m) { return {m.G, m.L, m.W, m.n0inv == 1}; }

int run_vm(sc_ctx* ctx, int mod, const Prog& p, const VmExt* exts, int next, uint64_t count, const uint32_t* fbt_rows = nullptr);

// resident waves per CU of that instance (the runtime's occupancy answer, not a compiled-in assumption); <= 0 when there is none
int pvm_occupancy(sc_ctx* ctx, int G, int L, bool neg1);

// pair programs: nscratch counts limb-form entries (2 per pair entry); macs = multiply-adds per item
int run_pvm(sc_ctx* ctx, int mod, const Prog& p, const VmExt* exts, int next, uint64_t count);

inline VmExt mk_ext(const void* p, uint32_t stride, uint32_t nwords, uint64_t limit = ~0ull) {
  VmExt e; e.ptr = p; e.stride = stride; e.nwords = nwords; e.limit = limit; return e;
}

inline bool valid_mod(sc_ctx* ctx, int mod) { return ctx && mod >= 0 && mod < (int)ctx->mods.size(); }

// emit: ACC = (ext value reduced mod n), for an operand of x_words >= mod words (Horner over chunks)
void emit_load_reduced(sc_ctx* ctx, const Mod& m, Builder& b, int ext, int x_words, int kred_lds);

int best_window(int bits);
inline int ebit(const Big& e, int i) { return (e[i >> 5] >> (i & 31)) & 1; }

// emit sliding-window exponentiation (ex.bits > 0) of the Montgomery-form value currently in the accumulator, with the table of odd
// powers x^1, x^3, .. in entries T0, T0 + 1, .. and x^2 in the entry after them; leaves x^e.  Either builder (k_vm or k_pvm).
template <class B>
void emit_window_pow(B& b, const Exp& ex, uint32_t T0) {
  const int bits = ex.bits;
  const int w = best_window(bits);
  const uint32_t NT = 1u << (w - 1);
  b.stt(T0);
  if (NT > 1) {
    b.sqr(); b.stt(T0 + NT);
    for (uint32_t k = 1; k < NT; k++) { b.loadt_tbl(T0 + k - 1); b.mul_tbl(T0 + NT); b.stt(T0 + k); }
  }
  bool first = true;
  int i = bits - 1;
  while (i >= 0) {
    if (!ebit(ex.e, i)) { b.sqr(); i--; continue; }
    int j = std::max(0, i - w + 1);
    while (!ebit(ex.e, j)) j++;
    int v = 0;
    for (int k = i; k >= j; k--) v = (v << 1) | ebit(ex.e, k);
    if (first) { b.loadt_tbl(T0 + (v - 1) / 2); first = false; }
    else { for (int k = 0; k < i - j + 1; k++) b.sqr(); b.mul_tbl(T0 + (v - 1) / 2); }
    i = j - 1;
  }
}

// x^e of the Montgomery-form value in ACC, left in ACC (Montgomery form); x^0 is the constant 1
void emit_pow_shared(Builder& b, const Exp& ex);

// ================================================================================================
// sc_lib.hip: registration, and the entries' bodies that other units call with more arguments than the C ABI carries
// ================================================================================================
// for_pairs: take the first configuration that has a pair kernel (used for the internal twin context of sc_modexp_shared_sq);
// forced: this configuration or failure (the one-lane twin)
int create_mod(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, bool for_pairs, int* out_mod, const Config* forced = nullptr);
// registers the residue v (host words) as a constant of `mod` once per (mod, value)
int sc_const_create_cached(sc_ctx* ctx, int mod, const Big& v, int* out_cid);
// Montgomery form of 2^(32 * nwords): multiplying by it shifts a residue up by one operand width
int get_const_kred(sc_ctx* ctx, int mod, int* out_cid);
// any_flags_clean: the caller guarantees that any_flags[0 .. inner) is zero already (a context-owned accumulator that its reader
// resets, OP_TAKEFLAG): no clearing launch
int modexp_shared_impl(sc_ctx* ctx, int mod, int exp, const uint32_t* x, int x_words, const uint32_t* mul_into, uint32_t* out, uint8_t* flags,
                       uint64_t count, uint64_t* any_flags, uint64_t inner, bool any_flags_clean = false);
// premul (nullable): a finished factor per item (e.g. a randomizer h^r computed ahead of time on another stream) multiplied in
// before the store -- the alternative to the fixed-base tail (fbt / e2)
// perm (nullable, instead of dest): int64 [count / planes][planes], one permutation per comparison of a bit-major vector
// [planes][inner]: item (j, b) is stored at plane k with perm[b][k] == j (the step-4i shuffle inside the store)
int modexp_var_impl(sc_ctx* ctx, int mod, const uint32_t* x, const uint32_t* e, int ewords, int ebits, int fbt, const uint32_t* e2, int e2words,
                    const uint64_t* dest, uint32_t* out, uint64_t count, const uint32_t* premul = nullptr, const int64_t* perm = nullptr,
                    uint32_t planes = 0);
// bits (nullable): additionally the bytes [l+1][count] of d and the bits of beta (k_plain_bob)
int plain_bob_impl(sc_ctx* ctx, const uint32_t* z, const uint32_t* n_hptr, int nw, int l, uint64_t count, uint64_t* beta, uint64_t* dbit,
                   uint32_t* zeta1, uint32_t* zeta2, uint8_t* bits);

// ================================================================================================
// sc_lib.hip: twins and the one-lane policy's calibration
// ================================================================================================
// The neg1 twin of `mod` (the context of its multiple M = c n = -1 mod 2^29) for the single-modulus interpreter when this batch should
// run on it, else -1: only the (4,18) instance k_vm<4,18,29,true> exists, and only programs whose outputs are word stores can use it
// (modexp_var_impl: the blinding launch of step 4i) -- limb-form outputs would carry residues up to 2M into launches of the original context.
int neg1_vm_twin(sc_ctx* ctx, int mod, uint64_t count);
// the one-lane twin of `mod` when this batch should run on it, else `mod` itself
int onelane_for(sc_ctx* ctx, int mod, uint64_t count);
// the calibration of this context's device (measured by the first context that asks; a failed measurement leaves round 3's constants)
OneLaneCal onelane_cal(sc_ctx* ctx);

// ================================================================================================
// sc_families.hip: the layout rules and refusals that the scheme-level entries (sc_schemes.hip) check as well
// ================================================================================================
// SelectLayout.__post_init__ (selection.py) on the host -- the one copy of the rule every selection entry checks before it launches
// anything (sc_select_prep / sc_select_split, the scheme-level entries of sc_schemes.hip)
int select_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int nfields, const int* widths, SelLayout* lay);
// MulLayout.__post_init__ (multiplication.py) on the host -- the one copy of the fit rule every multiplication entry checks before it
// launches anything: s + sum_j fbits_j < bits(N) - 1 and every s + fbits_j < bits(N) - 1
int mul_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int wx, int nfields, const int* wy, int is_signed, MulLayout* lay);
int mul_ebits(const MulLayout& lay);
// two refusals the scheme-level entries share: exponent rows of ew words hold `bits` bits; finish_ratio's coef is +1, -1 or -2
int exp_rows(sc_ctx* ctx, const char* who, int ew, int bits);
int ratio_coef(sc_ctx* ctx, const char* who, int coef);
// the draws' and exponents' row widths of the multiplication and the inner product: the kernels hold a field in MUL_FIELD_WORDS words
// (bw_max: the multiplication's r_b rows are no wider than N either; has_b: a square reads no r_b)
int row_words(sc_ctx* ctx, const char* who, int ebits, int aw, int bw, bool has_b, int bw_max, int ew);
// DotLayout.__post_init__ (dotproduct.py) on the host -- the one copy of the fit rule every inner-product entry checks before it launches
// anything: g = the largest integer with g pb < bits(N) - 1 must be at least 1, and the sum of k products must stay below N:
// pb' + ceil(log2 k) < bits(N) - 1 with pb' = sa + sb (2 sa for a square).  Every refusal names its quantity.
int dot_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int wx, int wy, int is_signed, int square, int k, DotLayout* lay);
// OnehotLayout.__post_init__ (lookup.py) on the host -- the one copy of the fit rule every one-hot entry checks before it launches
// anything: a field of f = ib + kappa + 1 bits must fit, f < bits(N) - 1; then g = floor((bits(N) - 2) / f) >= 1 fields per message.
// Every refusal names its quantity.
int onehot_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int ib, int k, int m, OnehotLayout* lay);
// the launches number their rows in 32 bits
int onehot_rows(sc_ctx* ctx, const char* who, int k, int m, uint64_t count);
int onehot_mask_words(sc_ctx* ctx, const char* who, const OnehotLayout& lay, int rw);
// out [m][k][count][words] from e [m][k][count][words] and rot [m][count]; the two arrays must not overlap: a row of out is read from
// another row of e
int onehot_rotate(sc_ctx* ctx, const char* who, int words, int k, int m, const uint32_t* e, const int32_t* rot, uint32_t* out, uint64_t count);

// ================================================================================================
// sc_schemes.hip: the key tables of a context (sc_ctx::scheme_keys), whose types stay in that unit
// ================================================================================================
void free_scheme_keys(void* p);
// The zero-divisor verdict of sc_plain_divmod: SC_OK, or SC_ERR_ARG once (the verdict is cleared) when a division queued on this context
// met a divisor of zero.  The caller has synchronised the context's stream (sc_ctx_synchronize asks after it has).
int div_verdict_check(sc_ctx* ctx);

}  // namespace sc_host

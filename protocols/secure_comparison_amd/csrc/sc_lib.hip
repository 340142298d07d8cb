// libsc_amd.so -- host side of the C ABI declared in include/sc_amd.h and include/sc_amd_dev.h: the context's life cycle and memory, the
// runners of the micro-programs (sc_vm.h; the builders are in sc_host.h), the registration of moduli, exponents, constants and tables, the
// modmul, modexp, fixed-base, Paillier raw and plain-word entries, the inversion, the axis entries, twins with the two calibrations and
// the pair arithmetic, RCCL with the generator, the policy setters, stats and probes.  The other host units hold the families
// (sc_families.hip), the schemes (sc_schemes.hip) and the top-m network (sc_topk.hip); what they use of this one is declared in sc_host.h;
// the kernels are instantiated in the sc_launch_*.hip translation units (sc_internal.h), so no host unit holds device code.
#include "sc_host.h"

#include <dlfcn.h>
#include <sys/random.h>

using namespace sc;
using namespace sc_host;

namespace sc_host {
int fail(sc_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

int dev_alloc(sc_ctx* ctx, size_t bytes, void** out) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc(out, bytes ? bytes : 4));
  ctx->owned.push_back(*out);
  return SC_OK;
}
int upload(sc_ctx* ctx, const void* h, size_t bytes, void** out) {
  int rc = dev_alloc(ctx, bytes, out);
  if (rc) return rc;
  // on the context's stream, then waited for: a plain hipMemcpy runs on the null stream, which does not order with the
  // non-blocking streams a caller may hand in (torch side streams), and the source is a short-lived host buffer
  HIPCHK(ctx, hipMemcpyAsync(*out, h, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}
// the scratch arena of the stream the context currently launches on (its own, or the forked one's: AuxFork)
int ensure_scratch(sc_ctx* ctx, size_t bytes, uint32_t** out) {
  uint32_t*& arena = ctx->in_aux ? ctx->scratch_aux : ctx->scratch;
  size_t& have = ctx->in_aux ? ctx->scratch_aux_bytes : ctx->scratch_bytes;
  if (bytes > have) {
    if (arena) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(arena)); arena = nullptr; have = 0; }
    size_t want = bytes + bytes / 4;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc((void**)&arena, want));
    have = want;
  }
  *out = arena;
  return SC_OK;
}

int tmp_buf(sc_ctx* ctx, int slot, size_t bytes, void** out) {
  auto& e = ctx->tmp[slot + (ctx->in_aux ? 1000 : 0)];       // the forked stream's calls never share a temporary with the main one's
  if (e.second < bytes) {
    if (e.first) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(e.first)); e.first = nullptr; e.second = 0; }
    size_t want = bytes + bytes / 8 + 256;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(&e.first, want));
    e.second = want;
  }
  *out = e.first;
  return SC_OK;
}

int zero_kept_flags(sc_ctx* ctx, uint64_t count, uint64_t** out) {
  auto& e = ctx->tmp[TMP_ANYFLAG + (ctx->in_aux ? 1000 : 0)];
  const size_t bytes = (size_t)count * sizeof(uint64_t);
  if (e.second < bytes) {
    if (e.first) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(e.first)); e.first = nullptr; e.second = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(&e.first, want));
    e.second = want;
    HIPCHK(ctx, hipMemsetAsync(e.first, 0, want, ctx->stream));
  }
  *out = (uint64_t*)e.first;
  return SC_OK;
}

void drop_zero_kept_flags(sc_ctx* ctx) {      // forget the accumulator: the next use allocates and clears a new one
  auto& e = ctx->tmp[TMP_ANYFLAG + (ctx->in_aux ? 1000 : 0)];
  if (e.first) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(e.first); e.first = nullptr; e.second = 0; }
}

int status_words(sc_ctx* ctx, size_t count, int** out) {
  const int s = ctx->in_aux ? 1 : 0;
  if (ctx->status_cap[s] < count) {
    if (ctx->status_host[s]) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipHostFree(ctx->status_host[s])); ctx->status_host[s] = nullptr; ctx->status_cap[s] = 0; }
    const size_t want = std::max<size_t>(count, SC_INV_TOP);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->status_host[s], want * sizeof(int), hipHostMallocMapped));
    ctx->status_cap[s] = want;
  }
  *out = ctx->status_host[s];
  return SC_OK;
}

int device_n_half(sc_ctx* ctx, const uint32_t* n_hptr, int nw, uint32_t** out) {
  std::vector<uint32_t> n(n_hptr, n_hptr + nw);
  auto it = ctx->nwords_cache.find(n);
  if (it != ctx->nwords_cache.end()) { *out = it->second; return SC_OK; }
  std::vector<uint32_t> both(2 * nw);
  for (int k = 0; k < nw; k++) { both[k] = n[k]; both[nw + k] = (n[k] >> 1) | ((k + 1 < nw) ? (n[k + 1] << 31) : 0u); }
  uint32_t* d = nullptr;
  int rc = upload(ctx, both.data(), both.size() * 4, (void**)&d);
  if (rc) return rc;
  ctx->nwords_cache[n] = d;
  *out = d;
  return SC_OK;
}

int get_pair_consts(sc_ctx* ctx, int mod, uint32_t** out) {
  auto it = ctx->pair_consts.find(mod);
  if (it != ctx->pair_consts.end()) { *out = it->second; return SC_OK; }
  const Mod& m = ctx->mods[mod];
  Big m2 = big_mul(m.n, m.n);
  Big one(m2.size(), 0); one[0] = 1;
  Big r2 = big_shl_mod(one, m2, 2 * m.W * m.S);                       // R^2 mod m^2
  Big br = big_shl_mod(one, m2, m.W * m.S + 32 * m.nwords);           // B R mod m^2
  std::vector<uint32_t> limbs;
  for (const Big* v : {&r2, &br}) {
    Big q, rem;
    big_divmod(*v, m.n, &q, &rem);
    q.resize(m.nwords);
    for (const Big* part : {&rem, &q}) { auto l = to_limbs(*part, m.S, m.W); limbs.insert(limbs.end(), l.begin(), l.end()); }
  }
  uint32_t* d = nullptr;
  int rc = upload(ctx, limbs.data(), limbs.size() * 4, (void**)&d);
  if (rc) return rc;
  ctx->pair_consts[mod] = d;
  *out = d;
  return SC_OK;
}

// The row of an interpreter instance in the part that compiles it, or null.
static const KernelRow* find_instance(uint32_t key) {
  for (auto part : {vm_part0, vm_part1, vm_part2, pvm_part0, pvm_part1, pvm_part2})
    if (const KernelRow* row = part(key)) return row;
  return nullptr;
}

int run_vm(sc_ctx* ctx, int mod, const Prog& p, const VmExt* exts, int next, uint64_t count, const uint32_t* fbt_rows) {
  if (count == 0) return SC_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));  // the caller may have switched the current device since sc_ctx_create
  const Mod& m = ctx->mods[mod];
  VmArgs a;
  memset(&a, 0, sizeof a);
  a.modctx = m.d_ctx;
  a.consts = p.d_consts;
  a.prog = p.d_ops;
  a.fbt = fbt_rows;
  a.count = count;
  a.n0inv = m.n0inv;
  a.nops = p.nops;
  a.nconst_extra = p.nconst;
  a.nscratch = p.nscratch;
  a.small_c = m.small_c; a.small_cinv = m.small_cinv;
  for (int i = 0; i < next; i++) a.ext[i] = exts[i];
  // multiply-adds issued per item: a product or a reduction pass is S^2 (S/G limb steps x L per lane x G lanes); the a*a part
  // of a squaring is L(L+1)/2 per (lane, block) pair, G^2 pairs
  const Instance k = vm_instance(shape_of(m), policy_of(ctx), count);
  ctx->mac_counter += (double)count * ((p.muls_per_item * 2.0 + p.redcs_per_item + p.sqrs_per_item) * (double)m.S * m.S +
                                        p.sqrs_per_item * (double)k.G * k.G * k.L * (k.L + 1) / 2.0);
  const KernelRow* row = find_instance(launch_key(false, k.G, k.L, k.W, k.neg1, false, false));
  if (!row) return fail(ctx, SC_ERR_UNSUPPORTED, "no kernel configuration for G=%d L=%d", k.G, k.L);
  return row->launch(ctx, a);
}

int pvm_occupancy(sc_ctx* ctx, int G, int L, bool neg1) {
  const KernelRow* row = find_instance(launch_key(true, G, L, kPairW, neg1, false, false));
  return row ? row->occupancy(ctx) : -1;
}

int run_pvm(sc_ctx* ctx, int mod, const Prog& p, const VmExt* exts, int next, uint64_t count) {
  if (count == 0) return SC_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Mod& m = ctx->mods[mod];
  VmArgs a;
  memset(&a, 0, sizeof a);
  a.modctx = m.d_ctx; a.consts = p.d_consts; a.prog = p.d_ops; a.count = count; a.n0inv = m.n0inv;
  a.nops = p.nops; a.nconst_extra = p.nconst; a.nscratch = p.nscratch;
  for (int i = 0; i < next; i++) a.ext[i] = exts[i];
  ctx->mac_counter += (double)count * p.muls_per_item;   // pair programs carry their exact multiply-add count here
  if (!pair_capable(m.G, m.L, m.W)) return fail(ctx, SC_ERR_UNSUPPORTED, "no pair kernel for G=%d L=%d", m.G, m.L);
  if (p.pair_dig) {      // per-row exponents: the modulus's own instance with PV_MULTDIG (no latency / n = -1 variants of it exist)
    const KernelRow* row = find_instance(launch_key(true, m.G, m.L, kPairW, false, false, true));
    if (!row) return fail(ctx, SC_ERR_UNSUPPORTED, "no per-row-exponent pair kernel for G=%d L=%d", m.G, m.L);
    return row->launch(ctx, a);
  }
  const Instance k = pvm_instance(shape_of(m), policy_of(ctx), count);
  const bool stamp = k.neg1 && k.G == 4 && k.L == 18 && ctx->stamps != nullptr;     // the stamping twin of (4,18,neg1) is sc_clock_probe's diagnostic launch
  const KernelRow* row = find_instance(launch_key(true, k.G, k.L, kPairW, k.neg1, stamp, false));
  if (!row) return fail(ctx, SC_ERR_UNSUPPORTED, "no pair kernel for G=%d L=%d", k.G, k.L);
  return row->launch(ctx, a);
}

void emit_load_reduced(sc_ctx* ctx, const Mod& m, Builder& b, int ext, int x_words, int kred_lds) {
  const int cw = m.nwords;
  const int nch = (x_words + cw - 1) / cw;
  for (int t = nch - 1; t >= 0; t--) {
    const int nw = std::min(cw, x_words - t * cw);
    if (t == nch - 1) {
      b.loadw(ext, 0, t * cw, nw);
    } else {
      b.mul_const(kred_lds);          // ACC *= 2^(32 cw)   (kred is Montgomery form of that power)
      b.addw(ext, 0, t * cw, nw);
    }
  }
  (void)ctx;
}

int best_window(int bits) {
  int best = 1; double bc = 1e30;
  for (int w = 1; w <= 6; w++) {
    double c = (double)(1 << (w - 1)) + (double)bits / (w + 1);
    if (c < bc) { bc = c; best = w; }
  }
  return best;
}
void emit_pow_shared(Builder& b, const Exp& ex) {
  if (ex.bits == 0) b.loadt_const(1);
  else emit_window_pow(b, ex, 0);
}

}  // namespace sc_host

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int sc_abi_version(void) { return SC_ABI_VERSION; }

int sc_ctx_create(int device_id, sc_ctx** out_ctx) {
  if (!out_ctx) return SC_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return SC_ERR_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return SC_ERR_HIP;
  sc_ctx* c = new sc_ctx();
  c->device = device_id;
  // developer switches, read per context: SC_PAIR_HOLD_MS (target hold time of a resident wave of a long pair launch on a shared chip;
  // 0 = never cut such launches), SC_PAIR_SEGMENTS=1 (the same "never", kept from round 4)
  if (const char* e = getenv("SC_PAIR_HOLD_MS")) c->pair_hold_ms = std::max(0.0, atof(e));
  if (const char* e = getenv("SC_PAIR_SEGMENTS")) if (atoi(e) == 1) c->pair_hold_ms = 0.0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->num_cu = prop.multiProcessorCount;
  *out_ctx = c;
  return SC_OK;
}

void sc_ctx_destroy(sc_ctx* ctx) {
  if (!ctx) return;
  // teardown: errors are not reportable any more, results deliberately ignored
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (void* p : ctx->owned) (void)hipFree(p);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->scratch_aux) (void)hipFree(ctx->scratch_aux);
  if (ctx->aux_fork) (void)hipEventDestroy(ctx->aux_fork);
  if (ctx->aux_join) (void)hipEventDestroy(ctx->aux_join);
  if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
  for (auto& kv : ctx->tmp) if (kv.second.first) (void)hipFree(kv.second.first);
  for (auto& kv : ctx->reduce_consts) { (void)hipFree(kv.second.first); (void)hipHostFree(kv.second.second); }
  for (int* h : ctx->status_host) if (h) (void)hipHostFree(h);
  if (ctx->lin_host) (void)hipHostFree(ctx->lin_host);
  if (ctx->lin_copied) (void)hipEventDestroy(ctx->lin_copied);
  if (ctx->switch_event) (void)hipEventDestroy(ctx->switch_event);
  if (ctx->comm) (void)sc_comm_destroy(ctx);
  if (ctx->scheme_keys) free_scheme_keys(ctx->scheme_keys);
  memset(&ctx->rng_key, 0, sizeof ctx->rng_key);            // the generator's key does not outlive the context
  delete ctx;
}

int sc_ctx_set_latency_mode(sc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return SC_ERR_ARG;
  ctx->latency_mode = mode;
  return SC_OK;
}
// The context reuses its scratch arena, temporaries and parked tables from call to call, so work queued on the previous stream
// must be ordered before anything the next stream does with them: an event recorded on the old stream, waited for on the new.
int sc_ctx_set_stream(sc_ctx* ctx, void* hip_stream) {
  if (!ctx) return SC_ERR_ARG;
  hipStream_t s = (hipStream_t)hip_stream;
  if (s == ctx->stream) return SC_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (!ctx->switch_event) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->switch_event, hipEventDisableTiming));
  if (hipEventRecord(ctx->switch_event, ctx->stream) == hipSuccess) {
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->switch_event, 0));
  } else {
    (void)hipGetLastError();                       // the previous stream no longer exists: its work was completed when it was destroyed
  }
  ctx->stream = s;
  return SC_OK;
}
// (a division by zero met by an earlier sc_plain_divmod of this context is reported here: include/sc_amd_dev.h)
int sc_ctx_synchronize(sc_ctx* ctx) { if (!ctx) return SC_ERR_ARG; HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return div_verdict_check(ctx); }
const char* sc_last_error(sc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int64_t sc_last_bad_index(sc_ctx* ctx) { return ctx ? ctx->last_bad_index : -1; }

int sc_malloc(sc_ctx* ctx, size_t bytes, void** out_dptr) {
  if (!ctx || !out_dptr) return SC_ERR_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc(out_dptr, bytes ? bytes : 4));
  return SC_OK;
}
int sc_free(sc_ctx* ctx, void* dptr) { if (!ctx) return SC_ERR_ARG; HIPCHK(ctx, hipFree(dptr)); return SC_OK; }
int sc_memcpy_h2d(sc_ctx* ctx, void* dptr, const void* hptr, size_t bytes) {
  if (!ctx) return SC_ERR_ARG;
  HIPCHK(ctx, hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}
int sc_memcpy_d2h(sc_ctx* ctx, void* hptr, const void* dptr, size_t bytes) {
  if (!ctx) return SC_ERR_ARG;
  HIPCHK(ctx, hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

int sc_mod_create(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, int* out_mod) {
  return create_mod(ctx, n_hptr, nwords, false, out_mod);
}

int sc_mod_words(sc_ctx* ctx, int mod) { return valid_mod(ctx, mod) ? ctx->mods[mod].nwords : SC_ERR_ARG; }

int sc_exp_create(sc_ctx* ctx, const uint32_t* e_hptr, int ewords, int* out_exp) {
  if (!ctx || !e_hptr || ewords <= 0 || !out_exp) return fail(ctx, SC_ERR_ARG, "sc_exp_create: bad argument");
  Exp e; e.e.assign(e_hptr, e_hptr + ewords); e.bits = big_bits(e.e);
  ctx->exps.push_back(e);
  *out_exp = (int)ctx->exps.size() - 1;
  return SC_OK;
}

int sc_const_create(sc_ctx* ctx, int mod, const uint32_t* v_hptr, int nwords, int* out_const) {
  if (!valid_mod(ctx, mod) || !v_hptr || !out_const) return fail(ctx, SC_ERR_ARG, "sc_const_create: bad argument");
  const Mod& m = ctx->mods[mod];
  Big v(v_hptr, v_hptr + nwords);
  v.resize(std::max(nwords, m.nwords), 0);
  Big nn = m.n; nn.resize(v.size(), 0);
  Big vm = big_shl_mod(v, nn, m.W * m.S);  // Montgomery form
  auto l = to_limbs(vm, m.S, m.W);
  Const c; c.mod = mod;
  int rc = upload(ctx, l.data(), l.size() * 4, (void**)&c.d_limbs);
  if (rc) return rc;
  ctx->consts.push_back(c);
  *out_const = (int)ctx->consts.size() - 1;
  return SC_OK;
}

}  // extern "C"

namespace sc_host {
int create_mod(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, bool for_pairs, int* out_mod, const Config* forced) {
  if (!ctx || !n_hptr || nwords <= 0 || !out_mod) return fail(ctx, SC_ERR_ARG, "sc_mod_create: bad argument");
  Mod m;
  m.n.assign(n_hptr, n_hptr + nwords);
  m.nwords = nwords;
  m.nbits = big_bits(m.n);
  if (m.nbits < 2 || !(m.n[0] & 1)) return fail(ctx, SC_ERR_ARG, "sc_mod_create: modulus must be odd and > 1");
  const Config* cfg = forced ? forced_fit(*forced, m.nbits) : first_fit(m.nbits, nwords, for_pairs);
  if (cfg) { m.G = cfg->G; m.L = cfg->L; m.W = cfg->W; }
  if (!m.G) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_mod_create: %d-bit modulus exceeds the largest configuration", m.nbits);
  m.S = m.G * m.L;
  const int W = m.W;
  const uint32_t LMASK = (1u << W) - 1;
  // the residue arrays must be representable below R = 2^(W S)
  if (32 * nwords > W * m.S + 31) return fail(ctx, SC_ERR_ARG, "sc_mod_create: nwords=%d too wide for a %d-bit modulus", nwords, m.nbits);
  // n0inv = -n^-1 mod 2^W (Newton)
  uint32_t n0 = m.n[0], inv = 1;
  for (int i = 0; i < 6; i++) inv *= 2 - n0 * inv;
  m.n0inv = (0u - inv) & LMASK;
  Big one(nwords, 0); one[0] = 1;
  Big r1 = big_shl_mod(one, m.n, W * m.S);
  Big r2 = big_shl_mod(r1, m.n, W * m.S);
  std::vector<uint32_t> ctxv;
  auto app = [&](const Big& x) { auto l = to_limbs(x, m.S, W); ctxv.insert(ctxv.end(), l.begin(), l.end()); };
  app(m.n); app(r2); app(r1);
  int rc = upload(ctx, ctxv.data(), ctxv.size() * 4, (void**)&m.d_ctx);
  if (rc) return rc;
  ctx->mods.push_back(m);
  *out_mod = (int)ctx->mods.size() - 1;
  return SC_OK;
}

int sc_const_create_cached(sc_ctx* ctx, int mod, const Big& v, int* out_cid) {
  auto key = std::make_pair(mod, v);
  auto it = ctx->const_by_value.find(key);
  if (it != ctx->const_by_value.end()) { *out_cid = it->second; return SC_OK; }
  int cid;
  int rc = sc_const_create(ctx, mod, v.data(), (int)v.size(), &cid);
  if (rc) return rc;
  ctx->const_by_value[key] = cid;
  *out_cid = cid;
  return SC_OK;
}
int get_const_kred(sc_ctx* ctx, int mod, int* out_cid) {
  const Mod& m = ctx->mods[mod];
  auto it = ctx->kred_cache.find(mod);
  if (it != ctx->kred_cache.end()) { *out_cid = it->second; return SC_OK; }
  Big one(m.nwords, 0); one[0] = 1;
  Big v = big_shl_mod(one, m.n, 32 * m.nwords);
  int cid;
  int rc = sc_const_create(ctx, mod, v.data(), m.nwords, &cid);
  if (rc) return rc;
  ctx->kred_cache[mod] = cid;
  *out_cid = cid;
  return SC_OK;
}

int modexp_shared_impl(sc_ctx* ctx, int mod, int exp, const uint32_t* x, int x_words, const uint32_t* mul_into,
                              uint32_t* out, uint8_t* flags, uint64_t count, uint64_t* any_flags, uint64_t inner, bool any_flags_clean) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || exp < 0 || exp >= (int)ctx->exps.size() || !x || (!out && !flags && !any_flags))
    return fail(ctx, SC_ERR_ARG, "sc_modexp_shared: bad argument");
  if (any_flags) {
    if (inner == 0 || count % inner != 0) return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_isone_any: count must be a multiple of the inner count");
    if (!any_flags_clean) HIPCHK(ctx, hipMemsetAsync(any_flags, 0, inner * sizeof(uint64_t), ctx->stream));
  }
  if (ctx->exps[exp].bits > 64) mod = onelane_for(ctx, mod, count);   // long exponentiations of a chip-filling batch: one-lane twin
  const Mod& m = ctx->mods[mod];
  if (x_words <= 0) x_words = m.nwords;
  const int mode = any_flags ? 3 : (flags ? 2 : (mul_into ? 1 : 0));
  std::string key = "mexp:" + std::to_string(mod) + ":" + std::to_string(exp) + ":" + std::to_string(x_words) + ":" + std::to_string(mode);
  const Prog* p;
  int rc = cached_prog(ctx, key, mod, [&](Builder& bd) -> int {
    if (x_words > m.nwords) {
      int kc; int rc = get_const_kred(ctx, mod, &kc); if (rc) return rc;
      emit_load_reduced(ctx, m, bd, 0, x_words, bd.use_const(kc));
    } else {
      bd.loadw(0, 0, 0, x_words);
    }
    bd.mul_const(0);                   // to Montgomery form
    emit_pow_shared(bd, ctx->exps[exp]);
    if (mode == 0) { bd.redc(); bd.storew(1); }
    else if (mode == 1) { bd.mul_extw(2); bd.storew(1); }
    else bd.storeflag(1, 0, 1, mode == 3);             // compare with R mod n (Montgomery one); mode 3: OR the verdict into the item's group flag
    return SC_OK;
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(x, x_words, x_words),
                 any_flags ? mk_ext(any_flags, 0, 0, inner) : (flags ? mk_ext(flags, 0, 0) : mk_ext(out, m.nwords, m.nwords)),
                 mk_ext(mul_into, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *p, ex, 3, count);
}

int modexp_var_impl(sc_ctx* ctx, int mod, const uint32_t* x, const uint32_t* e, int ewords, int ebits, int fbt,
                           const uint32_t* e2, int e2words, const uint64_t* dest, uint32_t* out, uint64_t count,
                           const uint32_t* premul, const int64_t* perm, uint32_t planes) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || !x || !e || !out || ewords <= 0 || ebits <= 0 || ebits > 32 * ewords)
    return fail(ctx, SC_ERR_ARG, "sc_modexp_var: bad argument");
  if (perm && (dest || planes == 0 || planes > SC_MAX_L + 1 || count % planes != 0)) return fail(ctx, SC_ERR_ARG, "sc_modexp_var: bad permutation batch");
  const Fbt* f = nullptr;
  if (fbt >= 0) {
    if (fbt >= (int)ctx->fbts.size() || ctx->fbts[fbt].mod != mod || !e2 || e2words <= 0) return fail(ctx, SC_ERR_ARG, "sc_modexp_var: bad fixed-base table");
    f = &ctx->fbts[fbt];
  }
  // chip-filling batches of a (4,18) modulus run in the context of its multiple M = c n = -1 (mod 2^29) (no quotient multiply per
  // limb step): inputs, constants and table rows are residues modulo n and therefore valid modulo M as they are; the program
  // leaves through the reduction pass times c and the exact division by c (sc_device.h).  Not with premul: that variant leaves
  // Montgomery form through a product, which has no room for the factor c.
  const int tmod = premul ? -1 : neg1_vm_twin(ctx, mod, count);
  const bool twin = tmod >= 0;
  const int rmod = twin ? tmod : mod;
  const Mod& m = ctx->mods[mod];        // (taken after the twin exists: creating it may move the table of moduli)
  std::string key = "mvar:" + std::to_string(rmod) + ":" + std::to_string(ebits) + ":" + std::to_string(fbt) + (dest ? ":s" : "") + (perm ? ":q" : "") + (premul ? ":p" : "");
  const Prog* p;
  int rc = cached_prog(ctx, key, rmod, [&](Builder& bd) {
    const int w = ebits <= 4 ? 1 : (ebits <= 12 ? 2 : 3);
    const int nd = (ebits + w - 1) / w;
    bd.loadw(0); bd.mul_const(0); bd.stt(1);          // t[1] = x (Montgomery)
    bd.loadt_const(1); bd.stt(0);                      // t[0] = 1
    for (int k = 2; k < (1 << w); k++) { bd.loadt_tbl(k - 1); bd.mul_tbl(1); bd.stt(k); }
    bd.loadt_tbldig(1, (nd - 1) * w, w, 0);
    for (int d = nd - 2; d >= 0; d--) { for (int k = 0; k < w; k++) bd.sqr(); bd.mul_tbldig(1, d * w, w, 0); }
    if (f) for (int j = 0; j < f->nwin; j++) bd.mul_fbt(3, j * f->window, f->window, j);
    if (premul) bd.mul_extw(5); else bd.redc(twin);      // (x^e R) * premul / R = x^e premul: leaves Montgomery form by itself
    if (dest || perm) bd.storew_at(2, 4, twin, perm != nullptr); else bd.storew(2, 0, twin);
  }, &p); if (rc) return rc;
  // a scattered store never leaves the output array: rows >= count are dropped by the limit of the output operand
  VmExt ex[6] = {mk_ext(x, m.nwords, m.nwords), mk_ext(e, ewords, ewords), mk_ext(out, m.nwords, m.nwords, (dest || perm) ? count : ~0ull),
                 mk_ext(e2, e2words, e2words), perm ? mk_ext(perm, planes, 0, count / planes) : mk_ext(dest, 2, 2), mk_ext(premul, m.nwords, m.nwords)};
  return run_vm(ctx, rmod, *p, ex, 6, count, f ? f->d_rows : nullptr);
}

int plain_bob_impl(sc_ctx* ctx, const uint32_t* z, const uint32_t* n_hptr, int nw, int l, uint64_t count, uint64_t* beta,
                          uint64_t* dbit, uint32_t* zeta1, uint32_t* zeta2, uint8_t* bits) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!ctx || !z || !n_hptr || nw <= 0 || l <= 0 || l > SC_MAX_L || !beta || !dbit || !zeta1 || !zeta2)
    return fail(ctx, SC_ERR_ARG, "sc_plain_bob: bad argument");
  if (l >= 32 * nw) return fail(ctx, SC_ERR_ARG, "sc_plain_bob: l = %d does not fit below a modulus of %d words (l < 32 nw)", l, nw);
  uint32_t* d_n = nullptr;
  { int rc = device_n_half(ctx, n_hptr, nw, &d_n); if (rc) return rc; }
  if (launch_plain_bob(ctx->stream, z, d_n, d_n + nw, nw, l, count, beta, dbit, zeta1, zeta2, bits)) return fail(ctx, SC_ERR_HIP, "sc_plain_bob: launch failed");
  return SC_OK;
}
}  // namespace sc_host

extern "C" {

int sc_modmul(sc_ctx* ctx, int mod, const uint32_t* a, int a_stride, const uint32_t* b, int b_stride, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || !a || !b || !out) return fail(ctx, SC_ERR_ARG, "sc_modmul: bad argument");
  const Mod& m = ctx->mods[mod];
  const Prog* p;
  int rc = cached_prog(ctx, "modmul:" + std::to_string(mod), mod, [&](Builder& bd) {
    bd.loadw(0); bd.mul_const(0);      // a * R
    bd.mul_extw(1);                    // (aR) * b / R = a b
    bd.storew(2);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(a, a_stride, m.nwords), mk_ext(b, b_stride, m.nwords), mk_ext(out, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *p, ex, 3, count);
}

int sc_modmul_const(sc_ctx* ctx, int mod, const uint32_t* a, int cst, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || !a || !out || cst < 0 || cst >= (int)ctx->consts.size() || ctx->consts[cst].mod != mod)
    return fail(ctx, SC_ERR_ARG, "sc_modmul_const: bad argument");
  const Mod& m = ctx->mods[mod];
  const Prog* p;
  int rc = cached_prog(ctx, "modmulc:" + std::to_string(mod) + ":" + std::to_string(cst), mod, [&](Builder& bd) {
    int c = bd.use_const(cst);
    bd.loadw(0); bd.mul_const(c);      // a * (cR) / R = a c
    bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[2] = {mk_ext(a, m.nwords, m.nwords), mk_ext(out, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *p, ex, 2, count);
}

int sc_modmul_const_sel(sc_ctx* ctx, int mod, const uint32_t* a, int cst0, int cst1, const uint8_t* flags, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!valid_mod(ctx, mod) || !a || !flags || !out) return fail(ctx, SC_ERR_ARG, "sc_modmul_const_sel: bad argument");
  for (int c : {cst0, cst1})
    if (c != -1 && (c < 0 || c >= (int)ctx->consts.size() || ctx->consts[c].mod != mod)) return fail(ctx, SC_ERR_ARG, "sc_modmul_const_sel: bad constant");
  const Mod& m = ctx->mods[mod];
  const Prog* p;
  int rc = cached_prog(ctx, "mmsel:" + std::to_string(mod) + ":" + std::to_string(cst0) + ":" + std::to_string(cst1), mod, [&](Builder& bd) {
    const int l0 = cst0 < 0 ? 1 : bd.use_const(cst0), l1 = cst1 < 0 ? 1 : bd.use_const(cst1);   // LDS constant 1 = R mod n = the residue 1
    bd.loadw(0);
    bd.mul_constsel(2, l0, l1);        // a * (c R) / R = a c
    bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(a, m.nwords, m.nwords), mk_ext(out, m.nwords, m.nwords), mk_ext(flags, 0, 0)};
  return run_vm(ctx, mod, *p, ex, 3, count);
}

int sc_modexp_shared(sc_ctx* ctx, int mod, int exp, const uint32_t* x, int x_words, const uint32_t* mul_into, uint32_t* out, uint64_t count) {
  return modexp_shared_impl(ctx, mod, exp, x, x_words, mul_into, out, nullptr, count, nullptr, 0);
}
int sc_modexp_shared_isone(sc_ctx* ctx, int mod, int exp, const uint32_t* x, int x_words, uint8_t* flags, uint64_t count) {
  return modexp_shared_impl(ctx, mod, exp, x, x_words, nullptr, nullptr, flags, count, nullptr, 0);
}
int sc_modexp_shared_isone_any(sc_ctx* ctx, int mod, int exp, const uint32_t* x, int x_words, uint64_t inner, uint64_t* any_flags,
                               uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!any_flags) return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_isone_any: no output");
  return modexp_shared_impl(ctx, mod, exp, x, x_words, nullptr, nullptr, nullptr, count, any_flags, inner);
}

int sc_fbt_create(sc_ctx* ctx, int mod, const uint32_t* base_hptr, int exp_bits, int window, int* out_fbt) {
  if (!valid_mod(ctx, mod) || !base_hptr || exp_bits <= 0 || window < 1 || window > 24 || !out_fbt)
    return fail(ctx, SC_ERR_ARG, "sc_fbt_create: bad argument");
  const Mod& m = ctx->mods[mod];
  Fbt f; f.mod = mod; f.window = window; f.exp_bits = exp_bits; f.nwin = (exp_bits + window - 1) / window;
  const uint64_t rows = (uint64_t)f.nwin << window;
  f.rows = std::make_shared<FbtRows>();
  f.rows->device = ctx->device; f.rows->bytes = rows * m.S * 4;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc((void**)&f.rows->d, f.rows->bytes));
  f.d_rows = f.rows->d;
  int rc;
  int cbase; rc = sc_const_create(ctx, mod, base_hptr, m.nwords, &cbase); if (rc) return rc;
  // stage A: B_j = base^(2^(window j)), limb form, one item
  uint32_t* d_B; rc = dev_alloc(ctx, (size_t)f.nwin * m.S * 4, (void**)&d_B); if (rc) return rc;
  {
    Builder bd; int c = bd.use_const(cbase);
    bd.loadt_const(c); bd.storel(0, 0);
    for (int j = 1; j < f.nwin; j++) { for (int k = 0; k < window; k++) bd.sqr(); bd.storel(0, j); }
    Prog p; rc = bd.finalize(ctx, mod, &p); if (rc) return rc;
    VmExt ex[1] = {mk_ext(d_B, m.S, 0)};
    rc = run_vm(ctx, mod, p, ex, 1, 1); if (rc) return rc;
  }
  // stage B: per window, item ch computes rows d = ch, ch + NCH, ... (start B^ch, step B^NCH)
  const int lg = std::min(window, 10);
  const uint32_t NCH = 1u << lg, CH = (1u << window) / NCH;
  std::vector<uint32_t> idx(NCH); for (uint32_t i = 0; i < NCH; i++) idx[i] = i;
  uint32_t* d_idx; rc = upload(ctx, idx.data(), NCH * 4, (void**)&d_idx); if (rc) return rc;
  {
    Builder bd;
    bd.loadt_extl(0); bd.stt(1);            // t[1] = B_j
    bd.loadt_const(1); bd.stt(0);           // t[0] = one
    bd.loadt_tbl(1); for (int k = 0; k < lg; k++) bd.sqr(); bd.stt(2);   // t[2] = B_j^NCH
    bd.loadt_tbldig(1, lg - 1, 1, 0);       // B_j^ch by square-and-multiply over the bits of ch
    for (int k = lg - 2; k >= 0; k--) { bd.sqr(); bd.mul_tbldig(1, k, 1, 0); }
    bd.storel(2, 0);
    for (uint32_t i = 1; i < CH; i++) { bd.mul_tbl(2); bd.storel(2, i); }
    Prog p; rc = bd.finalize(ctx, mod, &p); if (rc) return rc;
    for (int j = 0; j < f.nwin; j++) {
      VmExt ex[3] = {mk_ext(d_B + (size_t)j * m.S, 0, 0), mk_ext(d_idx, 1, 1),
                     mk_ext(f.d_rows + ((uint64_t)j << window) * m.S, m.S, 0)};
      rc = run_vm(ctx, mod, p, ex, 3, NCH); if (rc) return rc;
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->fbts.push_back(f);
  *out_fbt = (int)ctx->fbts.size() - 1;
  return SC_OK;
}

int sc_fbt_import(sc_ctx* ctx, int mod, sc_ctx* src_ctx, int src_fbt, int* out_fbt) {
  if (!valid_mod(ctx, mod) || !src_ctx || src_fbt < 0 || src_fbt >= (int)src_ctx->fbts.size() || !out_fbt)
    return fail(ctx, SC_ERR_ARG, "sc_fbt_import: bad argument");
  const Fbt& sf = src_ctx->fbts[src_fbt];
  const Mod& sm = src_ctx->mods[sf.mod];
  const Mod& m = ctx->mods[mod];
  if (src_ctx->device != ctx->device) return fail(ctx, SC_ERR_ARG, "sc_fbt_import: the table lives on another device");
  if (sm.G != m.G || sm.L != m.L || sm.W != m.W || sm.n != m.n)
    return fail(ctx, SC_ERR_ARG, "sc_fbt_import: the table was built for another modulus");
  Fbt f = sf;            // shares the rows (reference-counted); read-only from here on
  f.mod = mod;
  ctx->fbts.push_back(f);
  *out_fbt = (int)ctx->fbts.size() - 1;
  return SC_OK;
}

int sc_fbt_bytes(sc_ctx* ctx, int fbt, uint64_t* out_bytes) {
  if (!ctx || fbt < 0 || fbt >= (int)ctx->fbts.size() || !out_bytes) return fail(ctx, SC_ERR_ARG, "sc_fbt_bytes: bad argument");
  *out_bytes = ctx->fbts[fbt].rows ? (uint64_t)ctx->fbts[fbt].rows->bytes : 0;
  return SC_OK;
}

int sc_fixedbase_pow(sc_ctx* ctx, int fbt, const uint32_t* e, int ewords, const uint32_t* mul_into, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!ctx || fbt < 0 || fbt >= (int)ctx->fbts.size() || !e || !out || ewords <= 0) return fail(ctx, SC_ERR_ARG, "sc_fixedbase_pow: bad argument");
  const Fbt& f = ctx->fbts[fbt];
  const Mod& m = ctx->mods[f.mod];
  const Prog* p;
  int rc = cached_prog(ctx, "fbp:" + std::to_string(fbt) + ":" + std::to_string(mul_into ? 1 : 0), f.mod, [&](Builder& bd) {
    bd.loadt_fbt(0, 0, f.window, 0);
    for (int j = 1; j < f.nwin; j++) bd.mul_fbt(0, j * f.window, f.window, j);
    if (mul_into) bd.mul_extw(2); else bd.redc();
    bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(e, ewords, ewords), mk_ext(out, m.nwords, m.nwords), mk_ext(mul_into, m.nwords, m.nwords)};
  return run_vm(ctx, f.mod, *p, ex, 3, count, f.d_rows);
}

int sc_modexp_var(sc_ctx* ctx, int mod, const uint32_t* x, const uint32_t* e, int ewords, int ebits, int fbt,
                  const uint32_t* e2, int e2words, uint32_t* out, uint64_t count) {
  return modexp_var_impl(ctx, mod, x, e, ewords, ebits, fbt, e2, e2words, nullptr, out, count);
}

int sc_modexp_var_scatter(sc_ctx* ctx, int mod, const uint32_t* x, const uint32_t* e, int ewords, int ebits, int fbt,
                          const uint32_t* e2, int e2words, const uint64_t* dest_index, uint32_t* out, uint64_t count) {
  if (ctx && count != 0 && !dest_index) return fail(ctx, SC_ERR_ARG, "sc_modexp_var_scatter: no destination index");
  return modexp_var_impl(ctx, mod, x, e, ewords, ebits, fbt, e2, e2words, dest_index, out, count);
}

static int paillier_encrypt_raw_impl(sc_ctx* ctx, int mod_n2, int cst_n, const uint32_t* mwords, int m_words, uint32_t* out, uint64_t count, bool negate) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod_n2) || cst_n < 0 || cst_n >= (int)ctx->consts.size() || ctx->consts[cst_n].mod != mod_n2 || !mwords || !out || m_words <= 0)
    return fail(ctx, SC_ERR_ARG, "sc_paillier_encrypt_raw: bad argument");
  const Mod& m = ctx->mods[mod_n2];
  if (m_words > m.nwords) return fail(ctx, SC_ERR_ARG, "sc_paillier_encrypt_raw: plaintext wider than N^2");
  std::string key = std::string(negate ? "pencn:" : "penc:") + std::to_string(mod_n2) + ":" + std::to_string(cst_n) + ":" + std::to_string(m_words);
  const Prog* p;
  int rc = cached_prog(ctx, key, mod_n2, [&](Builder& bd) {
    int c = bd.use_const(cst_n);
    bd.loadw(0, 0, 0, m_words); bd.mul_const(c);   // m * (N R) / R = m N  (mod N^2)
    if (negate) bd.neg();                          // -m N: the inverse ciphertext (1 + mN)^-1 = 1 - mN (mod N^2)
    bd.add1(); bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[2] = {mk_ext(mwords, m_words, m_words), mk_ext(out, m.nwords, m.nwords)};
  return run_vm(ctx, mod_n2, *p, ex, 2, count);
}

int sc_paillier_encrypt_raw(sc_ctx* ctx, int mod_n2, int cst_n, const uint32_t* mwords, int m_words, uint32_t* out, uint64_t count) {
  return paillier_encrypt_raw_impl(ctx, mod_n2, cst_n, mwords, m_words, out, count, false);
}
int sc_paillier_encrypt_raw_neg(sc_ctx* ctx, int mod_n2, int cst_n, const uint32_t* mwords, int m_words, uint32_t* out, uint64_t count) {
  return paillier_encrypt_raw_impl(ctx, mod_n2, cst_n, mwords, m_words, out, count, true);
}

int sc_paillier_l_mul(sc_ctx* ctx, int mod, int cst_k, const uint32_t* x, int x_words, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || cst_k < 0 || cst_k >= (int)ctx->consts.size() || ctx->consts[cst_k].mod != mod || !x || !out || x_words <= 0)
    return fail(ctx, SC_ERR_ARG, "sc_paillier_l_mul: bad argument");
  const Mod& m = ctx->mods[mod];
  const Prog* p;
  int rc = cached_prog(ctx, "plmul:" + std::to_string(mod) + ":" + std::to_string(cst_k) + ":" + std::to_string(x_words), mod, [&](Builder& bd) {
    int c = bd.use_const(cst_k);
    const int lw = std::min(x_words, (m.W * m.S + 31) / 32);   // only x mod R matters for the exact quotient
    bd.loadw(0, 0, 0, lw);
    bd.sub1();                        // y = (x - 1) mod R, exact limbs
    bd.quot();                        // y / n  (< n because x < n^2)
    bd.mul_const(c);                  // * k
    bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[2] = {mk_ext(x, x_words, x_words), mk_ext(out, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *p, ex, 2, count);
}

int sc_plain_alice(sc_ctx* ctx, const uint32_t* r, const uint32_t* n_hptr, int nw, int l, uint64_t count, uint32_t* m1,
                   uint64_t* alpha, uint64_t* alpha_tilde, uint64_t* rsmall, uint32_t* rshift) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!ctx || !r || !n_hptr || nw <= 0 || l <= 0 || l > SC_MAX_L || !m1 || !alpha || !alpha_tilde || !rsmall || !rshift)
    return fail(ctx, SC_ERR_ARG, "sc_plain_alice: bad argument");
  // m1 = 2^l + r must fit nw + 1 words (the kernel adds 2^l into word l / 32 <= nw), and the protocol needs l + 2 < bits(N) anyway
  if (l >= 32 * nw) return fail(ctx, SC_ERR_ARG, "sc_plain_alice: l = %d does not fit below a modulus of %d words (l < 32 nw)", l, nw);
  uint32_t* d_n = nullptr;
  { int rc = device_n_half(ctx, n_hptr, nw, &d_n); if (rc) return rc; }
  if (launch_plain_alice(ctx->stream, r, d_n, d_n + nw, nw, l, count, m1, alpha, alpha_tilde, rsmall, rshift)) return fail(ctx, SC_ERR_HIP, "sc_plain_alice: launch failed");
  return SC_OK;
}

int sc_plain_bob(sc_ctx* ctx, const uint32_t* z, const uint32_t* n_hptr, int nw, int l, uint64_t count, uint64_t* beta,
                 uint64_t* dbit, uint32_t* zeta1, uint32_t* zeta2) {
  return plain_bob_impl(ctx, z, n_hptr, nw, l, count, beta, dbit, zeta1, zeta2, nullptr);
}

// ------------------------------------------------------------------------------------------------
// batch inversion: Montgomery's trick over strided chunks + on-device binary extended GCD at the top
// ------------------------------------------------------------------------------------------------
// One level of the tree, kept for the error path: its operand array, chunk length and chunk count
struct InvLevel { const uint32_t* x; uint64_t count; uint32_t K; uint64_t C; };
struct InvPending { std::vector<InvLevel> levels; int* d_status = nullptr; uint64_t top_count = 0; };

// Queues every launch of the inversion (up-sweeps, the division-step kernel at the top, down-sweeps) WITHOUT waiting for the top
// kernel's verdict: the host reads the status words once, after everything is in the stream (sc_modinv), so the GPU never idles
// on a host round trip in the middle of the tree.  A non-invertible element makes the results garbage; the caller reports it.
static int modinv_rec(sc_ctx* ctx, int mod, const uint32_t* x, uint32_t* out, uint64_t count, InvPending* pend, int depth) {
  const Mod& m = ctx->mods[mod];
  // residues inverted directly by the division-step kernel (one wave each, all of them resident at once: a few thousand cost
  // the latency of one); below that the tree's levels -- two latency-bound launches each -- cost more than they save
  const uint64_t TOP = SC_INV_TOP;
  if (count <= TOP) {
    int* d_status;
    { int rc0 = status_words(ctx, count, &d_status); if (rc0) return rc0; }
    uint32_t* d_nw = nullptr;
    { int rc0 = device_n_half(ctx, m.n.data(), m.nwords, &d_nw); if (rc0) return rc0; }
    int rc = launch_xgcd(ctx->stream, x, out, d_nw, m.nwords, count, d_status);
    if (rc != 0) return fail(ctx, SC_ERR_HIP, "xgcd launch failed");
    pend->d_status = d_status;
    pend->top_count = count;
    return SC_OK;
  }
  // Chunk length: a chunk is one sequential chain of 3 (K - 1) products, so the tree's latency is the sum of the chunk lengths
  // over its levels while its work (3 products per element) does not depend on K.  Take the shortest chunks that still fill
  // every resident group slot of the chip at this level (large batches: up to 24), and never fewer than 4 (fewer, wider levels).
  const uint64_t resident_groups = (uint64_t)ctx->num_cu * 8 * (64 / m.G);
  const uint32_t K = (uint32_t)std::min<uint64_t>(24, std::max<uint64_t>(4, (count + resident_groups - 1) / resident_groups));
  const uint64_t C = (count + K - 1) / K;
  uint32_t *d_P = nullptr, *d_tot = nullptr, *d_totinv = nullptr;
  { int rc0 = tmp_buf(ctx, TMP_INV_BASE + 2 * depth, (size_t)K * C * m.S * 4, (void**)&d_P); if (rc0) return rc0; }
  { int rc0 = tmp_buf(ctx, TMP_INV_BASE + 2 * depth + 1, (size_t)C * m.nwords * 4 * 2, (void**)&d_tot); if (rc0) return rc0; }
  d_totinv = d_tot + (size_t)C * m.nwords;
  // No operand is converted to Montgomery form and no result reduced out of it: the prefix products simply drift by one factor
  // 1/R per product,  Q_i = x_0 .. x_i / R^i  (Q_0 = x_0), the chunk total Q_{K-1} goes up the tree as it is (a residue like any
  // other), and its inverse u_{K-1} = (x_0 .. x_{K-1})^-1 R^(K-1) comes back carrying exactly the powers of R that the way down
  // divides out again:   x_i^-1 = u_i Q_{i-1} / R   and   u_{i-1} = u_i x_i / R = (x_0 .. x_{i-1})^-1 R^(i-1),   u_0 = x_0^-1.
  // Three products per element (round 3: six -- two conversions, a reduction pass and the same three).  Elements past the end
  // of the batch read as 1 and take part like any other factor.
  const Prog *up, *down;
  int rc = cached_prog(ctx, "inv1d:" + std::to_string(mod) + ":" + std::to_string(K), mod, [&](Builder& bd) {
    for (uint32_t i = 0; i < K; i++) {
      if (i == 0) bd.loadw(0, 0); else bd.mul_extw(0, i);
      bd.storel(1, i);
    }
    bd.storew(2);
  }, &up); if (rc) return rc;
  rc = cached_prog(ctx, "inv2d:" + std::to_string(mod) + ":" + std::to_string(K), mod, [&](Builder& bd) {
    bd.loadw(3);                                           // u_{K-1}: the inverse of the chunk total
    for (uint32_t i = K - 1; i >= 1; i--) {
      bd.stt(0);
      bd.mul_extl(1, i - 1); bd.storew(4, i);              // x_i^-1 = u_i Q_{i-1} / R
      bd.loadt_tbl(0); bd.mul_extw(0, i);                  // u_{i-1} = u_i x_i / R
    }
    bd.storew(4, 0);
  }, &down); if (rc) return rc;
  pend->levels.push_back(InvLevel{x, count, K, C});
  {
    VmExt ex[3] = {mk_ext(x, m.nwords, m.nwords, count), mk_ext(d_P, m.S, 0, (uint64_t)K * C), mk_ext(d_tot, m.nwords, m.nwords)};
    rc = run_vm(ctx, mod, *up, ex, 3, C);
  }
  if (!rc) rc = modinv_rec(ctx, mod, d_tot, d_totinv, C, pend, depth + 1);
  if (!rc) {
    VmExt ex[5] = {mk_ext(x, m.nwords, m.nwords, count), mk_ext(d_P, m.S, 0, (uint64_t)K * C), mk_ext(nullptr, 0, 0),
                   mk_ext(d_totinv, m.nwords, m.nwords), mk_ext(out, m.nwords, m.nwords, count)};
    rc = run_vm(ctx, mod, *down, ex, 5, C);
  }
  return rc;
}

// The product of chunk `chunk` of a level (members x[i C + chunk], i < K) is not invertible: test its members one by one with the
// division-step kernel and return the first that fails, like the reference's pow / gmpy2.invert name the operand.
static int modinv_find_member(sc_ctx* ctx, const Mod& m, const InvLevel& lv, int64_t chunk, int64_t* out_index) {
  uint64_t members = 0;
  while (members < lv.K && members * lv.C + (uint64_t)chunk < lv.count) members++;
  uint32_t* d_m = nullptr; int* d_status = nullptr; uint32_t* d_nw = nullptr;
  { int rc0 = tmp_buf(ctx, TMP_INV_MEMBERS, (size_t)members * m.nwords * 4 * 2, (void**)&d_m); if (rc0) return rc0; }
  { int rc0 = status_words(ctx, members, &d_status); if (rc0) return rc0; }
  { int rc0 = device_n_half(ctx, m.n.data(), m.nwords, &d_nw); if (rc0) return rc0; }
  HIPCHK(ctx, hipMemcpy2DAsync(d_m, (size_t)m.nwords * 4, lv.x + (size_t)chunk * m.nwords, (size_t)lv.C * m.nwords * 4,
                               (size_t)m.nwords * 4, members, hipMemcpyDeviceToDevice, ctx->stream));
  if (launch_xgcd(ctx->stream, d_m, d_m + (size_t)members * m.nwords, d_nw, m.nwords, members, d_status) != 0)
    return fail(ctx, SC_ERR_HIP, "xgcd launch failed");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const volatile int* st = d_status;                    // written by the kernel, in host memory
  for (uint64_t i = 0; i < members; i++)
    if (st[i] != 1) {
      *out_index = (int64_t)(i * lv.C + (uint64_t)chunk);
      if (st[i] == 3) {                                   // the caller's error, not a residue without an inverse
        ctx->last_bad_index = *out_index;
        return fail(ctx, SC_ERR_ARG, "sc_modinv: operand %lld is not reduced modulo n", (long long)*out_index);
      }
      return SC_OK;
    }
  return fail(ctx, SC_ERR_HIP, "sc_modinv: chunk %lld is not invertible but all of its members are", (long long)chunk);
}

int sc_modinv(sc_ctx* ctx, int mod, const uint32_t* x, uint32_t* out, uint64_t count, int64_t* bad_index) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || !x || !out) return fail(ctx, SC_ERR_ARG, "sc_modinv: bad argument");
  {
    // The down-sweeps are queued before the verdicts are read, and the error path re-reads the operands to name the bad
    // element: `out` must not overlap `x` (an in-place call would have overwritten them with garbage by then).
    const size_t bytes = (size_t)count * ctx->mods[mod].nwords * 4;
    const char *xb = (const char*)x, *ob = (const char*)out;
    if (xb < ob + bytes && ob < xb + bytes) return fail(ctx, SC_ERR_ARG, "sc_modinv: out overlaps x (in-place inversion is not supported)");
  }
  if (bad_index) *bad_index = -1;
  InvPending pend;
  int rc = modinv_rec(ctx, mod, x, out, count, &pend, 0);
  if (rc) return rc;
  // the one host round trip of the call: the verdicts of the top kernel (in pinned host memory, written by the kernel itself),
  // read after every launch has been queued
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const volatile int* st = pend.d_status;
  int64_t bad = -1;
  for (uint64_t i = 0; i < pend.top_count && bad < 0; i++) if (st[i] != 1) bad = (int64_t)i;
  if (bad < 0) return SC_OK;
  if (st[bad] == 2) return fail(ctx, SC_ERR_HIP, "sc_modinv: the inversion kernel left its proven value range (internal error)");
  if (st[bad] == 3 && pend.levels.empty()) {              // (with levels above it the top kernel sees chunk products, which are reduced)
    if (bad_index) *bad_index = bad;
    ctx->last_bad_index = bad;
    return fail(ctx, SC_ERR_ARG, "sc_modinv: operand %lld is not reduced modulo n", (long long)bad);
  }
  // error path: `bad` indexes the deepest level's chunk products; walk back up, one member test per level
  const Mod& m = ctx->mods[mod];
  for (int lv = (int)pend.levels.size() - 1; lv >= 0; lv--) {
    int64_t member = -1;
    rc = modinv_find_member(ctx, m, pend.levels[lv], bad, &member);
    if (rc) { if (bad_index && member >= 0 && lv == 0) *bad_index = member; return rc; }
    bad = member;
  }
  if (bad_index) *bad_index = bad;
  ctx->last_bad_index = bad;
  return fail(ctx, SC_ERR_NOT_INVERTIBLE, "element %lld is not invertible", (long long)bad);
}

// ------------------------------------------------------------------------------------------------
// product and running product along an axis: what sc_modprod_axis and sc_modscan_axis share (sc_axis_plan.h holds the plans)
// ------------------------------------------------------------------------------------------------
// An entry point, its kernel and what an in-place call would be: the words in which the two entries' messages differ.
struct AxisEntry { const char *name, *kernel, *in_place; };
static const AxisEntry kProdAxis = {"sc_modprod_axis", "k_prod_axis", "reduction"}, kScanAxis = {"sc_modscan_axis", "k_scan_axis", "scan"};

static int no_axis_instance(sc_ctx* ctx, const AxisEntry& e, const Mod& m) {
  return fail(ctx, SC_ERR_ARG, "%s: no %s instance for configuration (G=%d, L=%d, W=%d%s)", e.name, e.kernel, m.G, m.L, m.W, m.small_c ? ", NEG1" : "");
}

// Every refusal of the two entries, in one order and before anything is launched or allocated: context, modulus and pointers; then
// axis_verdict's; then a configuration without an instance.  out_rows: the numbers `out` holds.  *run is false where SC_OK means
// an empty array: nothing to do.
static int axis_check(sc_ctx* ctx, const AxisEntry& e, int mod, const uint32_t* x, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out,
                      uint64_t out_rows, bool* run) {
  *run = false;
  if (!valid_mod(ctx, mod) || !x || !out) return fail(ctx, SC_ERR_ARG, "%s: bad argument", e.name);
  const Mod& m = ctx->mods[mod];
  switch (axis_verdict((uint64_t)m.nwords, outer, K, inner, out_rows, (uintptr_t)x, (uintptr_t)out)) {
    case AXIS_NO_MEMBER: return fail(ctx, SC_ERR_ARG, "%s: K must be at least 1", e.name);
    case AXIS_TOO_LARGE: return fail(ctx, SC_ERR_ARG, "%s: outer * K * inner * nwords exceeds 2^40 words", e.name);
    case AXIS_EMPTY: return SC_OK;
    case AXIS_OVERLAP: return fail(ctx, SC_ERR_ARG, "%s: out overlaps x (in-place %s is not supported)", e.name, e.in_place);
    case AXIS_RUN: break;
  }
  if (m.W != 29 || m.G < 2 || m.small_c != 0) return no_axis_instance(ctx, e, m);
  *run = true;
  return SC_OK;
}

// The group slots of the chip that axis_chunk fills: 8 resident waves per CU, 64 / G groups each.
static uint64_t resident_groups(const sc_ctx* ctx, const Mod& m) { return (uint64_t)ctx->num_cu * 8 * (64 / m.G); }

// The limbs of R^e mod n for every exponent of `exps`, on the device, into out_limbs[0 .. exps.size()): sc_modprod_axis' closing factor
// R^K, sc_modscan_axis' level constants.  Each is built by square and multiply on the host, once per (modulus, e), and reaches the device by a copy on the context's
// stream out of a pinned host buffer that lives as long as the entry, so the call does not wait for the stream.  The context keeps at
// most REDUCE_CONSTS_MAX of them: a caller who sums over ever new K does not grow device memory.  Only when the table cannot take all
// that a call is missing does the call wait for the stream, to empty the table once before it builds any of them: the pointers of one
// call stay valid together.  A call asks for one exponent per level, and an array of at most 2^40 words has at most 41: a blocked level
// has K > chunk >= 2 and leaves fewer than K / 2 members to the next one.  More than the table holds is refused.
static const size_t REDUCE_CONSTS_MAX = 64;
static void free_reduce_consts(sc_ctx* ctx) {
  for (auto& kv : ctx->reduce_consts) { (void)hipFree(kv.second.first); (void)hipHostFree(kv.second.second); }
  ctx->reduce_consts.clear();
}
static int mont_power_limbs(sc_ctx* ctx, int mod, const std::vector<uint64_t>& exps, const uint32_t** out_limbs) {
  const Mod& m = ctx->mods[mod];
  if (exps.size() > REDUCE_CONSTS_MAX) return fail(ctx, SC_ERR_HIP, "%zu constants R^e in one call (internal error)", exps.size());
  size_t missing = 0;
  for (uint64_t e : exps) missing += !ctx->reduce_consts.count({mod, e});     // (an exponent given twice counts twice: emptied early, no more)
  if (missing) HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->reduce_consts.size() + missing > REDUCE_CONSTS_MAX) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    free_reduce_consts(ctx);
  }
  for (uint64_t e0 : exps) {
    auto it = ctx->reduce_consts.find({mod, e0});
    if (it == ctx->reduce_consts.end()) {
      Big one(m.nwords, 0); one[0] = 1;
      const Big v = big_powmod(big_shl_mod(one, m.n, m.W * m.S), Big{(uint32_t)e0, (uint32_t)(e0 >> 32)}, m.n);
      const std::vector<uint32_t> limbs = to_limbs(v, m.S, m.W);
      const size_t bytes = limbs.size() * 4;
      uint32_t *d = nullptr, *h = nullptr;
      HIPCHK(ctx, hipMalloc((void**)&d, bytes));
      if (hipHostMalloc((void**)&h, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipFree(d); return fail(ctx, SC_ERR_HIP, "sc_modprod_axis: hipHostMalloc failed"); }
      memcpy(h, limbs.data(), bytes);
      it = ctx->reduce_consts.emplace(std::make_pair(mod, e0), std::make_pair(d, h)).first;
      HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    *out_limbs++ = it->second.first;
  }
  return SC_OK;
}

int sc_ctx_set_reduce_chunk(sc_ctx* ctx, int c) {
  if (!ctx || (c != 0 && (c < 2 || c > 32))) return SC_ERR_ARG;
  ctx->reduce_chunk = c;
  return SC_OK;
}

// product along an axis: a tree of k_prod_axis levels (sc_launch_reduce.hip)
int sc_modprod_axis(sc_ctx* ctx, int mod, const uint32_t* x, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out) {
  bool run;
  { int rc = axis_check(ctx, kProdAxis, mod, x, outer, K, inner, out, outer * inner, &run); if (rc || !run) return rc; }
  const Mod& m = ctx->mods[mod];
  const std::vector<ReduceLevel> plan = reduce_plan(outer, K, inner, resident_groups(ctx, m), ctx->reduce_chunk);
  // partials: level v writes outer * nch_v * inner numbers in limb form; levels alternate between the two halves of one temporary
  // (sizes shrink from level to level, so the first two decide)
  uint32_t* half[2] = {nullptr, nullptr};
  if (plan.size() > 1) {
    const size_t n0 = (size_t)outer * plan[0].nch * inner, n1 = plan.size() > 2 ? (size_t)outer * plan[1].nch * inner : 0;
    int rc = tmp_buf(ctx, TMP_REDUCE, (n0 + n1) * m.S * 4, (void**)&half[0]); if (rc) return rc;
    half[1] = half[0] + n0 * m.S;
  }
  const uint32_t* fin = nullptr;                     // the closing factor R^K
  { int rc = mont_power_limbs(ctx, mod, {K}, &fin); if (rc) return rc; }
  const uint32_t* src = x;
  for (size_t v = 0; v < plan.size(); v++) {
    const ReduceLevel& lv = plan[v];
    const bool final = v + 1 == plan.size();
    uint32_t* dst = final ? out : half[v & 1];
    int rc = launch_prod_axis(ctx, m.G, m.L, m.W, m.d_ctx, m.n0inv, fin, src, dst, lv.K, inner, lv.chunk, lv.nch, outer * lv.nch * inner, m.nwords,
                              v == 0, final);
    if (rc == SC_ERR_UNSUPPORTED) return no_axis_instance(ctx, kProdAxis, m);
    if (rc) return rc;
    // one product per member past the first of a chain; the last level's product with the closing factor
    ctx->mac_counter += (double)m.S * m.S * 2.0 * (double)outer * (double)inner * ((double)(lv.K - lv.nch) + (final ? 1.0 : 0.0));
    src = dst;
  }
  return SC_OK;
}

// running product along an axis: reduce-then-scan over k_prod_axis and k_scan_axis (sc_launch_scan.hip)
int sc_modscan_axis(sc_ctx* ctx, int mod, const uint32_t* x, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out) {
  bool run;
  { int rc = axis_check(ctx, kScanAxis, mod, x, outer, K, inner, out, outer * K * inner, &run); if (rc || !run) return rc; }
  const Mod& m = ctx->mods[mod];
  const std::vector<ScanLevel> plan = scan_plan(outer, K, inner, resident_groups(ctx, m), ctx->reduce_chunk);
  const size_t D = plan.size() - 1;                  // blocked levels
  // level v < D keeps, in one temporary, the totals of its full chunks (limb form) and their prefixes (word form), outer * K_(v+1) * inner each
  std::vector<uint32_t*> totals(D, nullptr), prefix(D, nullptr);
  if (D) {
    size_t need = 0;
    for (size_t v = 0; v < D; v++) need += (size_t)outer * plan[v + 1].K * inner * ((size_t)m.S + m.nwords);
    uint32_t* buf = nullptr;
    int rc = tmp_buf(ctx, TMP_SCAN, need * 4, (void**)&buf); if (rc) return rc;
    for (size_t v = 0; v < D; v++) {
      const size_t cnt = (size_t)outer * plan[v + 1].K * inner;
      totals[v] = buf; buf += cnt * m.S;
      prefix[v] = buf; buf += cnt * m.nwords;
    }
  }
  // the level constants R^(members + 1), all from one fetch
  std::vector<uint64_t> exps;
  for (const ScanLevel& lv : plan) exps.push_back(lv.members + 1);
  std::vector<const uint32_t*> lift(plan.size(), nullptr);
  { int rc = mont_power_limbs(ctx, mod, exps, lift.data()); if (rc) return rc; }
  // k_prod_axis stages S limbs of `fin` at every level and multiplies by them at a final one only: the totals' levels, none of them
  // final, get S limbs that exist
  const uint32_t* const unused_fin = lift[0];
  // down: the totals of every blocked level's full chunks, one product per member past the first of a chunk
  for (size_t v = 0; v < D; v++) {
    const ScanLevel& lv = plan[v];
    const uint32_t* src = v == 0 ? x : totals[v - 1];
    int rc = launch_prod_axis(ctx, m.G, m.L, m.W, m.d_ctx, m.n0inv, unused_fin, src, totals[v], lv.K, inner, (uint32_t)lv.chunk, lv.nch - 1, outer * (lv.nch - 1) * inner,
                              m.nwords, v == 0, false);
    if (rc == SC_ERR_UNSUPPORTED) return no_axis_instance(ctx, kScanAxis, m);
    if (rc) return rc;
    ctx->mac_counter += (double)m.S * m.S * 2.0 * (double)outer * (double)inner * (double)(lv.nch - 1) * (double)(lv.chunk - 1);
  }
  // up: the direct scan of the deepest level, then every blocked level seeded with the prefixes of the level below it
  for (size_t v = D + 1; v-- > 0;) {
    const ScanLevel& lv = plan[v];
    const uint32_t* src = v == 0 ? x : totals[v - 1];
    uint32_t* dst = v == 0 ? out : prefix[v - 1];
    int rc = launch_scan_axis(ctx, m.G, m.L, m.W, m.d_ctx, m.n0inv, lift[v], src, lv.blocked ? prefix[v] : nullptr, dst, lv.K, inner, lv.chunk, lv.nch,
                              outer * lv.nch * inner, m.nwords, v == 0);
    if (rc == SC_ERR_UNSUPPORTED) return no_axis_instance(ctx, kScanAxis, m);
    if (rc) return rc;
    ctx->mac_counter += (double)m.S * m.S * 2.0 * 2.0 * (double)outer * (double)inner * (double)lv.K;
  }
  return SC_OK;
}

// linear maps with public weights along an axis: one k_lin_lift and one k_lin_axis launch (sc_launch_lin.hip)
static const AxisEntry kLinAxis = {"sc_modlin_axis", "k_lin_axis", "linear map"};
static const uint64_t LIN_MAX = 1024;     // K and J of one call

int sc_modlin_axis(sc_ctx* ctx, int mod, const uint32_t* x, uint64_t outer, uint64_t K, uint64_t inner, const uint64_t* w_host, uint64_t J, uint32_t* out) {
  if (!valid_mod(ctx, mod) || !x || !out || !w_host) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: bad argument");
  if (outer == 0) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: outer must be at least 1");
  if (inner == 0) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: inner must be at least 1");
  if (J == 0) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: J must be at least 1");
  if (K > LIN_MAX) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: K = %llu exceeds %llu", (unsigned long long)K, (unsigned long long)LIN_MAX);
  if (J > LIN_MAX) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: J = %llu exceeds %llu", (unsigned long long)J, (unsigned long long)LIN_MAX);
  {                                          // the output's size: outer * J * inner * nwords <= 2^40 words, factor by factor (the input's: axis_check)
    uint64_t words = (uint64_t)ctx->mods[mod].nwords * J;
    for (uint64_t f : {outer, inner}) {
      if (words > (1ull << 40) / f) return fail(ctx, SC_ERR_ARG, "sc_modlin_axis: outer * J * inner * nwords exceeds 2^40 words");
      words *= f;
    }
  }
  bool run;
  { int rc = axis_check(ctx, kLinAxis, mod, x, outer, K, inner, out, outer * J * inner, &run); if (rc || !run) return rc; }
  const Mod& m = ctx->mods[mod];
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // one grow-only temporary: the lifted members [outer][K][inner][S], the weights [J][K] (64 bits each, 8-byte aligned), rowbits [J]
  const size_t members = (size_t)outer * K * inner, lift_words = (members * m.S + 1) & ~(size_t)1, w_bytes = (size_t)J * K * 8, rb_bytes = (size_t)J * 4;
  uint32_t* buf = nullptr;
  { int rc = tmp_buf(ctx, TMP_LIN, lift_words * 4 + w_bytes + rb_bytes, (void**)&buf); if (rc) return rc; }
  uint32_t* const d_lift = buf;
  uint64_t* const d_w = (uint64_t*)(buf + lift_words);
  uint32_t* const d_rb = (uint32_t*)(d_w + J * K);
  // The weights leave through a pinned buffer of the context, so that the copy is queued on the stream and the caller's array is free on
  // return; the buffer is written again only after the previous call's copy has left it.
  if (ctx->lin_copied) HIPCHK(ctx, hipEventSynchronize(ctx->lin_copied));
  else HIPCHK(ctx, hipEventCreateWithFlags(&ctx->lin_copied, hipEventDisableTiming));
  if (ctx->lin_host_bytes < w_bytes + rb_bytes) {
    if (ctx->lin_host) { HIPCHK(ctx, hipHostFree(ctx->lin_host)); ctx->lin_host = nullptr; ctx->lin_host_bytes = 0; }
    const size_t want = w_bytes + rb_bytes + (w_bytes + rb_bytes) / 8 + 256;
    HIPCHK(ctx, hipHostMalloc(&ctx->lin_host, want, hipHostMallocDefault));
    ctx->lin_host_bytes = want;
  }
  uint64_t* const h_w = (uint64_t*)ctx->lin_host;
  uint32_t* const h_rb = (uint32_t*)(h_w + J * K);
  memcpy(h_w, w_host, w_bytes);
  double sqrs = 0, muls = 0;                 // per (o, i): what the chains of the J rows cost
  for (uint64_t j = 0; j < J; j++) {
    uint64_t top = 0;
    for (uint64_t k = 0; k < K; k++) { top |= w_host[j * K + k]; muls += __builtin_popcountll(w_host[j * K + k]); }
    h_rb[j] = top ? 64u - (uint32_t)__builtin_clzll(top) : 0u;
    sqrs += h_rb[j] ? h_rb[j] - 1 : 0;
  }
  HIPCHK(ctx, hipMemcpyAsync(d_w, h_w, w_bytes + rb_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->lin_copied, ctx->stream));
  int rc = launch_lin_lift(ctx, m.G, m.L, m.W, m.d_ctx, m.n0inv, x, d_lift, members, m.nwords);
  if (rc == SC_ERR_UNSUPPORTED) return no_axis_instance(ctx, kLinAxis, m);
  if (rc) return rc;
  rc = launch_lin_axis(ctx, m.G, m.L, m.W, m.d_ctx, m.n0inv, d_lift, d_w, d_rb, out, outer, K, inner, J, m.nwords);
  if (rc == SC_ERR_UNSUPPORTED) return no_axis_instance(ctx, kLinAxis, m);
  if (rc) return rc;
  // one product per member (the lift); per output its squarings (half the multiply-adds of a product's a * b part), its products and the
  // closing reduction pass
  const double S2 = (double)m.S * m.S, pairs = (double)outer * (double)inner;
  ctx->mac_counter += S2 * 2.0 * (double)members + pairs * S2 * (1.5 * sqrs + 2.0 * muls + 1.0 * (double)J);
  return SC_OK;
}

int sc_dgk_step4(sc_ctx* ctx, int mod, int cst_g, int cst_ginv, int l, const uint32_t* beta, const uint32_t* beta_inv,
                 const uint32_t* d, const uint32_t* d_inv, const uint64_t* alpha, const uint64_t* alpha_tilde,
                 const uint64_t* rsmall, const uint64_t* delta_a, uint32_t* c_out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;  // empty batch: nothing to do (pointers may be null)
  if (!valid_mod(ctx, mod) || l <= 0 || l > SC_MAX_L || !beta || !beta_inv || !d || !d_inv || !alpha || !alpha_tilde || !rsmall || !delta_a || !c_out)
    return fail(ctx, SC_ERR_ARG, "sc_dgk_step4: bad argument");
  if (cst_g < 0 || cst_ginv < 0 || cst_g >= (int)ctx->consts.size() || cst_ginv >= (int)ctx->consts.size() ||
      ctx->consts[cst_g].mod != mod || ctx->consts[cst_ginv].mod != mod)
    return fail(ctx, SC_ERR_ARG, "sc_dgk_step4: bad constant");
  const Mod& m = ctx->mods[mod];
  std::string key = "step4:" + std::to_string(mod) + ":" + std::to_string(cst_g) + ":" + std::to_string(cst_ginv) + ":" + std::to_string(l);
  // Per comparison and bit the step formulas (SC/initiator.py:317-320, 368-371, 471-482) multiply by factors that depend only on the
  // comparison and on the two flag bits (alpha_i, alpha~_i):
  //   w_i = base_i * K[alpha_i][alpha~_i],   base_i = [beta_i] (alpha_i = 0) or [beta_i]^-1 (alpha_i = 1),
  //         K = 1, d'^-1, g d'^-1, g   for (0,0), (0,1), (1,0), (1,1)      (4d: [1] - [beta_i] = g [beta_i]^-1; 4e: - [d] where the bits differ)
  //   c_i = [beta_i]^-1 * C[alpha_i][alpha~_i] * (w_sum)^3,
  //         C = g^s, g^s d', g^s g d'^-1, g^s g                            (4h: [s] + alpha_i + [d] (alpha~_i - alpha_i))
  // so launch (a) computes the six factors that are not constants once per comparison and parks them, and the bit loop of launch
  // (b) spends 6 + i products per bit (round 3: 9 + i and a reduction pass; it multiplied g, d'^-1, D and g^s g^alpha in one after
  // the other, by the residue 1 where a factor did not apply, and converted [beta_i], [beta_i]^-1 to Montgomery form first).
  // No conversion and no reduction pass inside the loop: [beta_i] and [beta_i]^-1 enter as the plain residues they are,
  //   * the K factors are parked with a second factor R (K R^2): plain base_i times K R^2 / R = w_i in Montgomery form, which is
  //     what the squarings need;
  //   * the C factors in Montgomery form (C R): plain [beta_i]^-1 times C R / R is plain, times (w_sum)^3 R / R is plain -- the
  //     stored value; likewise g^delta_a is parked plain for c_-1.
  // Same factors, another order: the canonical residues are the same.
  //   park entries: 0 = K01 = d'^-1, 1 = K10 = g d'^-1 (both times R^2), 2 = C00 = g^s, 3 = C01 = g^s d', 4 = C10 = g^s g d'^-1,
  //                 5 = C11 = g^s g (times R), 6 = g^delta_a (plain)
  const int NP = 7;
  uint32_t* d_park;
  { int rc0 = tmp_buf(ctx, TMP_PARK, (size_t)NP * count * m.S * 4, (void**)&d_park); if (rc0) return rc0; }
  const Prog *pa, *pb;
  int rc = cached_prog(ctx, key + ":a3", mod, [&](Builder& bd) {
    const int cg = bd.use_const(cst_g), cgi = bd.use_const(cst_ginv);
    // scratch (Montgomery form): 0 one, 1 g, 2 ginv, 3 d, 4 dinv, 5 d', 6 d'^-1, 7 g^s, 8 g d'^-1
    bd.loadt_const(1); bd.stt(0);
    bd.loadt_const(cg); bd.stt(1);
    bd.loadt_const(cgi); bd.stt(2);
    bd.loadw(0); bd.mul_const(0); bd.stt(3);
    bd.loadw(1); bd.mul_const(0); bd.stt(4);
    // d' = rsmall ? one : d ; d'^-1 likewise   (SC/initiator.py:289-290: [d] <- [0] = g^0 = 1)
    bd.loadt_tblsel(2, 0, 2, 0, 3, 3, 0, 0); bd.stt(5);
    bd.loadt_tblsel(2, 0, 2, 0, 4, 4, 0, 0); bd.stt(6);
    bd.mul_const(0); bd.storel(4, 0);                                              // K01 = d'^-1          (R^2)
    bd.loadt_tbl(6); bd.mul_tbl(1); bd.stt(8); bd.mul_const(0); bd.storel(4, 1);   // K10 = g d'^-1        (R^2)
    // g^s, s = 1 - 2 delta_a  (delta_a = 1 -> g^-1, SC/initiator.py:459-461)
    bd.loadt_tblsel(3, 0, 3, 0, 1, 1, 2, 2); bd.stt(7); bd.storel(4, 2);          // C00 = g^s
    bd.mul_tbl(5); bd.storel(4, 3);                                                // C01 = g^s d'
    bd.loadt_tbl(7); bd.mul_tbl(1); bd.storel(4, 5);                               // C11 = g^s g            (alpha_i = 1, :476)
    bd.loadt_tbl(7); bd.mul_tbl(8); bd.storel(4, 4);                               // C10 = g^s g d'^-1
    bd.loadt_tblsel(3, 0, 3, 0, 0, 0, 1, 1); bd.redc(); bd.storel(4, 6);           // g^delta_a (:484), plain
  }, &pa); if (rc) return rc;
  {
    VmExt ex[5] = {mk_ext(d, m.nwords, m.nwords), mk_ext(d_inv, m.nwords, m.nwords), mk_ext(rsmall, 2, 2), mk_ext(delta_a, 2, 2),
                   mk_ext(d_park, m.S, 0)};
    rc = run_vm(ctx, mod, *pa, ex, 5, count); if (rc) return rc;
  }
  // ---- launch (b): the bit loop i = l-1 .. 0 (SC/initiator.py:471-482) then c_-1 (:484).  About 12 micro-ops per bit (each run of
  // squarings is one op with a repeat count): some 3 000 ops, 48 KB, at l = 255, uploaded once per key and l like any program.
  rc = cached_prog(ctx, key + ":b3", mod, [&](Builder& bd) {
    const int cg = bd.use_const(cst_g);
    // ext: 0 beta, 1 beta_inv, 2 park, 3 alpha, 4 alpha_tilde, 5 out
    // scratch: 0 K00 = R^2, 1 K01, 2 K10, 3 K11 = g R^2, 4 C00, 5 C01, 6 C10, 7 C11, 8 w_sum, 9 w_sum^3
    bd.loadt_const(0); bd.stt(0);
    bd.loadt_extl(2, 0); bd.stt(1);
    bd.loadt_extl(2, 1); bd.stt(2);
    bd.loadt_const(cg); bd.mul_const(0); bd.stt(3);
    for (int e = 0; e < 4; e++) { bd.loadt_extl(2, 2 + e); bd.stt(4 + e); }
    for (int i = l - 1; i >= 0; i--) {
      bd.loadw(1, i);                                                     // [beta_i]^-1, plain
      bd.mul_tblsel(3, i, 4, i, 4, 5, 6, 7);                              // times C                (4h, :471-478)   flags: fa = alpha_i, fb = alpha~_i
      if (i != l - 1) bd.mul_tbl(9);                                      // times (w_sum)^3 ; first iteration: `3 * 0` is the int 0 -> [0] = 1
      bd.storew(5, i + 1);                                                // c_i
      bd.loadw_sel(1, 0, 3, i, i);                                        // base_i, plain          (4d, :317-320)
      bd.mul_tblsel(3, i, 4, i, 0, 1, 2, 3);                              // w_i = base_i K         (4d + 4e, :368-371), Montgomery form
      for (int k = 0; k < i; k++) bd.sqr();                               // w_i^(2^i)              (4f, :406)
      if (i != l - 1) bd.mul_tbl(8);                                      // w_sum *= w_i^(2^i)
      bd.stt(8);
      if (i > 0) { bd.sqr(); bd.mul_tbl(8); bd.stt(9); }                  // its cube for the next bit
    }
    bd.loadt_extl(2, 6); bd.mul_tbl(8); bd.storew(5, 0);                  // c_-1 = g^delta_a * w_sum (:484)
  }, &pb); if (rc) return rc;
  const uint32_t fw = 2 * (uint32_t)((l + 63) / 64);   // 32-bit words per flag row of alpha / alpha~ (include/sc_amd.h)
  VmExt ex[6] = {mk_ext(beta, m.nwords, m.nwords), mk_ext(beta_inv, m.nwords, m.nwords), mk_ext(d_park, m.S, 0),
                 mk_ext(alpha, fw, fw), mk_ext(alpha_tilde, fw, fw), mk_ext(c_out, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *pb, ex, 6, count);
}

int sc_crt_combine(sc_ctx* ctx, int mod_p, int mod_full, int cst_k, int cst_negk, int cst_mq, const uint32_t* a_p, int a_p_words,
                   const uint32_t* a_q, int a_q_words, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!valid_mod(ctx, mod_p) || !valid_mod(ctx, mod_full) || !a_p || !a_q || !out || a_p_words <= 0 || a_q_words <= 0)
    return fail(ctx, SC_ERR_ARG, "sc_crt_combine: bad argument");
  for (int c : {cst_k, cst_negk, cst_mq})
    if (c < 0 || c >= (int)ctx->consts.size()) return fail(ctx, SC_ERR_ARG, "sc_crt_combine: bad constant");
  if (ctx->consts[cst_k].mod != mod_p || ctx->consts[cst_negk].mod != mod_p || ctx->consts[cst_mq].mod != mod_full)
    return fail(ctx, SC_ERR_ARG, "sc_crt_combine: constant registered for another modulus");
  const Mod& mp = ctx->mods[mod_p];
  const Mod& mf = ctx->mods[mod_full];
  uint32_t* d_t;
  { int rc0 = tmp_buf(ctx, TMP_CRT, (size_t)count * mp.nwords * 4, (void**)&d_t); if (rc0) return rc0; }
  std::string k1 = "crt1:" + std::to_string(mod_p) + ":" + std::to_string(cst_k) + ":" + std::to_string(cst_negk) + ":" + std::to_string(a_p_words) + ":" + std::to_string(a_q_words);
  const Prog *p1, *p2;
  int rc = cached_prog(ctx, k1, mod_p, [&](Builder& bd) -> int {
    const int ck = bd.use_const(cst_k), cn = bd.use_const(cst_negk);
    int kc = -1;
    if (a_p_words > mp.nwords || a_q_words > mp.nwords) { int cid; int rc = get_const_kred(ctx, mod_p, &cid); if (rc) return rc; kc = bd.use_const(cid); }
    if (a_p_words > mp.nwords) emit_load_reduced(ctx, mp, bd, 0, a_p_words, kc); else bd.loadw(0, 0, 0, a_p_words);
    bd.mul_const(ck); bd.stt(0);                                     // a_p * k
    if (a_q_words > mp.nwords) emit_load_reduced(ctx, mp, bd, 1, a_q_words, kc); else bd.loadw(1, 0, 0, a_q_words);
    bd.mul_const(cn); bd.addt(0);                                    // + a_q * (m_p - k)  = (a_p - a_q) * m_q^-1  (mod m_p)
    bd.storew(2);
    return SC_OK;
  }, &p1); if (rc) return rc;
  {
    VmExt ex[3] = {mk_ext(a_p, a_p_words, a_p_words), mk_ext(a_q, a_q_words, a_q_words), mk_ext(d_t, mp.nwords, mp.nwords)};
    rc = run_vm(ctx, mod_p, *p1, ex, 3, count); if (rc) return rc;
  }
  std::string k2 = "crt2:" + std::to_string(mod_full) + ":" + std::to_string(cst_mq) + ":" + std::to_string(mp.nwords) + ":" + std::to_string(a_q_words);
  rc = cached_prog(ctx, k2, mod_full, [&](Builder& bd) {
    const int cm = bd.use_const(cst_mq);
    bd.loadw(0, 0, 0, mp.nwords); bd.mul_const(cm);                  // m_q * t   (< m_p m_q: exact)
    bd.addw(1, 0, 0, a_q_words);                                     // + a_q
    bd.storew(2);
  }, &p2); if (rc) return rc;
  VmExt ex[3] = {mk_ext(d_t, mp.nwords, mp.nwords), mk_ext(a_q, a_q_words, a_q_words), mk_ext(out, mf.nwords, mf.nwords)};
  return run_vm(ctx, mod_full, *p2, ex, 3, count);
}
}  // extern "C"

// ---- twin contexts ---------------------------------------------------------------------------------------------------------------
// A twin is a second registration of a modulus (or of its multiple M = c n) in another configuration, made on first use and kept
// for the life of the context.  Which twin a call takes is decided in sc_route.h; here they are made and remembered.
enum TwinKind { TWIN_PAIR, TWIN_LATENCY_PAIR, TWIN_NEG1, TWIN_ONELANE };

// The twin of `mod` of this kind: the remembered one, else what `make` registers for a COPY of the modulus -- create_mod appends to
// ctx->mods, so no reference into that table may be held across it, here or in `make` -- remembered too, a failure as -1.
static int twin_of(sc_ctx* ctx, TwinKind kind, int mod, const std::function<int(const Mod&)>& make) {
  const auto key = std::make_pair((int)kind, mod);
  auto it = ctx->twins.find(key);
  if (it != ctx->twins.end()) return it->second;
  const Mod m = ctx->mods[mod];
  const int twin = make(m);
  ctx->twins[key] = twin;
  return twin;
}
// ... of the same modulus in the first pair-capable configuration that fits (for_pairs) or in `forced`
static int same_modulus_twin(sc_ctx* ctx, TwinKind kind, int mod, bool for_pairs, const Config* forced) {
  return twin_of(ctx, kind, mod, [&](const Mod& m) {
    int twin = -1;
    return create_mod(ctx, m.n.data(), (int)m.n.size(), for_pairs, &twin, forced) == SC_OK ? twin : -1;
  });
}

// the context the pair kernel runs in for modulus `mod`: itself when its configuration has a pair kernel, otherwise a twin
// context of the same modulus in a pair-capable configuration (created on first use); -1 if no configuration fits
static int pair_twin(sc_ctx* ctx, int mod) {
  const Mod& m = ctx->mods[mod];
  return pair_capable(m.G, m.L, m.W) ? mod : same_modulus_twin(ctx, TWIN_PAIR, mod, true, nullptr);
}

// The small-batch pair twin of `mod` when this batch should run on it (latency_pair_config), else -1.
static int latency_pair_twin(sc_ctx* ctx, int mod, uint64_t count) {
  const Mod& m = ctx->mods[mod];
  const Config* cfg = latency_pair_config(shape_of(m), m.nbits, m.nwords, policy_of(ctx), count);
  return cfg ? same_modulus_twin(ctx, TWIN_LATENCY_PAIR, mod, false, cfg) : -1;
}

// The twin of a (4,18) / (4,14) / (8,14) modulus n whose own modulus is the multiple M = c n, c = -n^-1 mod 2^29, so that M = -1
// (mod 2^29): in its context the Montgomery quotient digit needs no multiplication (Grp::NEG1).  M has at most 29 more bits than n;
// the (4,18) configuration holds 2088 bits, so 2048-bit moduli fit (R / M >= 2^11), and the L = 14 pair twins of 1536 / 3072-bit
// moduli (1624 / 3248 bits) have the room as well; a multiple that would not fit whole words gets no twin.  Residues modulo M (and pairs modulo M^2) reduce to
// residues modulo n (n^2): the caller finishes in a context of the original modulus.  -1: no such twin (other configurations,
// moduli too long, or n already = -1).
static int neg1_twin(sc_ctx* ctx, int mod) {
  return twin_of(ctx, TWIN_NEG1, mod, [&](const Mod& m) {
    static const bool enabled = []{ const char* e = getenv("SC_NEG1"); return !(e && e[0] == '0'); }();      // A/B switch (dev): SC_NEG1=0
    if (!enabled || !neg1_candidate(shape_of(m), m.nbits)) return -1;
    const Big M = big_trimmed(big_mul(m.n, Big(1, m.n0inv)));
    const Config same = {m.G, m.L, m.W, false};
    int twin = -1;
    if (!fits(same, big_bits(M), (int)M.size(), true) || create_mod(ctx, M.data(), (int)M.size(), false, &twin, &same) != SC_OK) return -1;
    if (ctx->mods[twin].n0inv != 1) return -1;     // (cannot happen: M = -1 mod 2^29 by construction)
    // what a single-modulus program needs to leave the context with a residue modulo n (sc_vm.h)
    uint32_t inv = m.n0inv;                                    // c is odd: c c = 1 (mod 8); Newton doubles the good bits
    for (int it = 0; it < 5; it++) inv *= 2u - m.n0inv * inv;
    ctx->mods[twin].small_c = m.n0inv;
    ctx->mods[twin].small_cinv = inv & ((1u << m.W) - 1);
    return twin;
  });
}

int sc_host::neg1_vm_twin(sc_ctx* ctx, int mod, uint64_t count) {
  if (!neg1_vm_allowed(shape_of(ctx->mods[mod]), policy_of(ctx), count)) return -1;
  const int t = neg1_twin(ctx, mod);
  return (t >= 0 && ctx->mods[t].small_c != 0) ? t : -1;
}

// ---- the constants of the one-lane policy, measured per device ---------------------------------------------------------------
// Both forms run in rounds of their resident waves: 2 waves per SIMD, 64 numbers per one-lane wave and 32 per two-lane wave.  What a
// batch costs in either form is a sum of full rounds plus one partial round, and a partial round that leaves every SIMD at most one
// wave costs about half -- how much exactly depends on the part (issue rate of a lone wave, clocks), so it is measured, once per
// device and process, on a fixed 1024-bit odd modulus and a 1024-bit exponent -- the shape of the key holder's first CRT stage; a
// 256-bit exponent gave other RATIOS (two-lane round 0.53 instead of 0.60 of a one-lane round: the window tables weigh differently)
// and mis-ranked the forms at half a round.  About 80 ms of launches.  Round 3 had these as constants fitted on one box (0.6 / 0.27 /
// 0.38 of a one-lane round): the defaults of OneLaneCal (sc_route.h).
static std::mutex g_cal_mutex;
static std::map<int, OneLaneCal> g_cal;           // by device


static int onelane_calibrate(sc_ctx* ctx, OneLaneCal* out) {
  OneLaneCal c;
  c.simds = ctx->num_cu * 4;
  const int nw = 32;
  Big n(nw, 0xffffffffu); n[0] = 0xffffff61u; n[nw - 1] = 0xfffffff1u;          // any odd 1024-bit number serves Montgomery arithmetic
  Big e(32, 0xa5c3965au); e[31] = 0x96a5c35au;                                    // 1024 bits, half of them set
  int mod = -1, exp = -1;
  int rc = create_mod(ctx, n.data(), nw, false, &mod); if (rc) return rc;
  rc = sc_exp_create(ctx, e.data(), (int)e.size(), &exp); if (rc) return rc;
  const uint64_t n1 = (uint64_t)c.simds * 2 * 64, n2 = n1 / 2;                    // numbers of a full one-lane / two-lane round
  DevBuf<uint32_t> x, y;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc((void**)&x.p, n1 * nw * 4));
  HIPCHK(ctx, hipMalloc((void**)&y.p, n1 * nw * 4));
  HIPCHK(ctx, hipMemsetAsync(x.p, 0x5a, n1 * nw * 4, ctx->stream));
  LaunchTimer timer(ctx);
  PolicyOverride keep(ctx);
  ctx->latency_mode = 0; ctx->chip_share = 1;
  auto timed = [&](int form, uint64_t count, double* ms) -> int {
    ctx->onelane_mode = form;                     // 0: the modulus's own two-lane configuration, 2: the one-lane twin
    double best = 1e30;
    for (int rep = 0; rep < 2; rep++) {
      float t = 0;
      int r = timer.time([&] { return modexp_shared_impl(ctx, mod, exp, x.p, nw, nullptr, y.p, nullptr, count, nullptr, 0, false); }, &t);
      if (r) return r;
      if (t < best) best = t;
    }
    *ms = best;
    return SC_OK;
  };
  double two_15 = 0, warm = 0;
  rc = timed(2, 64, &warm);                       // program build, code load
  if (!rc) rc = timed(0, 64, &warm);
  if (!rc) rc = timed(2, n1, &c.one_full);
  if (!rc) rc = timed(2, n1 / 2, &c.one_half);
  if (!rc) rc = timed(0, n2, &c.two_full);
  if (!rc) rc = timed(0, n2 / 2, &c.two_only_half);
  if (!rc) rc = timed(0, n2 + n2 / 2, &two_15);
  if (rc) return rc;
  c.two_half = std::max(0.0, two_15 - c.two_full);
  // A calibration taken while something else used the chip (another context's launches, another process) gives ratios no idle
  // chip produces; the policy then keeps the built-in constants rather than rank the forms by a skewed measurement (results are
  // the same residues either way: only throughput depends on it).  Plausible: a half round costs between a third of and a whole
  // full round; a two-lane round -- half the numbers -- between 0.3 and 0.9 of a one-lane round.
  const double r_half = c.one_half / c.one_full, r_two = c.two_full / c.one_full, r_only = c.two_only_half / c.two_full;
  c.ok = c.one_full > 0 && c.two_full > 0 && r_half > 0.33 && r_half <= 1.0 && r_two > 0.3 && r_two < 0.9 && r_only > 0.3 && r_only <= 1.05 &&
         c.two_half <= c.two_full * 1.05;
  if (!c.ok) { OneLaneCal d; d.simds = c.simds; const double scale = c.one_full > 0 ? c.one_full : 1.0;
               d.one_full *= scale; d.one_half *= scale; d.two_full *= scale; d.two_half *= scale; d.two_only_half *= scale; c = d; }
  *out = c;
  return SC_OK;
}

OneLaneCal sc_host::onelane_cal(sc_ctx* ctx) {
  std::lock_guard<std::mutex> lock(g_cal_mutex);
  auto it = g_cal.find(ctx->device);
  if (it != g_cal.end()) return it->second;
  OneLaneCal c;
  if (onelane_calibrate(ctx, &c) != SC_OK) { c = OneLaneCal(); c.simds = ctx->num_cu * 4; }
  g_cal[ctx->device] = c;
  return c;
}

extern "C" int sc_ctx_policy(sc_ctx* ctx, double* out6) {
  if (!ctx || !out6) return SC_ERR_ARG;
  const OneLaneCal c = onelane_cal(ctx);
  out6[0] = c.one_full; out6[1] = c.one_half; out6[2] = c.two_full; out6[3] = c.two_half; out6[4] = c.two_only_half; out6[5] = (double)c.simds;
  return c.ok ? SC_OK : fail(ctx, SC_ERR_HIP, "sc_ctx_policy: the calibration launches failed (the built-in constants are in use)");
}

// The one-lane twin of `mod` when this batch should run on it, else `mod` itself.  Automatic policy: the modulus fits the one-lane
// configuration and the model above -- full rounds plus one partial round per form, with this device's measured round times -- says
// the one-lane form is faster.  Shape of the trade (MI355X, 1024-bit modulus and exponent, profiles/r03_onelane_policy_sweep.txt):
// 196608 numbers 19.8 -> 16.6 ms, 2.1 M numbers (zero tests) 37.3 -> 33.0 ms, but 98304 numbers 9.5 -> 11.6 ms -- three quarters of a
// round leaves a quarter of the SIMDs with one wave and nobody to hide its latencies, where the two-lane form still runs 1.5 rounds.
// When several contexts work on the GPU at once (concurrent shards: sc_ctx_set_chip_share) a launch owns its share of the chip
// only, and the idle SIMDs of an under-filled launch are taken by the other contexts' kernels: rounds are counted on that share
// (two shards of 32768 comparisons: the 98304-number launches run one-lane, +1.5 % on the whole step).
int sc_host::onelane_for(sc_ctx* ctx, int mod, uint64_t count) {
  if (ctx->onelane_mode == 0) return mod;
  if (const Mod& m = ctx->mods[mod]; !onelane_eligible(shape_of(m), m.nbits, m.nwords)) return mod;
  // (the calibration may register moduli: no reference into ctx->mods is held across it)
  if (ctx->onelane_mode == 1 && !onelane_faster(onelane_cal(ctx), count, ctx->chip_share, ctx->num_cu)) return mod;
  const int twin = same_modulus_twin(ctx, TWIN_ONELANE, mod, false, &kOneLane);
  return twin < 0 ? mod : twin;
}

// ---- measured op times of the pair kernel instances (the segment policy of sc_modexp_shared_sq) -------------------------------------
// One pair squaring and one pair product of a resident wave of the instance a launch takes, in milliseconds, with the chip as full as the
// launch itself makes it (up to one round of resident waves: two waves share a SIMD's issue slots, a lone wave runs its program almost
// twice as fast): timed as the difference of two short programs (16 / 48 squarings; 8 / 24 products) on the caller's own operands, best
// of three (other contexts may be using the chip), once per process, device and instance.  A few milliseconds.
struct PairOpTimes { double sqr_ms = 0, mul_ms = 0; };
static std::mutex g_pair_cal_mutex;
static std::map<std::tuple<int, int, int, bool>, PairOpTimes> g_pair_cal;     // (device, G, L, neg1)

static int pair_op_times(sc_ctx* ctx, int mod_m, uint64_t count, int x_words, const VmExt* ex3, double* sqr_ms, double* mul_ms) {
  const Instance k = pvm_instance(shape_of(ctx->mods[mod_m]), policy_of(ctx), count);
  const int G = k.G, L = k.L; const bool neg1 = k.neg1;
  const auto key = std::make_tuple(ctx->device, G, L, neg1);
  std::lock_guard<std::mutex> lock(g_pair_cal_mutex);
  auto it = g_pair_cal.find(key);
  if (it != g_pair_cal.end()) { *sqr_ms = it->second.sqr_ms; *mul_ms = it->second.mul_ms; return SC_OK; }
  const Mod m = ctx->mods[mod_m];
  const uint32_t nw = (uint32_t)std::min(x_words, m.nwords);
  Prog progs[4];
  const int shapes[4][2] = {{16, 0}, {48, 0}, {0, 8}, {0, 24}};
  for (int i = 0; i < 4; i++) {
    PairBuilder pb(m);
    pb.loadu(0, 0, nw); pb.mul_const(2); pb.stt(1);
    for (int k = 0; k < shapes[i][0]; k++) pb.sqr();
    for (int k = 0; k < shapes[i][1]; k++) pb.mul_tbl(1);
    pb.out(1, 2);
    int rc = pb.finalize(ctx, mod_m, &progs[i]); if (rc) return rc;
    progs[i].muls_per_item = 0; progs[i].pair_sqrs = progs[i].pair_muls = 0;     // probes, not work: nothing to count
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  LaunchTimer timer(ctx);
  PolicyOverride keep(ctx);
  // the wave must run on the SAME instance as the launch it stands for: the batch-size policy is told the real batch size by keeping
  // the latency mode out of it (a tiny batch would otherwise pick the small-batch twin)
  ctx->latency_mode = small_batch(shape_of(m), policy_of(ctx), count) ? 2 : 0;
  const int occ = pvm_occupancy(ctx, G, L, neg1);
  const uint64_t one_wave = std::min<uint64_t>(count, (uint64_t)(64 / G) * (uint64_t)ctx->num_cu * (uint64_t)std::max(1, occ));   // (at most one round)
  double ms[4] = {1e30, 1e30, 1e30, 1e30};
  for (int rep = 0; rep < 4; rep++)                 // the first pass loads the code
    for (int i = 0; i < 4; i++) {
      float t = 0;
      int rc = timer.time([&] { return run_pvm(ctx, mod_m, progs[i], ex3, 3, one_wave); }, &t); if (rc) return rc;
      if (rep > 0 && t < ms[i]) ms[i] = t;
    }
  PairOpTimes t;
  t.sqr_ms = std::max(1e-6, (ms[1] - ms[0]) / 32.0);
  t.mul_ms = std::max(1e-6, (ms[3] - ms[2]) / 16.0);
  g_pair_cal[key] = t;
  ctx->stat_pair_calibrations++;
  *sqr_ms = t.sqr_ms; *mul_ms = t.mul_ms;
  return SC_OK;
}

extern "C" {

int sc_ctx_set_pair_policy(sc_ctx* ctx, double hold_ms, double max_rounds) {
  if (!ctx || hold_ms < 0 || !(max_rounds > 0)) return SC_ERR_ARG;
  ctx->pair_hold_ms = hold_ms;
  ctx->pair_max_rounds = max_rounds;
  return SC_OK;
}

int sc_ctx_stats(sc_ctx* ctx, uint64_t* out, int n) {
  if (!ctx || !out || n < 0) return SC_ERR_ARG;
  const uint64_t v[3] = {ctx->stat_segmented_launches, ctx->stat_segments, ctx->stat_pair_calibrations};
  for (int i = 0; i < n; i++) out[i] = i < 3 ? v[i] : 0;
  return SC_OK;
}

int sc_ctx_launch_counts(sc_ctx* ctx, uint32_t* keys_out, uint64_t* counts_out, int cap, int* n_out) {
  if (!ctx || !n_out || cap < 0 || (cap > 0 && (!keys_out || !counts_out))) return SC_ERR_ARG;
  int i = 0;
  for (const auto& kv : ctx->launch_counts) {
    if (i < cap) { keys_out[i] = kv.first; counts_out[i] = kv.second; }
    i++;
  }
  *n_out = i;
  return SC_OK;
}

int sc_ctx_set_chip_share(sc_ctx* ctx, int contexts) {
  if (!ctx || contexts < 1 || contexts > 64) return SC_ERR_ARG;
  ctx->chip_share = contexts;
  return SC_OK;
}

int sc_ctx_set_fork_mode(sc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return SC_ERR_ARG;
  ctx->fork_mode = mode;
  return SC_OK;
}

int sc_ctx_set_onelane_mode(sc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return SC_ERR_ARG;
  ctx->onelane_mode = mode;
  return SC_OK;
}

int sc_mod_supports_sq(sc_ctx* ctx, int mod) {
  if (!valid_mod(ctx, mod)) return SC_ERR_ARG;
  return pair_twin(ctx, mod) >= 0 ? 1 : 0;
}

// ---- sc_modexp_shared_sq: x^e mod m^2 with products modulo m only --------------------------------------------------------------
// Launch 1, the pair exponentiation in the m context: the operand embedded (Horner over chunks of nwords words, LDS constants
// pair(R^2), pair(B R)), then the window schedule on pairs; leaves the raw pair halves w0, w1 in ext 1, 2.
static int pair_pow_prog(sc_ctx* ctx, const std::string& key, int mod_m, int exp, int x_words, const Prog** out) {
  const Mod& m = ctx->mods[mod_m];
  return cached_prog(ctx, key, mod_m, [&](PairBuilder& pb) -> int {
    const int nch = (x_words + m.nwords - 1) / m.nwords;
    const uint32_t TMP_E = 0;                                            // scratch pair entry used while embedding
    for (int t = nch - 1; t >= 0; t--) {
      const int nw = std::min(m.nwords, x_words - t * m.nwords);
      if (t != nch - 1) { pb.mul_const(4); pb.stt(TMP_E); }
      pb.loadu(0, (uint32_t)(t * m.nwords), (uint32_t)nw);
      pb.mul_const(2);
      if (t != nch - 1) pb.addt(TMP_E);
    }
    const Exp& ex = ctx->exps[exp];
    if (ex.bits == 0) return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_sq: zero exponent");
    emit_window_pow(pb, ex, 1);                                          // table entries 1 .. NT, x^2 at 1 + NT
    pb.out(1, 2);
    return SC_OK;
  }, out, PairBuilder(m));
}

// Into how many segments launch 1 is cut (1: left whole).
// A context that shares the chip (concurrent shards, sc_ctx_set_chip_share) runs a SINGLE-ROUND pair launch -- every resident
// wave holds its one group of items for the whole exponentiation: Alice's rho^N for a shard of 32768 is 2048 waves for 54 ms --
// in SEGMENTS: the same micro-program cut at window boundaries into a few launches, the pair parked in a row of the slot's
// table in between (slot = item while there is one round).  Waves of a launch retire together, so nothing another context
// queues behind such a launch gets a wave slot before it ends: the other shard's short, latency-bound launches (the inversion
// sweeps of steps 1 and 6 / 7, the assembly launch after ITS pair launch) were seen waiting 26 .. 32 ms each.  With segments
// they wait for a quarter of that.  Multi-round launches need none of this (their waves retire a round apart).
// Whether, and into how many segments: from MEASUREMENTS, not from the shape of the launch.  A resident wave holds its slot for
// hold = (pair squarings x t_sqr + pair products x t_mul) of this program, with the two op times of this kernel instance measured on
// the device (pair_op_times, once per process and instance: a lone wave, like each of two waves sharing a SIMD, issues one
// multiply-add per ~9.5 cycles, so its time through the program is the time a round of resident waves takes).  The launch is cut when
// it would take more than half of the chip's wave slots for that long on a SHARED chip (sc_ctx_set_chip_share), into
// round(hold / pair_hold_ms) segments; launches of more than pair_max_rounds rounds stay whole (their waves retire a round apart
// anyway, and every segment boundary costs a drain of the chip).  Both knobs: sc_ctx_set_pair_policy.
static int pair_segment_count(sc_ctx* ctx, int mod_m, const Prog& prog, uint64_t count, int x_words, const VmExt* ex3, int* out_K) {
  *out_K = 1;
  const Instance k = pvm_instance(shape_of(ctx->mods[mod_m]), policy_of(ctx), count);
  const int iG = k.G, occ = pvm_occupancy(ctx, k.G, k.L, k.neg1);
  const uint64_t wave_items = (count + (uint64_t)(64 / iG) - 1) / (uint64_t)(64 / iG);
  const uint64_t resident = (uint64_t)ctx->num_cu * (uint64_t)std::max(1, occ);
  const double rounds = (double)wave_items / (double)resident;
  if (ctx->pair_hold_ms > 0 && ctx->chip_share > 1 && !ctx->stamps && occ > 0 && wave_items * 2 > resident && rounds <= ctx->pair_max_rounds) {
    double t_sqr = 0, t_mul = 0;
    int rc = pair_op_times(ctx, mod_m, count, x_words, ex3, &t_sqr, &t_mul); if (rc) return rc;
    const double hold_ms = prog.pair_sqrs * t_sqr + prog.pair_muls * t_mul;
    *out_K = (int)std::min(16.0, std::max(1.0, std::floor(hold_ms / ctx->pair_hold_ms + 0.5)));
  }
  return SC_OK;
}

// Launch 1 in K segments, cut from the program's host copy (cached under `key`), each launched on a table slot per item.
static int run_pair_segments(sc_ctx* ctx, int mod_m, const std::string& key, const Prog& full, int K, const VmExt* ex3, uint64_t count) {
  auto its = ctx->seg_progs.find(key);
  if (its == ctx->seg_progs.end()) {
    if (!full.host_ops) return fail(ctx, SC_ERR_HIP, "sc_modexp_shared_sq: pair program without its host copy (internal error)");
    const std::vector<VmOp>& ops = *full.host_ops;
    // cut after a PV_MULT (the end of a window) nearest to each k / K of the op list past the table build
    std::vector<size_t> mults;
    size_t body = 0;
    for (size_t i = 0; i < ops.size(); i++) if ((ops[i].w0 & 0xff) == PV_MULT) mults.push_back(i);
    for (size_t i = 0; i < ops.size(); i++) if ((ops[i].w0 & 0xff) == PV_SQR && i > 0 && (ops[i - 1].w0 & 0xff) == PV_LOADT) body = i;   // first squaring run after the first window's load
    std::vector<size_t> cuts;      // index of the first op of segments 1 .. K-1
    for (int k = 1; k < K; k++) {
      const size_t target = body + (ops.size() - body) * (size_t)k / (size_t)K;
      size_t best = 0;
      for (size_t mi : mults) if (mi + 1 > body && (best == 0 || (mi + 1 > target ? mi + 1 - target : target - mi - 1) < (best > target ? best - target : target - best))) best = mi + 1;
      if (best > (cuts.empty() ? body : cuts.back()) && best + 1 < ops.size()) cuts.push_back(best);
    }
    const uint32_t E = full.nscratch / 2;            // one more pair row of the slot's table: the parked state
    std::vector<Prog> segs;
    size_t from = 0;
    for (size_t c = 0; c <= cuts.size(); c++) {
      const size_t to = c < cuts.size() ? cuts[c] : ops.size();     // the last segment ends with the program's own PV_OUT, PV_END
      std::vector<VmOp> so;
      if (c > 0) so.push_back(pv_op(PV_LOADT, E));
      so.insert(so.end(), ops.begin() + from, ops.begin() + to);
      if (c < cuts.size()) { so.push_back(pv_op(PV_STT, E)); so.push_back(pv_op(PV_END)); }
      Prog sp = full;
      sp.host_ops.reset();
      sp.nops = (uint32_t)so.size(); sp.nscratch = full.nscratch + 2;
      sp.muls_per_item = full.muls_per_item * (double)(to - from) / (double)ops.size();
      int rc = upload(ctx, so.data(), so.size() * sizeof(VmOp), (void**)&sp.d_ops); if (rc) return rc;
      segs.push_back(sp);
      from = to;
    }
    its = ctx->seg_progs.emplace(key, segs).first;
  }
  ctx->slot_per_item = true;        // a table slot per item: what a segment parks is still there for the next one, whatever the rounds
  ctx->stat_segmented_launches++; ctx->stat_segments += its->second.size();
  int rc = SC_OK;
  for (const Prog& sp : its->second) { rc = run_pvm(ctx, mod_m, sp, ex3, 3, count); if (rc) break; }
  ctx->slot_per_item = false;
  return rc;
}

// Launch 2, in the m^2 context: out = (w0 + w1 m) [* mul_into] mod m^2
static int pair_assemble(sc_ctx* ctx, int mod_m, int mod_m2, const uint32_t* d_w, const uint32_t* d_w1, int wm, const uint32_t* mul_into,
                         uint32_t* out, uint64_t count) {
  int cst_m;
  int rc = sc_const_create_cached(ctx, mod_m2, ctx->mods[mod_m].n, &cst_m); if (rc) return rc;
  std::string key = "psq2:" + std::to_string(mod_m2) + ":" + std::to_string(cst_m) + ":" + std::to_string(wm) + ":" + std::to_string(mul_into ? 1 : 0);
  const Prog* p;
  rc = cached_prog(ctx, key, mod_m2, [&](Builder& bd) {
    const int cm = bd.use_const(cst_m);
    bd.loadw(1, 0, 0, wm); bd.mul_const(cm);           // w1 * m  (mod m^2)
    bd.addw(0, 0, 0, wm);                              // + w0
    if (mul_into) { bd.mul_const(0); bd.mul_extw(2); } // to Montgomery form, times the ciphertext
    bd.storew(3);
  }, &p); if (rc) return rc;
  const Mod& m2 = ctx->mods[mod_m2];
  VmExt ex4[4] = {mk_ext(d_w, wm, wm), mk_ext(d_w1, wm, wm), mk_ext(mul_into, m2.nwords, m2.nwords), mk_ext(out, m2.nwords, m2.nwords)};
  return run_vm(ctx, mod_m2, *p, ex4, 4, count);
}

int sc_modexp_shared_sq(sc_ctx* ctx, int mod_m, int mod_m2, int exp, const uint32_t* x, int x_words, const uint32_t* mul_into,
                        uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!valid_mod(ctx, mod_m) || !valid_mod(ctx, mod_m2) || exp < 0 || exp >= (int)ctx->exps.size() || !x || !out || x_words <= 0)
    return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_sq: bad argument");
  const int lat = latency_pair_twin(ctx, mod_m, count);
  mod_m = lat >= 0 ? lat : pair_twin(ctx, mod_m);
  if (mod_m < 0) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_modexp_shared_sq: no pair configuration fits this modulus");
  {
    const Mod& m0 = ctx->mods[mod_m];
    const Mod& m2 = ctx->mods[mod_m2];
    Big sq = big_mul(m0.n, m0.n);
    sq.resize(std::max(sq.size(), m2.n.size()), 0);
    Big other = m2.n; other.resize(sq.size(), 0);
    if (big_cmp(sq, other) != 0) return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_sq: mod_m2 is not the square of mod_m");
    if (x_words > 4 * m0.nwords) return fail(ctx, SC_ERR_ARG, "sc_modexp_shared_sq: operand wider than 4 chunks");
  }
  // chip-filling batches of a (4,18) / (4,14) / (8,14) modulus: the pair launch runs modulo the multiple M = c m = -1 (mod 2^29),
  // which needs no quotient multiply; the assembly launch reduces w0 + w1 M modulo m^2 (m | M)
  if (!small_batch(shape_of(ctx->mods[mod_m]), policy_of(ctx), count)) { const int t = neg1_twin(ctx, mod_m); if (t >= 0) mod_m = t; }
  const int wm = ctx->mods[mod_m].nwords + 1;                            // words of the raw pair halves (< 2m + 1)
  uint32_t* d_w;
  int rc = tmp_buf(ctx, TMP_PAIR, (size_t)count * wm * 4 * 2, (void**)&d_w); if (rc) return rc;
  uint32_t* d_w1 = d_w + (size_t)count * wm;
  const std::string key = "psq:" + std::to_string(mod_m) + ":" + std::to_string(exp) + ":" + std::to_string(x_words);
  const Prog* prog;
  rc = pair_pow_prog(ctx, key, mod_m, exp, x_words, &prog); if (rc) return rc;
  const VmExt ex3[3] = {mk_ext(x, x_words, x_words), mk_ext(d_w, wm, wm), mk_ext(d_w1, wm, wm)};
  int K;
  rc = pair_segment_count(ctx, mod_m, *prog, count, x_words, ex3, &K); if (rc) return rc;
  if (K > 1) rc = run_pair_segments(ctx, mod_m, key + ":seg" + std::to_string(K), *prog, K, ex3, count);
  else rc = run_pvm(ctx, mod_m, *prog, ex3, 3, count);
  if (rc) return rc;
  return pair_assemble(ctx, mod_m, mod_m2, d_w, d_w1, wm, mul_into, out, count);
}

// ---- sc_modexp_var_sq: prod_j x_j^e_j mod m^2 with exponents per row, products modulo m only -----------------------------------
// The window that minimises the table build plus the digit products of nb tables of 2^w entries (squarings are ebits whatever w);
// at most 5 (nb * 32 pair rows of the slot's table).
static int var_sq_window(int nbases, int ebits) {
  int best = 1; double bc = 1e30;
  for (int w = 1; w <= 5; w++) {
    const double c = nbases * ((double)(1 << w) - 2.0 + std::ceil((double)ebits / w));
    if (c < bc) { bc = c; best = w; }
  }
  return best;
}

// Interleaved (Shamir) fixed-window schedule of up to three bases with exponents per row: table j holds x_j^0 .. x_j^(2^w - 1) in pair
// entries T_j .. T_j + 2^w - 1 (x^0 from the word 1 in ext 6), then per window of w exponent bits, top first: w squarings of the
// shared accumulator and one digit-indexed product per base (PV_MULTDIG on ext 3 + j).  The top window is ebits - (nd - 1) w bits
// wide, so no exponent bit at or above ebits is read.  Operands x: ext 0 as [nb][count][x_words]; the pair halves go to ext 1, 2.
static void emit_var_sq_pow(PairBuilder& pb, const Mod& m, int nbases, int x_words, int ebits, int w) {
  const uint32_t TMP_E = 0, NT = 1u << w;
  const int nch = (x_words + m.nwords - 1) / m.nwords;
  pb.loadu(6, 0, 1); pb.mul_const(2);                                    // pair form of 1
  for (int j = 0; j < nbases; j++) pb.stt(1 + j * NT);
  for (int j = 0; j < nbases; j++) {
    const uint32_t T = 1 + j * NT;
    for (int t = nch - 1; t >= 0; t--) {                                 // x_j embedded (Horner over chunks, as pair_pow_prog)
      const int nw = std::min(m.nwords, x_words - t * m.nwords);
      if (t != nch - 1) { pb.mul_const(4); pb.stt(TMP_E); }
      pb.loadu(0, (uint32_t)(t * m.nwords), (uint32_t)nw, (uint32_t)j);
      pb.mul_const(2);
      if (t != nch - 1) pb.addt(TMP_E);
    }
    pb.stt(T + 1);
    for (uint32_t k = 2; k < NT; k++) { pb.mul_tbl(T + 1); pb.stt(T + k); }
  }
  const int nd = (ebits + w - 1) / w;
  pb.loadt_tbl(1);
  for (int d = nd - 1; d >= 0; d--) {
    const uint32_t width = (d == nd - 1) ? (uint32_t)(ebits - (nd - 1) * w) : (uint32_t)w;
    if (d != nd - 1) for (int k = 0; k < w; k++) pb.sqr();
    for (int j = 0; j < nbases; j++) pb.mul_tbl_digit(3 + j, (uint32_t)(d * w), width, 1 + j * NT);
  }
  pb.out(1, 2);
}

int sc_modexp_var_sq(sc_ctx* ctx, int mod_m, int mod_m2, int nbases, const uint32_t* x, int x_words, const uint32_t* e, int ewords,
                     int ebits, const uint32_t* mul_into, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!valid_mod(ctx, mod_m) || !valid_mod(ctx, mod_m2) || nbases < 1 || nbases > 3 || !x || !e || !out || x_words <= 0 ||
      ewords <= 0 || ebits < 0 || ebits > 32 * ewords || ebits > (1 << 20) - 64)
    return fail(ctx, SC_ERR_ARG, "sc_modexp_var_sq: bad argument");
  mod_m = pair_twin(ctx, mod_m);
  if (mod_m < 0) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_modexp_var_sq: no pair configuration fits this modulus");
  {
    const Mod& m0 = ctx->mods[mod_m];
    const Mod& m2 = ctx->mods[mod_m2];
    if (!((m0.G == 2 && m0.L == 18) || (m0.G == 4 && m0.L == 18) || (m0.G == 8 && m0.L == 14)))
      return fail(ctx, SC_ERR_UNSUPPORTED, "sc_modexp_var_sq: no per-row-exponent pair kernel for G=%d L=%d", m0.G, m0.L);
    Big sq = big_mul(m0.n, m0.n);
    sq.resize(std::max(sq.size(), m2.n.size()), 0);
    Big other = m2.n; other.resize(sq.size(), 0);
    if (big_cmp(sq, other) != 0) return fail(ctx, SC_ERR_ARG, "sc_modexp_var_sq: mod_m2 is not the square of mod_m");
    if (x_words > 4 * m0.nwords) return fail(ctx, SC_ERR_ARG, "sc_modexp_var_sq: operand wider than 4 chunks");
  }
  if (!ctx->d_one) { const uint32_t one = 1; int rc = upload(ctx, &one, 4, (void**)&ctx->d_one); if (rc) return rc; }
  const int w = var_sq_window(nbases, ebits);
  const int wm = ctx->mods[mod_m].nwords + 1;
  uint32_t* d_w;
  int rc = tmp_buf(ctx, TMP_PAIR, (size_t)count * wm * 4 * 2, (void**)&d_w); if (rc) return rc;
  uint32_t* d_w1 = d_w + (size_t)count * wm;
  const std::string key = "pvsq:" + std::to_string(mod_m) + ":" + std::to_string(nbases) + ":" + std::to_string(ebits) + ":" +
                          std::to_string(w) + ":" + std::to_string(x_words);
  const Prog* prog;
  rc = cached_prog(ctx, key, mod_m, [&](PairBuilder& pb) { emit_var_sq_pow(pb, ctx->mods[mod_m], nbases, x_words, ebits, w); },
                   &prog, PairBuilder(ctx->mods[mod_m])); if (rc) return rc;
  VmExt ex[7] = {mk_ext(x, x_words, x_words), mk_ext(d_w, wm, wm), mk_ext(d_w1, wm, wm), mk_ext(e, ewords, ewords),
                 mk_ext(e, ewords, ewords), mk_ext(e, ewords, ewords), mk_ext(ctx->d_one, 0, 1)};
  for (int j = 1; j < nbases; j++) ex[3 + j] = mk_ext(e + (size_t)j * count * ewords, ewords, ewords);
  rc = run_pvm(ctx, mod_m, *prog, ex, 7, count); if (rc) return rc;
  return pair_assemble(ctx, mod_m, mod_m2, d_w, d_w1, wm, mul_into, out, count);
}

// ------------------------------------------------------------------------------------------------
// Multi-GPU: comparisons are independent, so the only exchange is the reassembly of per-rank result blocks -- one
// RCCL all-gather over xGMI on the context's stream.  RCCL is bound at run time (dlopen): a single-GPU user never loads it, and
// a process that already runs torch.distributed gets the very library instance torch loaded.
// ------------------------------------------------------------------------------------------------
namespace {
struct RcclId { char internal[128]; };
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
struct RcclLoad { RcclApi api; std::string err; };
void rccl_load(RcclLoad* out) {
  RcclLoad& r = *out;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
    r.api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (r.api.handle) break;
  }
  if (!r.api.handle) {
    const char* e = dlerror();
    r.err = std::string("cannot load librccl: ") + (e ? e : "not found");
    return;
  }
  r.api.GetUniqueId = (int (*)(RcclId*))dlsym(r.api.handle, "ncclGetUniqueId");
  r.api.CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(r.api.handle, "ncclCommInitRank");
  r.api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(r.api.handle, "ncclAllGather");
  r.api.CommDestroy = (int (*)(void*))dlsym(r.api.handle, "ncclCommDestroy");
  r.api.GetErrorString = (const char* (*)(int))dlsym(r.api.handle, "ncclGetErrorString");
  if (!r.api.GetUniqueId || !r.api.CommInitRank || !r.api.AllGather || !r.api.CommDestroy) { r.err = "librccl lacks an expected symbol"; r.api.handle = nullptr; }
}
RcclApi* rccl_api(std::string* why) {
  static RcclLoad loaded = [] { RcclLoad r; rccl_load(&r); return r; }();   // once per process; initialisation of a local static is thread-safe
  if (!loaded.api.handle) { if (why) *why = loaded.err; return nullptr; }
  return &loaded.api;
}
int rccl_fail(sc_ctx* ctx, RcclApi* api, const char* what, int code) {
  return fail(ctx, SC_ERR_HIP, "%s: %s", what, api->GetErrorString ? api->GetErrorString(code) : "RCCL error");
}
}  // namespace

int sc_comm_unique_id(sc_ctx* ctx, void* id_hptr) {
  if (!ctx || !id_hptr) return fail(ctx, SC_ERR_ARG, "sc_comm_unique_id: bad argument");
  std::string why;
  RcclApi* api = rccl_api(&why);
  if (!api) return fail(ctx, SC_ERR_UNSUPPORTED, "%s", why.c_str());
  RcclId id;
  const int rc = api->GetUniqueId(&id);
  if (rc) return rccl_fail(ctx, api, "ncclGetUniqueId", rc);
  memcpy(id_hptr, id.internal, sizeof id.internal);
  return SC_OK;
}

int sc_comm_init(sc_ctx* ctx, const void* id_hptr, int rank, int nranks) {
  if (!ctx || !id_hptr || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, SC_ERR_ARG, "sc_comm_init: bad argument");
  if (ctx->comm) return fail(ctx, SC_ERR_ARG, "sc_comm_init: the context already has a communicator");
  std::string why;
  RcclApi* api = rccl_api(&why);
  if (!api) return fail(ctx, SC_ERR_UNSUPPORTED, "%s", why.c_str());
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RcclId id;
  memcpy(id.internal, id_hptr, sizeof id.internal);
  void* comm = nullptr;
  const int rc = api->CommInitRank(&comm, nranks, id, rank);
  if (rc) return rccl_fail(ctx, api, "ncclCommInitRank", rc);
  ctx->comm = comm; ctx->comm_rank = rank; ctx->comm_nranks = nranks;
  return SC_OK;
}

int sc_allgather(sc_ctx* ctx, const uint32_t* send, uint32_t* recv, uint64_t words_per_rank) {
  if (!ctx || !ctx->comm) return fail(ctx, SC_ERR_ARG, "sc_allgather: no communicator (sc_comm_init)");
  if (words_per_rank == 0) return SC_OK;
  if (!send || !recv) return fail(ctx, SC_ERR_ARG, "sc_allgather: bad argument");
  RcclApi* api = rccl_api(nullptr);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = api->AllGather(send, recv, (size_t)words_per_rank, 3 /* ncclUint32 */, ctx->comm, ctx->stream);
  if (rc) return rccl_fail(ctx, api, "ncclAllGather", rc);
  return SC_OK;
}

int sc_comm_destroy(sc_ctx* ctx) {
  if (!ctx) return SC_ERR_ARG;
  if (!ctx->comm) return SC_OK;
  RcclApi* api = rccl_api(nullptr);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  const int rc = api ? api->CommDestroy(ctx->comm) : 0;
  ctx->comm = nullptr; ctx->comm_nranks = 0;
  return rc ? rccl_fail(ctx, api, "ncclCommDestroy", rc) : SC_OK;
}

// ------------------------------------------------------------------------------------------------
// Device-side CSPRNG (sc_rng.h): the random draws of a batch are generated where they are consumed.
// ------------------------------------------------------------------------------------------------
int sc_rng_seed(sc_ctx* ctx, const uint8_t* key32_hptr) {
  if (!ctx) return SC_ERR_ARG;
  uint8_t buf[32];
  if (key32_hptr) {
    memcpy(buf, key32_hptr, 32);
  } else {
    size_t got = 0;
    while (got < 32) {
      const ssize_t r = getrandom(buf + got, 32 - got, 0);
      if (r <= 0) return fail(ctx, SC_ERR_HIP, "sc_rng_seed: the operating system's random source failed");
      got += (size_t)r;
    }
  }
  for (int i = 0; i < 8; i++)
    ctx->rng_key.k[i] = (uint32_t)buf[4 * i] | ((uint32_t)buf[4 * i + 1] << 8) | ((uint32_t)buf[4 * i + 2] << 16) | ((uint32_t)buf[4 * i + 3] << 24);
  memset(buf, 0, sizeof buf);
  ctx->rng_seeded = true;
  ctx->rng_call = 0;
  return SC_OK;
}

// every generator call: seeded context (from the OS on first use), at most 2^32 items (the item index is one nonce word), and a
// call number of its own
static int rng_begin(sc_ctx* ctx, uint64_t count, const void* out, const char* who, uint64_t* call) {
  if (!ctx) return SC_ERR_ARG;
  if (!out) return fail(ctx, SC_ERR_ARG, "%s: no output array", who);
  if (count > 0xffffffffull) return fail(ctx, SC_ERR_ARG, "%s: at most 2^32 - 1 items per call", who);
  {
    std::lock_guard<std::mutex> lock(ctx->rng_seed_mutex);
    if (!ctx->rng_seeded) { int rc = sc_rng_seed(ctx, nullptr); if (rc) return rc; }
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  *call = ctx->rng_call.fetch_add(1);
  return SC_OK;
}

int sc_rng_bits(sc_ctx* ctx, int bits, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (ctx && bits <= 0) return fail(ctx, SC_ERR_ARG, "sc_rng_bits: bits must be positive");
  uint64_t call;
  int rc = rng_begin(ctx, count, out, "sc_rng_bits", &call); if (rc) return rc;
  if (launch_rng_bits(ctx->stream, ctx->rng_key, call, bits, (bits + 31) / 32, out, count)) return fail(ctx, SC_ERR_HIP, "sc_rng_bits: launch failed");
  return SC_OK;
}

int sc_rng_below(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, int nonzero, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (ctx && (!n_hptr || nwords <= 0)) return fail(ctx, SC_ERR_ARG, "sc_rng_below: bad bound");
  if (!ctx) return SC_ERR_ARG;
  Big n(n_hptr, n_hptr + nwords);
  const int nbits = big_bits(n);
  if (nbits == 0 || (nonzero && nbits == 1)) return fail(ctx, SC_ERR_ARG, "sc_rng_below: empty range");
  const int nw = (nbits + 31) / 32;
  if (nw != nwords) return fail(ctx, SC_ERR_ARG, "sc_rng_below: the bound must fill its top word (nwords = %d, bound has %d words)", nwords, nw);
  uint64_t call;
  int rc = rng_begin(ctx, count, out, "sc_rng_below", &call); if (rc) return rc;
  uint32_t* d_n = nullptr;
  rc = device_n_half(ctx, n_hptr, nwords, &d_n); if (rc) return rc;
  if (launch_rng_below(ctx->stream, ctx->rng_key, call, d_n, nbits, nw, nonzero ? 1 : 0, out, count)) return fail(ctx, SC_ERR_HIP, "sc_rng_below: launch failed");
  return SC_OK;
}

int sc_rng_coins(sc_ctx* ctx, uint64_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  uint64_t call;
  int rc = rng_begin(ctx, (count + 511) / 512, out, "sc_rng_coins", &call); if (rc) return rc;
  if (launch_rng_coins(ctx->stream, ctx->rng_key, call, out, count)) return fail(ctx, SC_ERR_HIP, "sc_rng_coins: launch failed");
  return SC_OK;
}

int sc_rng_permutations(sc_ctx* ctx, int k, int64_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (ctx && (k < 1 || k > 256)) return fail(ctx, SC_ERR_ARG, "sc_rng_permutations: 1 <= k <= 256");
  uint64_t call;
  int rc = rng_begin(ctx, count, out, "sc_rng_permutations", &call); if (rc) return rc;
  if (launch_rng_perm(ctx->stream, ctx->rng_key, call, k, out, count)) return fail(ctx, SC_ERR_HIP, "sc_rng_permutations: launch failed");
  return SC_OK;
}

int sc_peak_probe(sc_ctx* ctx, double* out_mac_per_s) {
  if (!ctx || !out_mac_per_s) return SC_ERR_ARG;
  DevBuf<uint32_t> d_out;
  const int grid = ctx->num_cu * 8;
  HIPCHK(ctx, hipMalloc((void**)&d_out.p, (size_t)grid * 256 * 4));
  LaunchTimer timer(ctx);
  const int iters = 40000;
  double best = 0;
  for (int rep = 0; rep < 4; rep++) {
    float ms = 0;
    int rc = timer.time([&] {
      return launch_peak_probe(ctx->stream, grid, d_out.p, 12345u, 67890u, iters) ? fail(ctx, SC_ERR_HIP, "sc_peak_probe: launch failed") : SC_OK;
    }, &ms); if (rc) return rc;
    double rate = (double)grid * 256 * (double)iters * 8 / (ms * 1e-3);
    if (rep > 0 && rate > best) best = rate;
  }
  *out_mac_per_s = best;
  return SC_OK;
}

int sc_table_traffic_probe(sc_ctx* ctx, int mod, const uint32_t* x, uint32_t* out, uint64_t count, int entries, int reads,
                           int* out_row_limbs) {
  if (!valid_mod(ctx, mod) || !x || !out || entries < 1 || entries > 64 || reads < 1 || reads > 4096)
    return fail(ctx, SC_ERR_ARG, "sc_table_traffic_probe: bad argument");
  const Mod& m = ctx->mods[mod];
  if (out_row_limbs) *out_row_limbs = m.S;
  std::string key = "tprobe:" + std::to_string(mod) + ":" + std::to_string(entries) + ":" + std::to_string(reads);
  const Prog* p;
  int rc = cached_prog(ctx, key, mod, [&](Builder& bd) {
    bd.loadw(0); bd.mul_const(0);                                   // x in Montgomery form
    for (int e = 0; e < entries; e++) bd.stt((uint32_t)e);          // `entries` rows written
    for (int r = 0; r < reads; r++) bd.loadt_tbl((uint32_t)((r * 7 + 3) % entries));   // `reads` rows read
    bd.redc(); bd.storew(1);
  }, &p); if (rc) return rc;
  VmExt ex[2] = {mk_ext(x, m.nwords, m.nwords), mk_ext(out, m.nwords, m.nwords)};
  return run_vm(ctx, mod, *p, ex, 2, count);
}

int sc_mac_counter(sc_ctx* ctx, int reset, double* out_macs) {
  if (!ctx) return SC_ERR_ARG;
  if (out_macs) *out_macs = ctx->mac_counter;
  if (reset) ctx->mac_counter = 0;
  return SC_OK;
}

}  // extern "C"

// Scheme-level entry points of the C ABI: what the reference's scheme objects and protocol steps do, ONE call each.
// The reference reaches its arithmetic through `ct.randomize()` (SC/keyholder.py:106-108, 126-128; SC/initiator.py:109,
// 153-154), `Paillier.decrypt` (SC/keyholder.py:195), `DGK.is_zero` (:249) and the operator algebra inside step_1 / step_4* /
// step_6 / step_7.  Rounds 1-2 exposed the primitives those decompose into; a maintainer binding them had to re-implement the
// key holder's CRT, the pair arithmetic's plumbing and the exponent reductions.  Here that composition lives in the library:
// a key object holds every derived modulus, exponent, constant and fixed-base table, and each entry point queues the same
// launches the Python layer used to compose -- identical residues.  Host code only.
#include "sc_host.h"

using namespace sc;
using namespace sc_host;

namespace {

int reg_exp(sc_ctx* ctx, const Big& e, int* out) { Big t = big_trimmed(e); return sc_exp_create(ctx, t.data(), (int)t.size(), out); }
int reg_const(sc_ctx* ctx, int mod, const Big& v, int* out) {
  return sc_const_create_cached(ctx, mod, big_fit(big_trimmed(v), std::max<size_t>(big_trimmed(v).size(), (size_t)ctx->mods[mod].nwords)), out);
}

struct PaillierHalf {            // one prime of the key holder's CRT
  int m1 = -1, m2 = -1;          // moduli p and p^2
  int exp_small = -1;            // q mod (p - 1): first stage of rho^N mod p^2
  int exp_p = -1, exp_pm1 = -1;  // p (second stage) and p - 1 (decryption)
  int cst_h = -1;                // h_p = L_p((N+1)^(p-1) mod p^2)^-1 mod p  (constant of m1)
};
struct PaillierKey {
  Big n; int nw = 0, hw = 0;
  int mod_n = -1, mod_n2 = -1, cst_n = -1, exp_n = -1;
  bool secret = false, crt = true, pairs = true;
  int exp_lambda = -1, cst_mu = -1;
  PaillierHalf hp, hq;
  int r_k = -1, r_negk = -1, r_mq = -1;   // recombination modulo p^2, q^2 -> N^2 (randomizers)
  int d_k = -1, d_negk = -1, d_mq = -1;   // recombination modulo p, q -> N (decryption)
};
struct DgkHalf { int m = -1, m_v = -1, fbt = -1, c_g = -1; };   // c_g: g mod p (mod q)
struct DgkKey {
  Big n, g, h, u; int nw = 0, rbits = 0, window = 0, t = 0;
  int mod_n = -1, cst_g = -1, cst_ginv = -1, fbt_h = -1;
  bool secret = false, crt = true;
  int mod_p = -1, exp_vp = -1, exp_one = -1;
  DgkHalf hp, hq;
  int c_k = -1, c_negk = -1, c_mq = -1;   // recombination modulo p, q -> n
};

}  // namespace

// (the key tables live in the context; declared here, stored through the pointers below)
struct sc_scheme_keys {
  std::vector<PaillierKey> paillier; std::vector<DgkKey> dgk;
  std::map<int, int> pow2_exps;      // bits -> the registered exponent 2^bits (the selection's Horner chain)
  uint32_t* select_verdict = nullptr; // pinned word the key holder's split kernel writes (sc_keyholder_select_mult)
  uint32_t* div_verdict = nullptr;    // pinned word k_divmod_words sets on a zero divisor (sc_plain_divmod); zero whenever nothing is pending
  ~sc_scheme_keys() { if (select_verdict) (void)hipHostFree(select_verdict); if (div_verdict) (void)hipHostFree(div_verdict); }
};

void sc_host::free_scheme_keys(void* p) { delete (sc_scheme_keys*)p; }

namespace {

sc_scheme_keys* keys_of(sc_ctx* ctx) {
  if (!ctx->scheme_keys) ctx->scheme_keys = new sc_scheme_keys();
  return (sc_scheme_keys*)ctx->scheme_keys;
}
PaillierKey* paillier_key(sc_ctx* ctx, int key) {
  if (!ctx || !ctx->scheme_keys) return nullptr;
  auto& v = ((sc_scheme_keys*)ctx->scheme_keys)->paillier;
  return (key >= 0 && key < (int)v.size()) ? &v[key] : nullptr;
}
DgkKey* dgk_key(sc_ctx* ctx, int key) {
  if (!ctx || !ctx->scheme_keys) return nullptr;
  auto& v = ((sc_scheme_keys*)ctx->scheme_keys)->dgk;
  return (key >= 0 && key < (int)v.size()) ? &v[key] : nullptr;
}

enum SchemeTmp { TMP_S_A = 40, TMP_S_B, TMP_S_C, TMP_S_D, TMP_S_E, TMP_S_F, TMP_S_G, TMP_S_H, TMP_S_I };

// rho^N mod N^2 for the key holder: ((rho mod p)^(q mod p-1) mod p)^p mod p^2 per prime, recombined (identical integers)
int paillier_crt_pow_n(sc_ctx* ctx, const PaillierKey& k, const uint32_t* rho, uint32_t* out, uint64_t count) {
  uint32_t *y, *part_p, *part_q;
  int rc = tmp_words(ctx, TMP_S_A, count * k.hw, &y); if (rc) return rc;
  rc = tmp_words(ctx, TMP_S_B, count * 2 * k.hw, &part_p); if (rc) return rc;
  rc = tmp_words(ctx, TMP_S_C, count * 2 * k.hw, &part_q); if (rc) return rc;
  AuxFork fork;
  const bool forked = small_enough_to_fork(ctx, ctx->mods[k.hp.m1], count);
  for (int pass = 0; pass < 2; pass++) {
    const int side = forked ? 1 - pass : pass;       // forked: the q-side is queued first, on the second stream, the p-side beside it
    const PaillierHalf& h = side ? k.hq : k.hp;
    uint32_t* part = side ? part_q : part_p;
    if (forked && pass == 0) {
      rc = fork.begin(ctx); if (rc) return rc;
      rc = tmp_words(ctx, TMP_S_A, count * k.hw, &y); if (rc) return rc;
    }
    if (forked && pass == 1) {
      rc = fork.suspend(); if (rc) return rc;
      rc = tmp_words(ctx, TMP_S_A, count * k.hw, &y); if (rc) return rc;
    }
    rc = sc_modexp_shared(ctx, h.m1, h.exp_small, rho, k.nw, nullptr, y, count); if (rc) return rc;       // wide operand reduced mod p
    if (k.pairs && sc_mod_supports_sq(ctx, h.m1) == 1) {
      rc = sc_modexp_shared_sq(ctx, h.m1, h.m2, h.exp_p, y, k.hw, nullptr, part, count);
    } else {
      rc = sc_modexp_shared(ctx, h.m2, h.exp_p, y, k.hw, nullptr, part, count);
    }
    if (rc) return rc;
  }
  rc = fork.join(); if (rc) return rc;
  return sc_crt_combine(ctx, k.hp.m2, k.mod_n2, k.r_k, k.r_negk, k.r_mq, part_p, 2 * k.hw, part_q, 2 * k.hw, out, count);
}

}  // namespace

extern "C" {

int sc_paillier_key_create(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, const uint32_t* p_hptr, const uint32_t* q_hptr, int pwords,
                           int flags, int* out_key) {
  if (!ctx || !n_hptr || nwords <= 0 || !out_key || ((p_hptr == nullptr) != (q_hptr == nullptr)) || (p_hptr && pwords <= 0))
    return fail(ctx, SC_ERR_ARG, "sc_paillier_key_create: bad argument");
  PaillierKey k;
  k.n.assign(n_hptr, n_hptr + nwords);
  k.nw = nwords;
  k.crt = !(flags & SC_KEY_NO_CRT);
  k.pairs = !(flags & SC_KEY_NO_PAIRS);
  const Big n2 = big_fit(big_mul(k.n, k.n), 2 * (size_t)nwords);
  int rc = sc_mod_create(ctx, k.n.data(), nwords, &k.mod_n); if (rc) return rc;
  rc = sc_mod_create(ctx, n2.data(), 2 * nwords, &k.mod_n2); if (rc) return rc;
  rc = reg_const(ctx, k.mod_n2, k.n, &k.cst_n); if (rc) return rc;
  rc = reg_exp(ctx, k.n, &k.exp_n); if (rc) return rc;
  if (p_hptr) {
    const Big p = big_trimmed(Big(p_hptr, p_hptr + pwords)), q = big_trimmed(Big(q_hptr, q_hptr + pwords));
    {
      Big pq = big_fit(big_trimmed(big_mul(p, q)), (size_t)nwords);
      if (big_trimmed(big_mul(p, q)).size() > (size_t)nwords || big_cmp(pq, k.n) != 0) return fail(ctx, SC_ERR_ARG, "sc_paillier_key_create: p * q != n");
    }
    k.secret = true;
    k.hw = (std::max(big_bits(p), big_bits(q)) + 31) / 32;
    const Big pm1 = big_sub_small(p, 1), qm1 = big_sub_small(q, 1);
    // lambda = (p - 1)(q - 1), mu = lambda^-1 mod N  (literal decryption)
    const Big lambda = big_trimmed(big_mul(pm1, qm1));
    rc = reg_exp(ctx, lambda, &k.exp_lambda); if (rc) return rc;
    const Big mu = big_modinv_odd(lambda, k.n);
    if (mu.empty()) return fail(ctx, SC_ERR_ARG, "sc_paillier_key_create: lambda is not invertible modulo n");
    rc = reg_const(ctx, k.mod_n, mu, &k.cst_mu); if (rc) return rc;
    for (int side = 0; side < 2; side++) {
      const Big& pr = side ? q : p; const Big& other = side ? p : q; const Big& prm1 = side ? qm1 : pm1;
      PaillierHalf& h = side ? k.hq : k.hp;
      const Big pr_w = big_fit(pr, (size_t)k.hw), pr2 = big_fit(big_mul(pr, pr), 2 * (size_t)k.hw);
      rc = sc_mod_create(ctx, pr_w.data(), k.hw, &h.m1); if (rc) return rc;
      rc = sc_mod_create(ctx, pr2.data(), 2 * k.hw, &h.m2); if (rc) return rc;
      rc = reg_exp(ctx, big_mod(other, big_trimmed(prm1)), &h.exp_small); if (rc) return rc;
      rc = reg_exp(ctx, pr, &h.exp_p); if (rc) return rc;
      rc = reg_exp(ctx, prm1, &h.exp_pm1); if (rc) return rc;
      // (N+1)^(p-1) = 1 + (p-1) N (mod p^2), so L_p of it is (p-1) q = -q (mod p):  h_p = (-q)^-1 = p - (q^-1 mod p)
      const Big qinv = big_modinv_odd(other, pr_w);
      if (qinv.empty()) return fail(ctx, SC_ERR_ARG, "sc_paillier_key_create: p and q are not coprime");
      Big hval = pr_w; big_sub(hval, qinv);
      rc = reg_const(ctx, h.m1, hval, &h.cst_h); if (rc) return rc;
    }
    // recombination constants: x = a_q + m_q ((a_p - a_q) m_q^-1 mod m_p)
    {
      const Big p2 = big_fit(big_mul(p, p), 2 * (size_t)k.hw), q2 = big_trimmed(big_mul(q, q));
      const Big kk = big_modinv_odd(q2, p2);
      if (kk.empty()) return fail(ctx, SC_ERR_ARG, "sc_paillier_key_create: q^2 is not invertible modulo p^2");
      Big neg = p2; big_sub(neg, kk);
      rc = reg_const(ctx, k.hp.m2, kk, &k.r_k); if (rc) return rc;
      rc = reg_const(ctx, k.hp.m2, neg, &k.r_negk); if (rc) return rc;
      rc = reg_const(ctx, k.mod_n2, q2, &k.r_mq); if (rc) return rc;
      const Big pw = big_fit(p, (size_t)k.hw);
      const Big kd = big_modinv_odd(q, pw);
      Big negd = pw; big_sub(negd, kd);
      rc = reg_const(ctx, k.hp.m1, kd, &k.d_k); if (rc) return rc;
      rc = reg_const(ctx, k.hp.m1, negd, &k.d_negk); if (rc) return rc;
      rc = reg_const(ctx, k.mod_n, q, &k.d_mq); if (rc) return rc;
    }
  }
  keys_of(ctx)->paillier.push_back(k);
  *out_key = (int)keys_of(ctx)->paillier.size() - 1;
  // the key holder's CRT runs its half-size exponentiations under the one-lane policy: measure that policy's constants now (once
  // per device and process), not inside the first step
  if (k.secret && k.crt && ctx->onelane_mode == 1 && k.hw <= 32) (void)onelane_cal(ctx);
  return SC_OK;
}

int sc_paillier_key_mods(sc_ctx* ctx, int key, int* out_mod_n, int* out_mod_n2) {
  const PaillierKey* k = paillier_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_paillier_key_mods: bad key");
  if (out_mod_n) *out_mod_n = k->mod_n;
  if (out_mod_n2) *out_mod_n2 = k->mod_n2;
  return SC_OK;
}

int sc_paillier_encrypt(sc_ctx* ctx, int key, const uint32_t* m, int m_words, int negate, uint32_t* out, uint64_t count) {
  const PaillierKey* k = paillier_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_paillier_encrypt: bad key");
  return negate ? sc_paillier_encrypt_raw_neg(ctx, k->mod_n2, k->cst_n, m, m_words, out, count)
                : sc_paillier_encrypt_raw(ctx, k->mod_n2, k->cst_n, m, m_words, out, count);
}

int sc_paillier_randomize(sc_ctx* ctx, int key, const uint32_t* c, const uint32_t* rho, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, key);
  if (!kp || !rho || !out) return fail(ctx, SC_ERR_ARG, "sc_paillier_randomize: bad argument");
  const PaillierKey k = *kp;    // (the key table may grow while programs are built: work on a copy)
  if (k.secret && k.crt) {
    if (!c) return paillier_crt_pow_n(ctx, k, rho, out, count);
    uint32_t* rn;
    int rc = tmp_words(ctx, TMP_S_D, count * 2 * k.nw, &rn); if (rc) return rc;
    rc = paillier_crt_pow_n(ctx, k, rho, rn, count); if (rc) return rc;
    return sc_modmul(ctx, k.mod_n2, c, 2 * k.nw, rn, 2 * k.nw, out, count);
  }
  if (k.pairs && sc_mod_supports_sq(ctx, k.mod_n) == 1)
    return sc_modexp_shared_sq(ctx, k.mod_n, k.mod_n2, k.exp_n, rho, k.nw, c, out, count);     // arithmetic modulo N only
  return sc_modexp_shared(ctx, k.mod_n2, k.exp_n, rho, k.nw, c, out, count);
}

int sc_paillier_sum_axis(sc_ctx* ctx, int key, const uint32_t* c, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out) {
  const PaillierKey* k = paillier_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_paillier_sum_axis: bad key");
  return sc_modprod_axis(ctx, k->mod_n2, c, outer, K, inner, out);
}

int sc_paillier_cumsum_axis(sc_ctx* ctx, int key, const uint32_t* c, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out) {
  const PaillierKey* k = paillier_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_paillier_cumsum_axis: bad key");
  return sc_modscan_axis(ctx, k->mod_n2, c, outer, K, inner, out);
}

int sc_paillier_linear_axis(sc_ctx* ctx, int key, const uint32_t* c, uint64_t outer, uint64_t K, uint64_t inner, const uint64_t* w_host, uint64_t J,
                            uint32_t* out) {
  const PaillierKey* k = paillier_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_paillier_linear_axis: bad key");
  return sc_modlin_axis(ctx, k->mod_n2, c, outer, K, inner, w_host, J, out);
}

int sc_paillier_decrypt(sc_ctx* ctx, int key, const uint32_t* c, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, key);
  if (!kp || !c || !out) return fail(ctx, SC_ERR_ARG, "sc_paillier_decrypt: bad argument");
  if (!kp->secret) return fail(ctx, SC_ERR_ARG, "sc_paillier_decrypt: this key has no secret part");
  const PaillierKey k = *kp;
  int rc;
  if (!k.crt) {
    uint32_t* x;
    rc = tmp_words(ctx, TMP_S_A, count * 2 * k.nw, &x); if (rc) return rc;
    if (k.pairs && sc_mod_supports_sq(ctx, k.mod_n) == 1) rc = sc_modexp_shared_sq(ctx, k.mod_n, k.mod_n2, k.exp_lambda, c, 2 * k.nw, nullptr, x, count);
    else rc = sc_modexp_shared(ctx, k.mod_n2, k.exp_lambda, c, 2 * k.nw, nullptr, x, count);
    if (rc) return rc;
    return sc_paillier_l_mul(ctx, k.mod_n, k.cst_mu, x, 2 * k.nw, out, count);
  }
  // m_p = L_p(c^(p-1) mod p^2) h_p mod p, likewise q, recombined modulo N
  uint32_t *x, *m_p, *m_q;
  rc = tmp_words(ctx, TMP_S_A, count * 2 * k.hw, &x); if (rc) return rc;
  rc = tmp_words(ctx, TMP_S_B, count * k.hw, &m_p); if (rc) return rc;
  rc = tmp_words(ctx, TMP_S_C, count * k.hw, &m_q); if (rc) return rc;
  AuxFork fork;
  const bool forked = small_enough_to_fork(ctx, ctx->mods[k.hp.m1], count);
  for (int pass = 0; pass < 2; pass++) {
    const int side = forked ? 1 - pass : pass;       // forked: c^(q-1) mod q^2 first, on the second stream; c^(p-1) mod p^2 beside it
    const PaillierHalf& h = side ? k.hq : k.hp;
    if (forked && pass == 0) {
      rc = fork.begin(ctx); if (rc) return rc;
      rc = tmp_words(ctx, TMP_S_A, count * 2 * k.hw, &x); if (rc) return rc;
    }
    if (forked && pass == 1) {
      rc = fork.suspend(); if (rc) return rc;
      rc = tmp_words(ctx, TMP_S_A, count * 2 * k.hw, &x); if (rc) return rc;
    }
    if (k.pairs && sc_mod_supports_sq(ctx, h.m1) == 1) rc = sc_modexp_shared_sq(ctx, h.m1, h.m2, h.exp_pm1, c, 2 * k.nw, nullptr, x, count);
    else rc = sc_modexp_shared(ctx, h.m2, h.exp_pm1, c, 2 * k.nw, nullptr, x, count);
    if (rc) return rc;
    rc = sc_paillier_l_mul(ctx, h.m1, h.cst_h, x, 2 * k.hw, side ? m_q : m_p, count); if (rc) return rc;
  }
  rc = fork.join(); if (rc) return rc;
  return sc_crt_combine(ctx, k.hp.m1, k.mod_n, k.d_k, k.d_negk, k.d_mq, m_p, k.hw, m_q, k.hw, out, count);
}

int sc_dgk_key_create(sc_ctx* ctx, const uint32_t* n_hptr, const uint32_t* g_hptr, const uint32_t* h_hptr, int nwords, const uint32_t* u_hptr,
                      int uwords, int t_bits, const uint32_t* p_hptr, const uint32_t* q_hptr, int pwords, const uint32_t* vp_hptr,
                      const uint32_t* vq_hptr, int vwords, int randomizer_bits, int window, int flags, sc_ctx* table_src_ctx,
                      int table_src_key, int* out_key) {
  if (!ctx || !n_hptr || !g_hptr || !h_hptr || nwords <= 0 || !u_hptr || uwords <= 0 || randomizer_bits <= 0 || window < 1 || window > 24 || !out_key)
    return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: bad argument");
  const bool secret = p_hptr != nullptr;
  if (secret && (!q_hptr || !vp_hptr || !vq_hptr || pwords <= 0 || vwords <= 0)) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: incomplete secret key");
  DgkKey k;
  k.n.assign(n_hptr, n_hptr + nwords); k.g.assign(g_hptr, g_hptr + nwords); k.h.assign(h_hptr, h_hptr + nwords);
  k.u.assign(u_hptr, u_hptr + uwords);
  k.nw = nwords; k.rbits = randomizer_bits; k.window = window; k.t = t_bits; k.secret = secret; k.crt = !(flags & SC_KEY_NO_CRT);
  const DgkKey* src = nullptr;
  if (table_src_ctx) {
    src = dgk_key(table_src_ctx, table_src_key);
    if (!src || src->n != k.n || src->h != k.h || src->window != window || src->rbits != randomizer_bits || src->secret != secret || src->crt != k.crt)
      return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: tables can only be shared between keys with the same modulus, h, window and randomizer width");
  }
  int rc = sc_mod_create(ctx, k.n.data(), nwords, &k.mod_n); if (rc) return rc;
  rc = reg_const(ctx, k.mod_n, k.g, &k.cst_g); if (rc) return rc;
  const Big ginv = big_modinv_odd(k.g, k.n);
  if (ginv.empty()) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: g is not invertible modulo n");
  rc = reg_const(ctx, k.mod_n, ginv, &k.cst_ginv); if (rc) return rc;
  auto table = [&](int mod, const Big& base, int exp_bits, int w, int src_fbt, int* out_fbt) -> int {
    if (src) return sc_fbt_import(ctx, mod, table_src_ctx, src_fbt, out_fbt);
    const Big b = big_fit(base, (size_t)ctx->mods[mod].nwords);
    return sc_fbt_create(ctx, mod, b.data(), exp_bits, w, out_fbt);
  };
  if (!secret || !k.crt) {     // Alice -- and a key holder told not to use CRT -- randomize modulo n with the table for h
    rc = table(k.mod_n, k.h, randomizer_bits, window, src ? src->fbt_h : -1, &k.fbt_h); if (rc) return rc;
  }
  if (secret) {
    const Big p = big_trimmed(Big(p_hptr, p_hptr + pwords)), q = big_trimmed(Big(q_hptr, q_hptr + pwords));
    const Big vp = big_trimmed(Big(vp_hptr, vp_hptr + vwords)), vq = big_trimmed(Big(vq_hptr, vq_hptr + vwords));
    // a secret key that does not belong to the public one would silently give randomizers that are not h^r mod n (the CRT halves
    // reduce r modulo v_p, v_q) and zero tests that test nothing: check p q = n and that h has order dividing v_p (v_q) modulo p (q)
    {
      const Big pq = big_trimmed(big_mul(p, q));
      if (pq.size() > (size_t)nwords || big_cmp(big_fit(pq, (size_t)nwords), k.n) != 0) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: p * q != n");
      if (!big_is_one(big_powmod(k.h, vp, p)) || !big_is_one(big_powmod(k.h, vq, q)))
        return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: h^v_p mod p and h^v_q mod q must be 1 (the secret key does not match h)");
    }
    rc = sc_mod_create(ctx, p.data(), (int)p.size(), &k.mod_p); if (rc) return rc;
    rc = reg_exp(ctx, vp, &k.exp_vp); if (rc) return rc;
    if (k.crt) {
      Big one(1, 1);
      rc = reg_exp(ctx, one, &k.exp_one); if (rc) return rc;
      for (int side = 0; side < 2; side++) {
        const Big& pr = side ? q : p; const Big& v = side ? vq : vp;
        DgkHalf& h = side ? k.hq : k.hp;
        rc = sc_mod_create(ctx, pr.data(), (int)pr.size(), &h.m); if (rc) return rc;
        if (!(v[0] & 1)) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: v_p, v_q must be odd (they are primes)");
        rc = sc_mod_create(ctx, v.data(), (int)v.size(), &h.m_v); if (rc) return rc;
        // h has order v_p modulo p: h^r mod p = (h mod p)^(r mod v_p) -- a t-bit exponent and a half-size modulus
        rc = table(h.m, big_mod(k.h, pr), big_bits(v), std::min(window, 20), src ? (side ? src->hq.fbt : src->hp.fbt) : -1, &h.fbt); if (rc) return rc;
        rc = reg_const(ctx, h.m, big_mod(k.g, pr), &h.c_g); if (rc) return rc;
      }
      const Big kk = big_modinv_odd(q, p);
      if (kk.empty()) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_create: p and q are not coprime");
      Big neg = big_fit(p, kk.size()); big_sub(neg, kk);
      rc = reg_const(ctx, k.hp.m, kk, &k.c_k); if (rc) return rc;
      rc = reg_const(ctx, k.hp.m, neg, &k.c_negk); if (rc) return rc;
      rc = reg_const(ctx, k.mod_n, q, &k.c_mq); if (rc) return rc;
    }
  }
  keys_of(ctx)->dgk.push_back(k);
  *out_key = (int)keys_of(ctx)->dgk.size() - 1;
  if (secret && ctx->onelane_mode == 1 && pwords <= 32) (void)onelane_cal(ctx);      // the zero tests run under the one-lane policy
  return SC_OK;
}

int sc_dgk_key_info(sc_ctx* ctx, int key, int* out_mod_n, int* out_mod_p, uint64_t* out_table_bytes) {
  const DgkKey* k = dgk_key(ctx, key);
  if (!k) return fail(ctx, SC_ERR_ARG, "sc_dgk_key_info: bad key");
  if (out_mod_n) *out_mod_n = k->mod_n;
  if (out_mod_p) *out_mod_p = k->mod_p;
  if (out_table_bytes) {
    uint64_t total = 0, b = 0;
    for (int f : {k->fbt_h, k->hp.fbt, k->hq.fbt})
      if (f >= 0 && sc_fbt_bytes(ctx, f, &b) == SC_OK) total += b;
    *out_table_bytes = total;
  }
  return SC_OK;
}

// h^r [* c] mod n; `bits` (nullable): additionally times g where bits[i] != 0 (the unrandomized encryption of a bit)
static int dgk_randomize_impl(sc_ctx* ctx, const DgkKey& k, const uint32_t* c, const uint8_t* bits, const uint32_t* r, int ewords, uint32_t* out, uint64_t count) {
  int rc;
  if (!k.secret || !k.crt) {
    rc = sc_fixedbase_pow(ctx, k.fbt_h, r, ewords, c, out, count); if (rc) return rc;
  } else if (!c) {
    // Key holder, CRT (SC/keyholder.py:106-108): h^r mod q, then h^r mod p with the first half of the recombination in the same
    // launch -- t = (a_p - a_q) q^-1 mod p leaves the fixed-base program instead of a_p --, then a_q + q t: five launches over the
    // l + 1 values of every comparison instead of seven (each pass over the batch costs a load, a canonical store and the launch's
    // ramp, whatever it multiplies).  The factor g^bit of the unrandomized encryption enters the two halves -- times g mod q, g mod p
    // where the bit is set, two half-size products -- instead of the recombined value (one full-size product).  Same residues.
    uint32_t *r_red, *tq, *a_q;
    const int pw = ctx->mods[k.hp.m].nwords, qw = ctx->mods[k.hq.m].nwords;
    const int vpw = ctx->mods[k.hp.m_v].nwords, vqw = ctx->mods[k.hq.m_v].nwords;
    rc = tmp_words(ctx, TMP_S_A, count * std::max(vpw, vqw), &r_red); if (rc) return rc;
    rc = tmp_words(ctx, TMP_S_B, count * pw, &tq); if (rc) return rc;
    rc = tmp_words(ctx, TMP_S_C, count * qw, &a_q); if (rc) return rc;
    rc = sc_modexp_shared(ctx, k.hq.m_v, k.exp_one, r, ewords, nullptr, r_red, count); if (rc) return rc;                 // r mod v_q
    if (!bits) {
      rc = sc_fixedbase_pow(ctx, k.hq.fbt, r_red, vqw, nullptr, a_q, count); if (rc) return rc;                             // a_q = h^r mod q
    } else {
      const Fbt f = ctx->fbts[k.hq.fbt];
      const Prog* pr;
      rc = cached_prog(ctx, "fbcrt0:" + std::to_string(k.hq.fbt) + ":" + std::to_string(k.hq.c_g), k.hq.m, [&](Builder& bd) {
        const int cg = bd.use_const(k.hq.c_g);
        bd.loadt_fbt(0, 0, f.window, 0);
        for (int j = 1; j < f.nwin; j++) bd.mul_fbt(0, j * f.window, f.window, j);
        bd.mul_constsel(2, 1, cg);                                                           // times g mod q where the bit is set
        bd.redc(); bd.storew(1);                                                             // a_q = g^bit h^r mod q
      }, &pr); if (rc) return rc;
      VmExt ex[3] = {mk_ext(r_red, vqw, vqw), mk_ext(a_q, qw, qw), mk_ext(bits, 0, 0)};
      rc = run_vm(ctx, k.hq.m, *pr, ex, 3, count, f.d_rows); if (rc) return rc;
    }
    rc = sc_modexp_shared(ctx, k.hp.m_v, k.exp_one, r, ewords, nullptr, r_red, count); if (rc) return rc;                 // r mod v_p
    {
      const Fbt f = ctx->fbts[k.hp.fbt];
      const Mod mp = ctx->mods[k.hp.m];
      std::string key = "fbcrt1:" + std::to_string(k.hp.fbt) + ":" + std::to_string(k.c_k) + ":" + std::to_string(k.c_negk) + ":" + std::to_string(qw) + (bits ? ":g" + std::to_string(k.hp.c_g) : "");
      const Prog* pr;
      rc = cached_prog(ctx, key, k.hp.m, [&](Builder& bd) -> int {
        const int ck = bd.use_const(k.c_k), cn = bd.use_const(k.c_negk);
        int kc = -1;
        if (qw > mp.nwords) { int cid; int rc = get_const_kred(ctx, k.hp.m, &cid); if (rc) return rc; kc = bd.use_const(cid); }
        bd.loadt_fbt(0, 0, f.window, 0);
        for (int j = 1; j < f.nwin; j++) bd.mul_fbt(0, j * f.window, f.window, j);
        if (bits) bd.mul_constsel(3, 1, bd.use_const(k.hp.c_g));                          // times g mod p where the bit is set
        bd.redc();                                                                         // a_p = [g^bit] h^r mod p
        bd.mul_const(ck); bd.stt(0);                                                       // a_p k,  k = q^-1 mod p
        if (qw > mp.nwords) emit_load_reduced(ctx, mp, bd, 1, qw, kc); else bd.loadw(1, 0, 0, qw);
        bd.mul_const(cn); bd.addt(0);                                                      // + a_q (p - k)
        bd.storew(2);
        return SC_OK;
      }, &pr); if (rc) return rc;
      VmExt ex[4] = {mk_ext(r_red, vpw, vpw), mk_ext(a_q, qw, qw), mk_ext(tq, mp.nwords, mp.nwords), mk_ext(bits, 0, 0)};
      rc = run_vm(ctx, k.hp.m, *pr, ex, bits ? 4 : 3, count, f.d_rows); if (rc) return rc;
    }
    {
      const Mod mn = ctx->mods[k.mod_n];
      std::string key = "fbcrt2:" + std::to_string(k.mod_n) + ":" + std::to_string(k.c_mq) + ":" + std::to_string(pw) + ":" + std::to_string(qw);
      const Prog* pr;
      rc = cached_prog(ctx, key, k.mod_n, [&](Builder& bd) {
        const int cm = bd.use_const(k.c_mq);
        bd.loadw(0, 0, 0, pw); bd.mul_const(cm);                                           // q t  (< p q: exact)
        bd.addw(1, 0, 0, qw);                                                              // + a_q = [g^bit] h^r mod n
        bd.storew(2);
      }, &pr); if (rc) return rc;
      VmExt ex[3] = {mk_ext(tq, pw, pw), mk_ext(a_q, qw, qw), mk_ext(out, mn.nwords, mn.nwords)};
      return run_vm(ctx, k.mod_n, *pr, ex, 3, count);
    }
  } else {
    uint32_t *r_red, *part_p, *part_q;
    const int pw = ctx->mods[k.hp.m].nwords, qw = ctx->mods[k.hq.m].nwords;
    const int vpw = ctx->mods[k.hp.m_v].nwords, vqw = ctx->mods[k.hq.m_v].nwords;
    rc = tmp_words(ctx, TMP_S_A, count * std::max(vpw, vqw), &r_red); if (rc) return rc;
    rc = tmp_words(ctx, TMP_S_B, count * pw, &part_p); if (rc) return rc;
    rc = tmp_words(ctx, TMP_S_C, count * qw, &part_q); if (rc) return rc;
    for (int side = 0; side < 2; side++) {
      const DgkHalf& h = side ? k.hq : k.hp;
      rc = sc_modexp_shared(ctx, h.m_v, k.exp_one, r, ewords, nullptr, r_red, count); if (rc) return rc;            // r mod v (wide operand reduced)
      rc = sc_fixedbase_pow(ctx, h.fbt, r_red, side ? vqw : vpw, nullptr, side ? part_q : part_p, count); if (rc) return rc;
    }
    uint32_t* hr = out;
    if (c) { rc = tmp_words(ctx, TMP_S_D, count * k.nw, &hr); if (rc) return rc; }
    rc = sc_crt_combine(ctx, k.hp.m, k.mod_n, k.c_k, k.c_negk, k.c_mq, part_p, pw, part_q, qw, hr, count); if (rc) return rc;
    if (c) { rc = sc_modmul(ctx, k.mod_n, c, k.nw, hr, k.nw, out, count); if (rc) return rc; }
  }
  if (bits) return sc_modmul_const_sel(ctx, k.mod_n, out, -1, k.cst_g, bits, out, count);
  return SC_OK;
}

int sc_dgk_randomize(sc_ctx* ctx, int key, const uint32_t* c, const uint32_t* r, int ewords, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const DgkKey* kp = dgk_key(ctx, key);
  if (!kp || !r || ewords <= 0 || !out) return fail(ctx, SC_ERR_ARG, "sc_dgk_randomize: bad argument");
  const DgkKey k = *kp;
  return dgk_randomize_impl(ctx, k, c, nullptr, r, ewords, out, count);
}

int sc_dgk_encrypt_bits_randomized(sc_ctx* ctx, int key, const uint8_t* bits, const uint32_t* r, int ewords, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const DgkKey* kp = dgk_key(ctx, key);
  if (!kp || !bits || !r || ewords <= 0 || !out) return fail(ctx, SC_ERR_ARG, "sc_dgk_encrypt_bits_randomized: bad argument");
  const DgkKey k = *kp;
  return dgk_randomize_impl(ctx, k, nullptr, bits, r, ewords, out, count);
}

int sc_dgk_is_zero(sc_ctx* ctx, int key, const uint32_t* c, uint8_t* flags, uint64_t count) {
  const DgkKey* k = dgk_key(ctx, key);
  if (!k || !k->secret) return fail(ctx, SC_ERR_ARG, "sc_dgk_is_zero: needs the secret key");
  return sc_modexp_shared_isone(ctx, k->mod_p, k->exp_vp, c, k->nw, flags, count);
}

int sc_dgk_any_zero(sc_ctx* ctx, int key, const uint32_t* c, int planes, uint64_t inner, uint64_t* any_flags) {
  const DgkKey* k = dgk_key(ctx, key);
  if (!k || !k->secret || planes <= 0) return fail(ctx, SC_ERR_ARG, "sc_dgk_any_zero: needs the secret key");
  return sc_modexp_shared_isone_any(ctx, k->mod_p, k->exp_vp, c, k->nw, inner, any_flags, (uint64_t)planes * inner);
}

// ---- protocol steps ----------------------------------------------------------------------------------------------------------
int sc_initiator_step1(sc_ctx* ctx, int paillier_key_id, int l, const uint32_t* x_enc, const uint32_t* y_enc, const uint32_t* r,
                       const uint32_t* rho_z, int flags, uint32_t* z_out, uint64_t* alpha, uint64_t* alpha_tilde, uint64_t* rsmall,
                       uint32_t* rshift, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !x_enc || !y_enc || !r || !z_out || !alpha || !alpha_tilde || !rsmall || !rshift || l <= 0 || l > SC_MAX_L)
    return fail(ctx, SC_ERR_ARG, "sc_initiator_step1: bad argument");
  const PaillierKey k = *kp;
  if (l + 3 >= big_bits(k.n) - 1) return fail(ctx, SC_ERR_ARG, "sc_initiator_step1: 2^(l+2) must be below N / 2 (SC/initiator.py:249)");
  uint32_t *m1, *xinv, *t;
  int rc = tmp_words(ctx, TMP_S_E, count * (k.nw + 1), &m1); if (rc) return rc;
  rc = tmp_words(ctx, TMP_S_F, count * 2 * k.nw, &xinv); if (rc) return rc;
  rc = sc_plain_alice(ctx, r, k.n.data(), k.nw, l, count, m1, alpha, alpha_tilde, rsmall, rshift); if (rc) return rc;
  int64_t bad = -1;
  rc = sc_modinv(ctx, k.mod_n2, x_enc, xinv, count, &bad);
  if (rc) return rc;
  // one launch for the rest of step 1: [[y]] [[x]]^-1 [[2^l + r]] (SC/initiator.py:254-256), times the finished randomizer when it
  // was computed ahead of time.  Same products as the separate modmul / encrypt launches, identical residues.
  const bool ready = rho_z && (flags & SC_STEP_RANDOMIZERS_READY);
  const bool fused_out = !rho_z || ready;                 // else the product goes to a temporary and .randomize() (:109) finishes
  uint32_t* dst = z_out;
  if (!fused_out) { rc = tmp_words(ctx, TMP_S_G, count * 2 * k.nw, &t); if (rc) return rc; dst = t; }
  const int w2 = ctx->mods[k.mod_n2].nwords;
  const Prog* p;
  rc = cached_prog(ctx, "step1:" + std::to_string(k.mod_n2) + ":" + std::to_string(k.cst_n) + (ready ? ":r" : ""), k.mod_n2, [&](Builder& bd) {
    const int cn = bd.use_const(k.cst_n);
    bd.loadw(0); bd.mul_const(0); bd.mul_extw(1);        // [[y]] [[x]]^-1
    bd.mul_const(0); bd.stt(0);                          // ... in Montgomery form
    bd.loadw(2, 0, 0, k.nw + 1); bd.mul_const(cn); bd.add1();          // [[2^l + r]] = 1 + (2^l + r) N  (mod N^2)
    bd.mul_tbl(0);
    if (ready) { bd.mul_const(0); bd.mul_extw(4); }      // times rho_z^N
    bd.storew(3);
  }, &p); if (rc) return rc;
  VmExt ex[5] = {mk_ext(y_enc, w2, w2), mk_ext(xinv, w2, w2), mk_ext(m1, k.nw + 1, k.nw + 1),
                 mk_ext(dst, w2, w2), mk_ext(ready ? rho_z : nullptr, w2, w2)};
  rc = run_vm(ctx, k.mod_n2, *p, ex, 5, count); if (rc) return rc;
  if (fused_out) return SC_OK;
  return sc_paillier_randomize(ctx, paillier_key_id, t, rho_z, z_out, count);                                         // .randomize() (:109)
}

int sc_initiator_step4i(sc_ctx* ctx, int dgk_key_id, int l, const uint32_t* c_in, const uint32_t* rhos, int rho_words, const int64_t* permutation,
                        const uint32_t* r_rand, int r_words, int flags, uint32_t* c_out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const DgkKey* kp = dgk_key(ctx, dgk_key_id);
  if (!kp || l <= 0 || l > SC_MAX_L || !c_in || !rhos || rho_words <= 0 || !c_out || (r_rand && r_words <= 0))
    return fail(ctx, SC_ERR_ARG, "sc_initiator_step4i: bad argument");
  const DgkKey k = *kp;
  const bool ready = r_rand && (flags & SC_STEP_RANDOMIZERS_READY);     // r_rand holds h^r itself ([l+1][count][nwords]), computed ahead
  if (r_rand && !ready && k.fbt_h < 0) return fail(ctx, SC_ERR_ARG, "sc_initiator_step4i: this key has no table for h modulo n (key holder with CRT)");
  const uint64_t planes = (uint64_t)l + 1, items = planes * count;
  const int ubits = big_bits(big_sub_small(k.u, 1));
  const int fbt = (r_rand && !ready) ? k.fbt_h : -1;
  const uint32_t* e2 = ready ? nullptr : r_rand;
  const uint32_t* premul = ready ? r_rand : nullptr;
  if (!permutation) return modexp_var_impl(ctx, k.mod_n, c_in, rhos, rho_words, ubits, fbt, e2, r_words, nullptr, c_out, items, premul);
  if (c_in == c_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_step4i: a shuffled store cannot work in place");
  // the store of the blinding launch finds each item's output plane in the permutation itself (OP_STOREW, sc_vm.h): rows that
  // are not permutations act as the identity, so every output row is written; no destination array, no launch to build one
  // (round 3's 26-us k_perm_to_dest waited up to 18 ms for a wave slot beside the other shard's chip-filling launches)
  return modexp_var_impl(ctx, k.mod_n, c_in, rhos, rho_words, ubits, fbt, e2, r_words, nullptr, c_out, items, premul, permutation, (uint32_t)planes);
}

int sc_initiator_step4(sc_ctx* ctx, int dgk_key_id, int l, const uint32_t* d_enc, const uint32_t* beta_enc, const uint64_t* alpha,
                       const uint64_t* alpha_tilde, const uint64_t* rsmall, const uint64_t* delta_a, const uint32_t* rhos, int rho_words,
                       const int64_t* permutation, const uint32_t* r_rand, int r_words, int flags, uint32_t* c_unblinded_out, uint32_t* c_out,
                       uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const DgkKey* kp = dgk_key(ctx, dgk_key_id);
  if (!kp || l <= 0 || l > SC_MAX_L || !d_enc || !beta_enc || !alpha || !alpha_tilde || !rsmall || !delta_a || !c_out ||
      (rhos && rho_words <= 0) || (r_rand && (r_words <= 0 || !rhos)))
    return fail(ctx, SC_ERR_ARG, "sc_initiator_step4: bad argument");
  const DgkKey k = *kp;
  const uint64_t planes = (uint64_t)l + 1, items = planes * count;
  const size_t row = (size_t)k.nw;
  // one inversion pass over [d], [beta_0] .. [beta_{l-1}]: in place when they are the planes of one array, else joined first
  const uint32_t* joined = d_enc;
  uint32_t* inv;
  int rc = tmp_words(ctx, TMP_S_E, items * row, &inv); if (rc) return rc;
  if (beta_enc != d_enc + count * row) {
    uint32_t* j;
    rc = tmp_words(ctx, TMP_S_F, items * row, &j); if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(j, d_enc, count * row * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(j + count * row, beta_enc, (size_t)l * count * row * 4, hipMemcpyDeviceToDevice, ctx->stream));
    joined = j;
  }
  int64_t bad = -1;
  rc = sc_modinv(ctx, k.mod_n, joined, inv, items, &bad);
  if (rc) return rc;
  uint32_t* c_h = c_unblinded_out;
  if (!rhos) c_h = c_out;                                    // steps 4c-4h only
  else if (!c_h) { rc = tmp_words(ctx, TMP_S_G, items * row, &c_h); if (rc) return rc; }
  rc = sc_dgk_step4(ctx, k.mod_n, k.cst_g, k.cst_ginv, l, beta_enc, inv + count * row, d_enc, inv, alpha, alpha_tilde, rsmall, delta_a, c_h, count);
  if (rc || !rhos) return rc;
  return sc_initiator_step4i(ctx, dgk_key_id, l, c_h, rhos, rho_words, permutation, r_rand, r_words, flags, c_out, count);
}

int sc_keyholder_step2_4b(sc_ctx* ctx, int paillier_key_id, int dgk_key_id, int l, const uint32_t* z_enc, const uint32_t* r_rand, int r_words,
                          int flags, uint32_t* z_out, uint64_t* beta, uint64_t* dbit, uint32_t* zeta1, uint32_t* zeta2, uint32_t* d_beta_out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* pk = paillier_key(ctx, paillier_key_id);
  const DgkKey* dk = dgk_key(ctx, dgk_key_id);
  if (!pk || !dk || !pk->secret || l <= 0 || l > SC_MAX_L || !z_enc || !z_out || !beta || !dbit || !zeta1 || !zeta2 || !d_beta_out || (r_rand && r_words <= 0))
    return fail(ctx, SC_ERR_ARG, "sc_keyholder_step2_4b: bad argument");
  if (big_bits(dk->u) <= l + 2) return fail(ctx, SC_ERR_ARG, "sc_keyholder_step2_4b: u must exceed 2^(l+2) (SC/keyholder.py:212)");
  const PaillierKey p = *pk; const DgkKey d = *dk;
  int rc = sc_paillier_decrypt(ctx, paillier_key_id, z_enc, z_out, count); if (rc) return rc;
  const uint64_t items = ((uint64_t)l + 1) * count;
  uint8_t* bits;
  rc = tmp_words(ctx, TMP_S_I, items, &bits); if (rc) return rc;
  rc = plain_bob_impl(ctx, z_out, p.n.data(), p.nw, l, count, beta, dbit, zeta1, zeta2, bits); if (rc) return rc;   // + the bits of steps 4a / 4b
  if (r_rand && (flags & SC_STEP_RANDOMIZERS_READY))        // r_rand holds h^r itself: g^bit * h^r is one selected-constant product
    return sc_modmul_const_sel(ctx, d.mod_n, r_rand, -1, d.cst_g, bits, d_beta_out, items);
  if (r_rand) return dgk_randomize_impl(ctx, d, nullptr, bits, r_rand, r_words, d_beta_out, items);
  // unrandomized: g^bit -- the residue 1 times (1 or g), chosen per item inside the launch
  const Prog* pr;
  rc = cached_prog(ctx, "bits1:" + std::to_string(d.mod_n) + ":" + std::to_string(d.cst_g), d.mod_n, [&](Builder& bd) {
    const int cg = bd.use_const(d.cst_g);
    bd.loadt_const(1);
    bd.mul_constsel(1, 1, cg);
    bd.redc(); bd.storew(0);
  }, &pr); if (rc) return rc;
  VmExt ex[2] = {mk_ext(d_beta_out, d.nw, d.nw), mk_ext(bits, 0, 0)};
  return run_vm(ctx, d.mod_n, *pr, ex, 2, items);
}

int sc_keyholder_step4j_5(sc_ctx* ctx, int paillier_key_id, int dgk_key_id, int l, const uint32_t* c_enc, const uint32_t* zeta1,
                          const uint32_t* zeta2, const uint32_t* rho3, int flags, uint64_t* delta_b_out, uint32_t* out3, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* pk = paillier_key(ctx, paillier_key_id);
  const DgkKey* dk = dgk_key(ctx, dgk_key_id);
  if (!pk || !dk || !pk->secret || !dk->secret || l <= 0 || l > SC_MAX_L || !c_enc || !zeta1 || !zeta2 || !delta_b_out || !out3)
    return fail(ctx, SC_ERR_ARG, "sc_keyholder_step4j_5: bad argument");
  const PaillierKey p = *pk;
  const DgkKey d = *dk;
  // step 4j: the l + 1 zero tests of a comparison OR their verdicts into a context-owned accumulator that is zero at rest -- the
  // launch that encrypts delta_B below reads it, hands it to delta_b_out and resets it (OP_TAKEFLAG): no clearing launch, which as a
  // runtime fill kernel waited up to 14 ms for a wave slot beside another context's chip-filling launch
  uint64_t* acc;
  int rc = zero_kept_flags(ctx, count, &acc); if (rc) return rc;
  struct Dirty {      // an error between the accumulation and the launch that resets the accumulator must not leave verdicts behind
    sc_ctx* c; bool armed = true;
    ~Dirty() { if (armed) drop_zero_kept_flags(c); }
  } dirty{ctx};
  rc = modexp_shared_impl(ctx, d.mod_p, d.exp_vp, c_enc, d.nw, nullptr, nullptr, nullptr, ((uint64_t)l + 1) * count, acc, count, true); if (rc) return rc;
  // step 5: three encryptions into the row blocks of one array (no copies of zeta_1 / zeta_2 into a joined plaintext array)
  uint32_t* enc = out3;
  if (rho3) { rc = tmp_words(ctx, TMP_S_F, 3 * count * 2 * p.nw, &enc); if (rc) return rc; }
  const size_t blk = (size_t)count * 2 * p.nw;
  rc = sc_paillier_encrypt_raw(ctx, p.mod_n2, p.cst_n, zeta1, p.nw, enc, count); if (rc) return rc;
  rc = sc_paillier_encrypt_raw(ctx, p.mod_n2, p.cst_n, zeta2, p.nw, enc + blk, count); if (rc) return rc;
  {
    const Prog* pr;
    rc = cached_prog(ctx, "encflag:" + std::to_string(p.mod_n2) + ":" + std::to_string(p.cst_n), p.mod_n2, [&](Builder& bd) {
      const int c = bd.use_const(p.cst_n);
      bd.takeflag(0, 1); bd.mul_const(c);                     // delta_B N
      bd.add1(); bd.storew(2);
    }, &pr); if (rc) return rc;
    const int w2 = 2 * p.nw;
    VmExt ex[3] = {mk_ext(acc, 2, 2), mk_ext(delta_b_out, 2, 2), mk_ext(enc + 2 * blk, w2, w2)};
    rc = run_vm(ctx, p.mod_n2, *pr, ex, 3, count); if (rc) return rc;
    dirty.armed = false;
  }
  if (!rho3) return SC_OK;                                                                                             // unrandomized
  if (flags & SC_STEP_RANDOMIZERS_READY) return sc_modmul(ctx, p.mod_n2, enc, 2 * p.nw, rho3, 2 * p.nw, out3, 3 * count);   // rho^N computed ahead
  return sc_paillier_randomize(ctx, paillier_key_id, enc, rho3, out3, 3 * count);                                    // the 3 .randomize() (:126-128)
}

int sc_initiator_step67(sc_ctx* ctx, int paillier_key_id, const uint64_t* delta_a, const uint32_t* delta_b_enc, const uint32_t* zeta1_enc,
                        const uint32_t* zeta2_enc, const uint64_t* rsmall, const uint32_t* rshift, int flags, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !delta_a || !delta_b_enc || !zeta1_enc || !zeta2_enc || !rsmall || !rshift || !out)
    return fail(ctx, SC_ERR_ARG, "sc_initiator_step67: bad argument");
  const PaillierKey k = *kp;
  const int w2 = 2 * k.nw;
  // [[x<=y]] = [[zeta]] * D * [[-(r div 2^l) - (1 - delta_A)]],  D = [[delta_B]]^-1 (delta_A = 1) or [[delta_B]] (delta_A = 0):
  // steps 6 and 7 (SC/initiator.py:529-531, 558-563) with ONE inversion pass -- [[a]] [[b]] = [[a + b]] holds exactly for
  // unrandomized g = N + 1 encryptions, so the residues equal the literal formula's
  uint32_t* inv;
  int rc = tmp_words(ctx, TMP_S_E, count * w2, &inv); if (rc) return rc;
  int64_t bad = -1;
  rc = sc_modinv(ctx, k.mod_n2, delta_b_enc, inv, count, &bad);
  if (rc) return rc;
  // one launch for the rest: the selections "zeta_1 if r < (N-1)/2 else zeta_2" and "D" are per-item operand choices of the loads,
  // and [[-(r div 2^l)]] [[-1]]^(1 - delta_A) = 1 - (r div 2^l + 1 - delta_A) N  (mod N^2) is one encryption
  const Prog* p;
  rc = cached_prog(ctx, "step67:" + std::to_string(k.mod_n2) + ":" + std::to_string(k.cst_n), k.mod_n2, [&](Builder& bd) {
    const int cn = bd.use_const(k.cst_n);
    bd.loadw(6, 0, 0, k.nw); bd.add_flag(5, 0, true);                      // r div 2^l + (1 - delta_A)
    bd.mul_const(cn); bd.neg(); bd.add1();                                 // 1 - (...) N
    bd.mul_const(0); bd.stt(0);
    bd.loadw_sel(0, 1, 4, 0); bd.mul_const(0); bd.stt(1);                  // [[zeta]]  (SC/initiator.py:558-560)
    bd.loadw_sel(2, 3, 5, 0); bd.mul_const(0);                             // D: [[delta_B]]^-1 where delta_A = 1 (:529-531)
    bd.mul_tbl(1); bd.mul_tbl(0);
    bd.redc(); bd.storew(7);
  }, &p); if (rc) return rc;
  VmExt ex[8] = {mk_ext(zeta1_enc, w2, w2), mk_ext(zeta2_enc, w2, w2), mk_ext(inv, w2, w2), mk_ext(delta_b_enc, w2, w2),
                 mk_ext(rsmall, 2, 2), mk_ext(delta_a, 2, 2), mk_ext(rshift, k.nw, k.nw), mk_ext(out, w2, w2)};
  return run_vm(ctx, k.mod_n2, *p, ex, 8, count);
}

// ---- secure selection and compare-exchange -----------------------------------------------------------------
// What selection.py / sorting.py used to compose from the primitives, one call per protocol step: the field layout, the Horner chain
// of shared-exponent squarings, T_j with per-row exponents (pair kernel, or exponentiations modulo N^2 where the modulus has no
// per-row pair instance), and the two finishes.  Temporaries TMP_SEL_*; the callees' own (TMP_S_A .. TMP_S_D, TMP_PAIR) are not held
// across their calls.  The selection, the multiplication (§8e), the inner product (§8g) and the one-hot encoding (§8i) share one blinded
// round trip: pack_messages packs a family's field list (sc_pack_plan.h), keyholder_round is the key holder's step, finish_ratio divides
// the blinding out (the one-hot has nothing to divide out: its finish is a rotation of rows).
enum SelectTmp { TMP_SEL_A = 49, TMP_SEL_B, TMP_SEL_C, TMP_SEL_D, TMP_SEL_E, TMP_SEL_F };

// one pinned, device-visible word per context for keyholder_round's verdict (freed with the context's other allocations)
static int select_verdict_word(sc_ctx* ctx, uint32_t** out) {
  auto* ks = keys_of(ctx);
  if (!ks->select_verdict) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc((void**)&ks->select_verdict, sizeof(uint32_t), hipHostMallocMapped));
  }
  *out = ks->select_verdict;
  return SC_OK;
}
static int sel_t_bits(const SelLayout& lay) { int b = 0; for (int j = 0; j < lay.nf; j++) b = std::max(b, lay.fbits[j]); return b; }

// 1 + v N for v < N (words of N): a residue modulo N^2
static Big one_plus_vn(const Big& v, const Big& n) {
  Big r = big_fit(big_mul(big_fit(v, n.size()), n), 2 * n.size());
  for (size_t i = 0; i < r.size() && ++r[i] == 0; i++) {}
  return r;
}
static Big pow2_words(int bit, size_t words) { Big r(words, 0); r[bit >> 5] = 1u << (bit & 31); return r; }

// x^(2^bits) * mul_into mod N^2 (selection._pow2_shared): the exponent is registered once per context
static int sel_pow2(sc_ctx* ctx, const PaillierKey& k, int bits, const uint32_t* x, const uint32_t* mul_into, uint32_t* out, uint64_t count) {
  auto& cache = keys_of(ctx)->pow2_exps;
  auto it = cache.find(bits);
  if (it == cache.end()) {
    int id;
    int rc = reg_exp(ctx, pow2_words(bits, (size_t)bits / 32 + 1), &id); if (rc) return rc;
    it = cache.emplace(bits, id).first;
  }
  if (k.pairs && sc_mod_supports_sq(ctx, k.mod_n) == 1) return sc_modexp_shared_sq(ctx, k.mod_n, k.mod_n2, it->second, x, 2 * k.nw, mul_into, out, count);
  return sc_modexp_shared(ctx, k.mod_n2, it->second, x, 2 * k.nw, mul_into, out, count);
}

// out = acc * prod_j base_j^(e_j) over `planes` consecutive planes base [planes][items][2 nw], e [planes][items][ew] where the modulus has
// no pair kernel with per-row exponents: one exponentiation modulo N^2 (into tmp) and one product (into acc, the last into out) per plane
static int pow_product_plain(sc_ctx* ctx, const PaillierKey& k, int planes, int ebits, const uint32_t* base, const uint32_t* e, int ew, uint32_t* tmp,
                             uint32_t* acc, uint32_t* out, uint64_t items) {
  const int w2 = 2 * k.nw;
  for (int j = 0; j < planes; j++) {
    int rc = sc_modexp_var(ctx, k.mod_n2, base + (size_t)j * items * w2, e + (size_t)j * items * ew, ew, ebits, -1, nullptr, 0, tmp, items); if (rc) return rc;
    rc = sc_modmul(ctx, k.mod_n2, acc, w2, tmp, w2, j == planes - 1 ? out : acc, items); if (rc) return rc;
  }
  return SC_OK;
}

// T_j = [[sigma]]^(e_j) [[d_j]]^(r_a) (1 + rab_j N) for the flat items j count + i (selection.select_t): t_out [nf count][2 nw].
// The multiplication's T_j (8e) is the same product with sigma = x, d_j = y_j, e_j = e_x_j and r_a = e_y, exponents of `ebits` bits.
static int two_base_t(sc_ctx* ctx, const PaillierKey& k, int nf, int ebits, const uint32_t* sigma, const uint32_t* d, const uint32_t* r_a, int aw,
                      const uint32_t* e, int ew, const uint32_t* rab, uint32_t* t_out, uint64_t count) {
  const int w2 = 2 * k.nw;
  const uint64_t items = (uint64_t)nf * count;
  uint32_t *x, *ex, *mi;
  int rc = tmp_words(ctx, TMP_SEL_A, 2 * items * w2, &x); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_B, 2 * items * ew, &ex); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_C, items * w2, &mi); if (rc) return rc;
  // bases [2][nf count]: sigma for every column, then d; exponents likewise: e, then r_a (zero-extended to ew words) for every column.
  // These are the copies the Python composition made (torch.stack / expand): sc_modexp_var_sq reads its bases as rows of one array
  // and an item cannot address "its row modulo count".  A variant of the pair program with one operand per base and a broadcast
  // period would save about 2 nf count 2nw words of traffic per call; against the exponentiations that is noise, so it is left out.
  for (int j = 0; j < nf; j++)
    HIPCHK(ctx, hipMemcpyAsync(x + (size_t)j * count * w2, sigma, (size_t)count * w2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(x + items * w2, d, items * w2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ex, e, items * ew * 4, hipMemcpyDeviceToDevice, ctx->stream));
  uint32_t* ex_a = ex + items * ew;
  const int cw = std::min(aw, ew);            // r_a < 2^kappa < 2^(32 ew): words past ew are zero
  if (cw != ew) HIPCHK(ctx, hipMemsetAsync(ex_a, 0, items * ew * 4, ctx->stream));
  for (int j = 0; j < nf; j++)
    HIPCHK(ctx, hipMemcpy2DAsync(ex_a + (size_t)j * count * ew, (size_t)ew * 4, r_a, (size_t)aw * 4, (size_t)cw * 4, count, hipMemcpyDeviceToDevice, ctx->stream));
  rc = sc_paillier_encrypt_raw(ctx, k.mod_n2, k.cst_n, rab, k.nw, mi, items); if (rc) return rc;
  rc = k.pairs ? sc_modexp_var_sq(ctx, k.mod_n, k.mod_n2, 2, x, w2, ex, ew, ebits, mi, t_out, items) : SC_ERR_UNSUPPORTED;
  if (rc != SC_ERR_UNSUPPORTED) return rc;
  // no pair kernel with per-row exponents for this modulus: the same residues from exponentiations modulo N^2 (ex_a follows ex)
  return pow_product_plain(ctx, k, 2, ebits, x, ex, ew, t_out, mi, t_out, items);
}
static int sel_t(sc_ctx* ctx, const PaillierKey& k, const SelLayout& lay, const uint32_t* sigma, const uint32_t* d, const uint32_t* r_a, int aw,
                 const uint32_t* e, int ew, const uint32_t* rab, uint32_t* t_out, uint64_t count) {
  return two_base_t(ctx, k, lay.nf, sel_t_bits(lay), sigma, d, r_a, aw, e, ew, rab, t_out, count);
}

static int sel_finish_args(sc_ctx* ctx, const char* who, const PaillierKey* kp, const SelLayout& lay, int aw, int ew, bool ptrs_ok) {
  if (!kp || !ptrs_ok || aw < 1 || aw > 2 || ew < 1) return fail(ctx, SC_ERR_ARG, "%s: bad argument", who);
  return exp_rows(ctx, who, ew, sel_t_bits(lay));
}

// ---- the blinded round trip the selection, the multiplication and the inner product share ----------------------------
// dst = [[x + R]] rho^N over `items` rows (x, dst [items][2 nw], R [items][nw]): the packing program of all four families
static int blind_and_randomize(sc_ctx* ctx, const PaillierKey& k, int key_id, const uint32_t* x, const uint32_t* R, const uint32_t* rho, uint32_t* dst,
                               uint64_t items) {
  const int w2 = 2 * k.nw;
  const Prog* p;
  int rc = cached_prog(ctx, "selpk:" + std::to_string(k.mod_n2) + ":" + std::to_string(k.cst_n), k.mod_n2, [&](Builder& bd) {
    const int cn = bd.use_const(k.cst_n);
    bd.loadw(1, 0, 0, k.nw); bd.mul_const(cn); bd.add1();                 // [[R]] = 1 + R N
    bd.mul_const(0); bd.mul_extw(0);                                      // [[x + R]]
    bd.storew(2);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(x, w2, w2), mk_ext(R, k.nw, k.nw), mk_ext(dst, w2, w2)};
  rc = run_vm(ctx, k.mod_n2, *p, ex, 3, items); if (rc) return rc;
  return sc_paillier_randomize(ctx, key_id, dst, rho, dst, items);        // * rho^N
}

// out = msg prod_(f >= 1) field_f^(2^off_f), off_f the bits of fld[0 .. f - 1] (sc_pack_plan.h; msg stands in for field 0): the exponents
// are shared by the batch, so Horner from the top field with squarings only.  A field holds a prefix of the rows of the one below it, whose
// further rows join as copies of themselves.  The step that joins field f - 1 writes half[(f - 1) & 1], the last one `out`.
static int horner_pow2(sc_ctx* ctx, const PaillierKey& k, const PackField* fld, int F, const uint32_t* msg, uint32_t* const half[2], uint32_t* out) {
  const size_t w2 = 2 * (size_t)k.nw;
  const uint32_t* cur = fld[F - 1].rows;
  for (int f = F - 1; f >= 1; f--) {
    uint32_t* dst = f == 1 ? out : half[(f - 1) & 1];
    const uint32_t* low = f == 1 ? msg : fld[f - 1].rows;
    const uint64_t ncur = fld[f].held, nlow = fld[f - 1].held;
    int rc = sel_pow2(ctx, k, fld[f - 1].bits, cur, low, dst, ncur); if (rc) return rc;
    if (nlow > ncur) HIPCHK(ctx, hipMemcpyAsync(dst + ncur * w2, low + ncur * w2, (nlow - ncur) * w2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    cur = dst;
  }
  return SC_OK;
}

// The pack step of all four families once the entry has checked its arguments, launched its prep kernel (R [items][nw], TMP_SEL_A) and
// listed its fields: field 0, held by all `items` messages, becomes m = [[x + R]] rho_p^N (TMP_SEL_B) -- P itself where it is the only
// field -- and the fields above it join by horner_pow2 over the two halves of TMP_SEL_C.
static int pack_messages(sc_ctx* ctx, const PaillierKey& k, int key_id, const std::vector<PackField>& fld, const uint32_t* R, const uint32_t* rho_p,
                         uint32_t* p_out, uint64_t items) {
  const size_t words = items * 2 * k.nw;
  uint32_t *m, *acc;
  int rc = tmp_words(ctx, TMP_SEL_B, words, &m); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_C, 2 * words, &acc); if (rc) return rc;
  rc = blind_and_randomize(ctx, k, key_id, fld[0].rows, R, rho_p, fld.size() == 1 ? p_out : m, items); if (rc) return rc;
  uint32_t* const half[2] = {acc, acc + words};
  return horner_pow2(ctx, k, fld.data(), (int)fld.size(), m, half, p_out);
}

// The key holder's step: decrypt the n_messages rows of P, let the family's split kernel (`split`, given the plaintexts, the n_products
// products and the verdict word) multiply the fields, encrypt and randomize the products, then read the kernel's verdict.
static int keyholder_round(sc_ctx* ctx, const char* who, const PaillierKey& k, int key_id, const uint32_t* p_enc, const uint32_t* rho, uint32_t* out,
                           uint64_t n_messages, uint64_t n_products, const std::function<int(const uint32_t*, uint32_t*, uint32_t*)>& split,
                           const char* layout_message) {
  uint32_t *pl, *prod, *c;
  int rc = tmp_words(ctx, TMP_SEL_A, n_messages * k.nw, &pl); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_B, n_products * k.nw, &prod); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_C, n_products * 2 * k.nw, &c); if (rc) return rc;
  // the verdict word lives in pinned host memory the kernel writes itself (like the inversion's verdicts: no copy back) -- a word
  // of its own, so nothing a callee does with the inversion's status words (status_words may free and regrow them) can touch it
  uint32_t* bad;
  rc = select_verdict_word(ctx, &bad); if (rc) return rc;
  *(volatile uint32_t*)bad = 0;             // (an earlier call has waited for its kernels before it returned)
  rc = sc_paillier_decrypt(ctx, key_id, p_enc, pl, n_messages); if (rc) return rc;
  if (split(pl, prod, bad)) return fail(ctx, SC_ERR_HIP, "%s: launch failed", who);
  rc = sc_paillier_encrypt_raw(ctx, k.mod_n2, k.cst_n, prod, k.nw, c, n_products); if (rc) return rc;
  rc = sc_paillier_randomize(ctx, key_id, c, rho, out, n_products); if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (*(volatile uint32_t*)bad) return fail(ctx, SC_ERR_LAYOUT, "%s", layout_message);
  return SC_OK;
}

// out = ([[AB]] T^-1)^coef * base for coef in {+1, -1, -2} (checked by the entry, before anything is launched) and an optional base:
// coef = +1 inverts T, a negative coef inverts num_if_plus = [[AB]] instead -- one inversion pass over `items` rows either way (into
// inv_tmp), so SC_ERR_NOT_INVERTIBLE names the row; then one launch: the lift num R^m for the m Montgomery products that follow,
// (num inv)^|coef|, then the base
static int finish_ratio(sc_ctx* ctx, const PaillierKey& k, int coef, const uint32_t* num_if_plus, const uint32_t* T, const uint32_t* base, uint32_t* out,
                        uint64_t items, uint32_t* inv_tmp) {
  const int w2 = 2 * k.nw;
  const uint32_t* num = coef == 1 ? num_if_plus : T;
  int rc = sc_modinv(ctx, k.mod_n2, coef == 1 ? T : num_if_plus, inv_tmp, items, nullptr); if (rc) return rc;
  const int pairs = coef == -2 ? 2 : 1, nmul = 2 * pairs - 1 + (base ? 1 : 0);
  const Mod& m2 = ctx->mods[k.mod_n2];
  int cid;
  { Big one(m2.nwords, 0); one[0] = 1; rc = sc_const_create_cached(ctx, k.mod_n2, big_shl_mod(one, m2.n, nmul * m2.W * m2.S), &cid); if (rc) return rc; }   // R^nmul mod N^2
  const Prog* p;
  rc = cached_prog(ctx, "ratiofin:" + std::to_string(k.mod_n2) + ":" + std::to_string(pairs) + (base ? ":b" : ""), k.mod_n2, [&](Builder& bd) {
    bd.loadw(0); bd.mul_const(bd.use_const(cid));                         // num R^nmul
    bd.mul_extw(1);                                                       // num inv
    if (pairs == 2) { bd.mul_extw(0); bd.mul_extw(1); }                   // (num inv)^2
    if (base) bd.mul_extw(2);
    bd.storew(3);
  }, &p); if (rc) return rc;
  VmExt ex[4] = {mk_ext(num, w2, w2), mk_ext(inv_tmp, w2, w2), mk_ext(base, w2, w2), mk_ext(out, w2, w2)};
  return run_vm(ctx, k.mod_n2, *p, ex, 4, items);
}

int sc_initiator_select_d(sc_ctx* ctx, int paillier_key_id, const uint32_t* z_enc, const uint32_t* r, uint32_t* d_out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !z_enc || !r || !d_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_select_d: bad argument");
  const PaillierKey k = *kp;
  const int w2 = 2 * k.nw;
  const Prog* p;
  int rc = cached_prog(ctx, "seld:" + std::to_string(k.mod_n2) + ":" + std::to_string(k.cst_n), k.mod_n2, [&](Builder& bd) {
    const int cn = bd.use_const(k.cst_n);
    bd.loadw(1, 0, 0, k.nw); bd.mul_const(cn); bd.neg(); bd.add1();       // [[-r]] = 1 - r N
    bd.mul_const(0); bd.mul_extw(0);                                      // times [[z]] = [[y - x + 2^l + r]]
    bd.storew(2);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(z_enc, w2, w2), mk_ext(r, k.nw, k.nw), mk_ext(d_out, w2, w2)};
  return run_vm(ctx, k.mod_n2, *p, ex, 3, count);
}

int sc_paillier_one_minus(sc_ctx* ctx, int paillier_key_id, const uint32_t* c, uint32_t* out, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !c || !out) return fail(ctx, SC_ERR_ARG, "sc_paillier_one_minus: bad argument");
  const PaillierKey k = *kp;
  int cst_g;
  int rc = reg_const(ctx, k.mod_n2, one_plus_vn(Big(1, 1), k.n), &cst_g); if (rc) return rc;      // g = N + 1
  rc = sc_modinv(ctx, k.mod_n2, c, out, count, nullptr); if (rc) return rc;
  return sc_modmul_const(ctx, k.mod_n2, out, cst_g, out, count);
}

int sc_initiator_cx_differences(sc_ctx* ctx, int paillier_key_id, int kappa, int nfields, const int* widths_hptr, const uint32_t* f_enc,
                                const uint32_t* g_enc, const uint32_t* d_key, uint32_t* d_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_cx_differences: bad key");
  const PaillierKey k = *kp;
  SelLayout lay;
  int rc = select_layout(ctx, "sc_initiator_cx_differences", big_bits(k.n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (!f_enc || !g_enc || !d_key || !d_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_cx_differences: bad argument");
  const int w2 = 2 * k.nw, np = nfields - 1;
  const size_t col = (size_t)count * w2;
  HIPCHK(ctx, hipMemcpyAsync(d_out, d_key, col * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (np == 0) return SC_OK;
  const uint64_t items = (uint64_t)np * count;
  uint32_t* finv;
  rc = tmp_words(ctx, TMP_SEL_A, items * w2, &finv); if (rc) return rc;
  rc = sc_modinv(ctx, k.mod_n2, f_enc + col, finv, items, nullptr); if (rc) return rc;
  // One launch over the np * count flat items of the columns j >= 1: G_j F_j^-1 c_j with c_j = 1 + 2^w_j N.  The interpreter takes
  // nothing from an item's number but the `limit` of an operand (items at or past it read the residue 1), so the item's column picks
  // its constant through limits: broadcast operand t holds c_(t+1) / c_(t+2) for the items below (t + 1) count, and every item takes
  // the last column's constant -- a column's factors telescope to its own c_j.  One product per column after an item's own.
  const Mod& m2 = ctx->mods[k.mod_n2];
  const Big& n2 = m2.n;
  int cid_last, cid_ratio[SEL_MAX_FIELDS] = {-1, -1, -1, -1};
  rc = sc_const_create_cached(ctx, k.mod_n2, big_shl_mod(one_plus_vn(pow2_words(lay.width[np], k.n.size()), k.n), n2, m2.W * m2.S), &cid_last);   // c_np R
  if (rc) return rc;
  for (int t = 0; t + 1 < np; t++) {          // c_(t+1) / c_(t+2) = 1 + (2^w_(t+1) - 2^w_(t+2)) N  (mod N^2)
    Big a = pow2_words(lay.width[t + 1], k.n.size()), b = pow2_words(lay.width[t + 2], k.n.size());
    if (big_cmp(a, b) >= 0) big_sub(a, b); else { big_sub(b, a); a = k.n; big_sub(a, b); }
    rc = sc_const_create_cached(ctx, k.mod_n2, one_plus_vn(a, k.n), &cid_ratio[t]); if (rc) return rc;
  }
  const Prog* p;
  rc = cached_prog(ctx, "cxdiff:" + std::to_string(k.mod_n2) + ":" + std::to_string(np) + ":" + std::to_string(cid_last), k.mod_n2, [&](Builder& bd) {
    bd.loadw(0);
    for (int t = 0; t + 1 < np; t++) bd.mul_extl(3 + t);                  // times c_(t+1) / c_(t+2) below (t + 1) count, else times 1
    bd.mul_const(bd.use_const(cid_last));                                 // G c_j R
    bd.mul_extw(1);                                                       // G c_j F^-1
    bd.storew(2);
  }, &p); if (rc) return rc;
  VmExt ex[5] = {mk_ext(g_enc + col, w2, w2), mk_ext(finv, w2, w2), mk_ext(d_out + col, w2, w2), mk_ext(nullptr, 0, 0), mk_ext(nullptr, 0, 0)};
  for (int t = 0; t + 1 < np; t++) ex[3 + t] = mk_ext(ctx->consts[cid_ratio[t]].d_limbs, 0, (uint32_t)m2.S, (uint64_t)(t + 1) * count);
  return run_vm(ctx, k.mod_n2, *p, ex, 5, items);
}

int sc_initiator_select_pack(sc_ctx* ctx, int paillier_key_id, int kappa, int nfields, const int* widths_hptr, const uint32_t* sigma_enc,
                             const uint32_t* d_enc, const uint32_t* r_a, int aw, const uint32_t* r_b, int bw, const uint32_t* rho_p, int ew,
                             uint32_t* p_out, uint32_t* e_out, uint32_t* rab_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_select_pack: bad key");
  const PaillierKey k = *kp;
  SelLayout lay;
  int rc = select_layout(ctx, "sc_initiator_select_pack", big_bits(k.n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  if (!rho_p) return fail(ctx, SC_ERR_ARG, "sc_initiator_select_pack: rho_p is required: P must carry a fresh rho^N");
  if (!sigma_enc || !d_enc || !r_a || !r_b || !p_out || !e_out || !rab_out || aw < 1 || aw > 2 || bw < 1 || bw > k.nw || ew < 1)
    return fail(ctx, SC_ERR_ARG, "sc_initiator_select_pack: bad argument");
  rc = exp_rows(ctx, "sc_initiator_select_pack", ew, sel_t_bits(lay)); if (rc) return rc;
  if (count == 0) return SC_OK;
  uint32_t* R;
  rc = tmp_words(ctx, TMP_SEL_A, count * k.nw, &R); if (rc) return rc;
  if (launch_select_prep(ctx->stream, r_a, aw, r_b, bw, lay, k.nw, ew, count, R, e_out, rab_out)) return fail(ctx, SC_ERR_HIP, "sc_initiator_select_pack: launch failed");
  return pack_messages(ctx, k, paillier_key_id, column_fields(sigma_enc, d_enc, nfields, lay.s, lay.fbits, count, (size_t)count * 2 * k.nw), R, rho_p, p_out, count);
}

int sc_keyholder_select_mult(sc_ctx* ctx, int paillier_key_id, int kappa, int nfields, const int* widths_hptr, const uint32_t* p_enc,
                             const uint32_t* rho_products, uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !kp->secret) return fail(ctx, SC_ERR_ARG, "sc_keyholder_select_mult: needs the secret key");
  const PaillierKey k = *kp;
  SelLayout lay;
  int rc = select_layout(ctx, "sc_keyholder_select_mult", big_bits(k.n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (!p_enc || !rho_products || !out) return fail(ctx, SC_ERR_ARG, "sc_keyholder_select_mult: bad argument");
  return keyholder_round(ctx, "sc_keyholder_select_mult", k, paillier_key_id, p_enc, rho_products, out, count, (uint64_t)nfields * count,
                         [&](const uint32_t* pl, uint32_t* prod, uint32_t* bad) { return launch_select_split(ctx->stream, pl, k.nw, lay, count, prod, bad); },
                         "select: a decrypted P exceeds the announced field layout (kappa or widths differ between the players)");
}

int sc_initiator_select_finish(sc_ctx* ctx, int paillier_key_id, int kappa, int nfields, const int* widths_hptr, const uint32_t* sigma_enc,
                               const uint32_t* d_enc, const uint32_t* b_enc, const uint32_t* products, const uint32_t* r_a, int aw,
                               const uint32_t* e, int ew, const uint32_t* rab, uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_select_finish: bad key");
  const PaillierKey k = *kp;
  SelLayout lay;
  int rc = select_layout(ctx, "sc_initiator_select_finish", big_bits(k.n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  rc = sel_finish_args(ctx, "sc_initiator_select_finish", kp, lay, aw, ew, sigma_enc && d_enc && b_enc && products && r_a && e && rab && out); if (rc) return rc;
  if (count == 0) return SC_OK;
  const int w2 = 2 * k.nw;
  const uint64_t items = (uint64_t)nfields * count;
  uint32_t *T, *t_inv;
  rc = tmp_words(ctx, TMP_SEL_D, items * w2, &T); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_E, items * w2, &t_inv); if (rc) return rc;
  rc = sel_t(ctx, k, lay, sigma_enc, d_enc, r_a, aw, e, ew, rab, T, count); if (rc) return rc;
  rc = sc_modinv(ctx, k.mod_n2, T, t_inv, items, nullptr); if (rc) return rc;
  // one launch: b ab T^-1 -- the lift b R^2, then the two Montgomery products
  const Mod& m2 = ctx->mods[k.mod_n2];
  int cid;
  { Big one(m2.nwords, 0); one[0] = 1; rc = sc_const_create_cached(ctx, k.mod_n2, big_shl_mod(one, m2.n, 2 * m2.W * m2.S), &cid); if (rc) return rc; }   // R^2 mod N^2
  const Prog* p;
  rc = cached_prog(ctx, "selfin:" + std::to_string(k.mod_n2), k.mod_n2, [&](Builder& bd) {
    bd.loadw(0); bd.mul_const(bd.use_const(cid));                         // b R^2
    bd.mul_extw(1); bd.mul_extw(2);                                       // b ab T^-1
    bd.storew(3);
  }, &p); if (rc) return rc;
  VmExt ex[4] = {mk_ext(b_enc, w2, w2), mk_ext(products, w2, w2), mk_ext(t_inv, w2, w2), mk_ext(out, w2, w2)};
  return run_vm(ctx, k.mod_n2, *p, ex, 4, items);
}

int sc_initiator_cx_finish(sc_ctx* ctx, int paillier_key_id, int kappa, int nfields, const int* widths_hptr, const uint32_t* delta_enc,
                           const uint32_t* d_enc, const uint32_t* f_enc, const uint32_t* g_enc, const uint32_t* products, const uint32_t* r_a,
                           int aw, const uint32_t* e, int ew, const uint32_t* rab, const uint64_t* lo_index, const uint64_t* hi_index,
                           uint32_t* out, uint64_t out_rows, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_cx_finish: bad key");
  const PaillierKey k = *kp;
  SelLayout lay;
  int rc = select_layout(ctx, "sc_initiator_cx_finish", big_bits(k.n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  rc = sel_finish_args(ctx, "sc_initiator_cx_finish", kp, lay, aw, ew,
                       delta_enc && d_enc && f_enc && g_enc && products && r_a && e && rab && out && (!lo_index) == (!hi_index)); if (rc) return rc;
  const uint64_t items = (uint64_t)nfields * count;
  if (!lo_index && out_rows < 2 * items)
    return fail(ctx, SC_ERR_ARG, "sc_initiator_cx_finish: out holds %llu rows, the contiguous [2][nf][count] form needs %llu",
                (unsigned long long)out_rows, (unsigned long long)(2 * items));
  if (count == 0) return SC_OK;
  const int w2 = 2 * k.nw;
  uint32_t *T, *U, *u_inv;
  rc = tmp_words(ctx, TMP_SEL_D, items * w2, &T); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_E, items * w2, &U); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_F, items * w2, &u_inv); if (rc) return rc;
  rc = sel_t(ctx, k, lay, delta_enc, d_enc, r_a, aw, e, ew, rab, T, count); if (rc) return rc;
  rc = sc_modmul(ctx, k.mod_n2, T, w2, products, w2, U, items); if (rc) return rc;
  rc = sc_modinv(ctx, k.mod_n2, U, u_inv, items, nullptr); if (rc) return rc;
  return sc_select_finish_cx(ctx, k.mod_n2, nfields, T, products, u_inv, f_enc, g_enc, lo_index, hi_index, out, out_rows, count);
}

// ---- secure multiplication -------------------------------------------------------------------------------------------
// The selection's round trip with both factors blinded: P carries A = x + e_y and B_j = y_j + e_x_j, the key holder returns [[A B_j]],
// and [[x y_j]] = [[A B_j]] T_j^-1 with T_j = [[x]]^(e_x_j) [[y_j]]^(e_y) (1 + e_x_j e_y N).  Same temporaries as the selection's.
int sc_initiator_mul_pack(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int nfields, const int* wy_hptr, int is_signed,
                          const uint32_t* x_enc, const uint32_t* y_enc, const uint32_t* r_a, int aw, const uint32_t* r_b, int bw,
                          const uint32_t* rho_p, int ew, uint32_t* p_out, uint32_t* e_out, uint32_t* rab_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_mul_pack: bad key");
  const PaillierKey k = *kp;
  MulLayout lay;
  int rc = mul_layout(ctx, "sc_initiator_mul_pack", big_bits(k.n), kappa, wx, nfields, wy_hptr, is_signed, &lay); if (rc) return rc;
  if (!rho_p) return fail(ctx, SC_ERR_ARG, "sc_initiator_mul_pack: rho_p is required: P must carry a fresh rho^N");
  if (!x_enc || !y_enc || !r_a || !r_b || !p_out || !e_out || !rab_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_mul_pack: bad argument");
  rc = row_words(ctx, "sc_initiator_mul_pack", mul_ebits(lay), aw, bw, true, std::min(k.nw, MUL_FIELD_WORDS), ew); if (rc) return rc;
  if (count == 0) return SC_OK;
  uint32_t* R;
  rc = tmp_words(ctx, TMP_SEL_A, count * k.nw, &R); if (rc) return rc;
  if (launch_mul_prep(ctx->stream, r_a, aw, r_b, bw, lay, k.nw, ew, count, R, e_out, rab_out)) return fail(ctx, SC_ERR_HIP, "sc_initiator_mul_pack: launch failed");
  return pack_messages(ctx, k, paillier_key_id, column_fields(x_enc, y_enc, nfields, lay.s, lay.fbits, count, (size_t)count * 2 * k.nw), R, rho_p, p_out, count);
}

int sc_keyholder_mul(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int nfields, const int* wy_hptr, const uint32_t* p_enc,
                     const uint32_t* rho_products, uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !kp->secret) return fail(ctx, SC_ERR_ARG, "sc_keyholder_mul: needs the secret key");
  const PaillierKey k = *kp;
  MulLayout lay;
  int rc = mul_layout(ctx, "sc_keyholder_mul", big_bits(k.n), kappa, wx, nfields, wy_hptr, 0, &lay); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (!p_enc || !rho_products || !out) return fail(ctx, SC_ERR_ARG, "sc_keyholder_mul: bad argument");
  return keyholder_round(ctx, "sc_keyholder_mul", k, paillier_key_id, p_enc, rho_products, out, count, (uint64_t)nfields * count,
                         [&](const uint32_t* pl, uint32_t* prod, uint32_t* bad) { return launch_mul_split(ctx->stream, pl, k.nw, lay, count, prod, bad); },
                         "mul: a decrypted P exceeds the announced field layout (kappa or widths differ between the players)");
}

int sc_initiator_mul_finish(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int nfields, const int* wy_hptr, const uint32_t* x_enc,
                            const uint32_t* y_enc, const uint32_t* products, const uint32_t* e, int ew, const uint32_t* rab,
                            const uint32_t* base, int coef, uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_mul_finish: bad key");
  const PaillierKey k = *kp;
  MulLayout lay;
  int rc = mul_layout(ctx, "sc_initiator_mul_finish", big_bits(k.n), kappa, wx, nfields, wy_hptr, 0, &lay); if (rc) return rc;
  if (!x_enc || !y_enc || !products || !e || !rab || !out || ew < 1) return fail(ctx, SC_ERR_ARG, "sc_initiator_mul_finish: bad argument");
  rc = ratio_coef(ctx, "sc_initiator_mul_finish", coef); if (rc) return rc;
  rc = exp_rows(ctx, "sc_initiator_mul_finish", ew, mul_ebits(lay)); if (rc) return rc;
  if (count == 0) return SC_OK;
  const int w2 = 2 * k.nw;
  const uint64_t items = (uint64_t)nfields * count;
  uint32_t *T, *inv;
  rc = tmp_words(ctx, TMP_SEL_D, items * w2, &T); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_E, items * w2, &inv); if (rc) return rc;
  rc = two_base_t(ctx, k, nfields, mul_ebits(lay), x_enc, y_enc, e + items * ew /* e_y */, ew, e, ew, rab, T, count); if (rc) return rc;
  return finish_ratio(ctx, k, coef, products, T, base, out, items, inv);
}

// ---- secure inner product ----------------------------------------------------------------------------------------------
// The multiplication's round trip with k pairs per row: the key holder adds the products under the blinding and returns one ciphertext,
// [[sum_j x_j y_j]] = [[D]] T^-1 with D = sum_j A_j B_j and T = prod_j [[x_j]]^(b_j) [[y_j]]^(a_j) (1 + S N), S = sum_j a_j b_j.  A row's
// pairs are packed g to a message, pair j in message j mod M at position j div M, so the planes of one position are contiguous in
// x_enc [k][count][2 nw] and the messages that hold the (partial) top position are a prefix of P [M][count][2 nw].  Same temporaries as
// the selection's.
int sc_initiator_dot_pack(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int wy, int is_signed, int square, int kk, const uint32_t* x_enc,
                          const uint32_t* y_enc, const uint32_t* r_a, int aw, const uint32_t* r_b, int bw, const uint32_t* rho_p, int ew,
                          uint32_t* p_out, uint32_t* e_out, uint32_t* s_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_dot_pack: bad key");
  const PaillierKey k = *kp;
  DotLayout lay;
  int rc = dot_layout(ctx, "sc_initiator_dot_pack", big_bits(k.n), kappa, wx, wy, is_signed, square, kk, &lay); if (rc) return rc;
  if (!rho_p) return fail(ctx, SC_ERR_ARG, "sc_initiator_dot_pack: rho_p is required: every P must carry a fresh rho^N");
  if (!x_enc || !r_a || (!square && (!y_enc || !r_b)) || !p_out || !e_out || !s_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_dot_pack: bad argument");
  rc = row_words(ctx, "sc_initiator_dot_pack", lay.ebits, aw, bw, !square, MUL_FIELD_WORDS, ew); if (rc) return rc;
  if (count == 0) return SC_OK;
  const uint64_t items = (uint64_t)lay.M * count;      // the messages
  uint32_t* R;
  rc = tmp_words(ctx, TMP_SEL_A, items * k.nw, &R); if (rc) return rc;
  if (launch_dot_prep(ctx->stream, r_a, aw, r_b, bw, lay, k.nw, ew, count, e_out, R, s_out)) return fail(ctx, SC_ERR_HIP, "sc_initiator_dot_pack: launch failed");
  // x and y of position 0, x and y of position 1, ..; a message below the partial top position joins the chain as a copy of its field
  return pack_messages(ctx, k, paillier_key_id, dot_fields(x_enc, y_enc, square, kk, lay.M, lay.sa, lay.sb, count, (size_t)count * 2 * k.nw), R, rho_p, p_out, items);
}

int sc_keyholder_dot(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int wy, int square, int kk, const uint32_t* p_enc, const uint32_t* rho_d,
                     uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !kp->secret) return fail(ctx, SC_ERR_ARG, "sc_keyholder_dot: needs the secret key");
  const PaillierKey k = *kp;
  DotLayout lay;
  int rc = dot_layout(ctx, "sc_keyholder_dot", big_bits(k.n), kappa, wx, wy, 0, square, kk, &lay); if (rc) return rc;
  if (!p_enc || !rho_d || !out) return fail(ctx, SC_ERR_ARG, "sc_keyholder_dot: bad argument");
  if (count == 0) return SC_OK;
  return keyholder_round(ctx, "sc_keyholder_dot", k, paillier_key_id, p_enc, rho_d, out, (uint64_t)lay.M * count, count,
                         [&](const uint32_t* pl, uint32_t* D, uint32_t* bad) { return launch_dot_split(ctx->stream, pl, k.nw, lay, count, D, bad); },
                         "dot: a decrypted P exceeds the end of its message in the announced layout (kappa, widths, k or the mode differ between the players)");
}

// acc_out = acc_in * prod_j base_j^(e_j) over `planes` consecutive planes base [planes][count][2 nw], e [planes][count][ew]: groups of at
// most three planes per pair launch, alternating between the two halves of `pp` [2][count][2 nw]; *acc follows the running product.
// SC_ERR_UNSUPPORTED from the first group means that the key has no pair kernel with per-row exponents.
static int dot_t_side(sc_ctx* ctx, const PaillierKey& k, int planes, int ebits, const uint32_t* base, const uint32_t* e, int ew, uint32_t* pp,
                      const uint32_t** acc, uint64_t count) {
  const int w2 = 2 * k.nw;
  for (int j = 0; j < planes; j += 3) {
    uint32_t* dst = *acc == pp ? pp + (size_t)count * w2 : pp;
    int rc = sc_modexp_var_sq(ctx, k.mod_n, k.mod_n2, std::min(3, planes - j), base + (size_t)j * count * w2, w2, e + (size_t)j * count * ew, ew, ebits,
                              *acc, dst, count); if (rc) return rc;
    *acc = dst;
  }
  return SC_OK;
}

int sc_initiator_dot_finish(sc_ctx* ctx, int paillier_key_id, int kappa, int wx, int wy, int square, int kk, const uint32_t* x_enc,
                            const uint32_t* y_enc, const uint32_t* d_enc, const uint32_t* e, int ew, const uint32_t* s, const uint32_t* base,
                            int coef, uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_dot_finish: bad key");
  const PaillierKey k = *kp;
  DotLayout lay;
  int rc = dot_layout(ctx, "sc_initiator_dot_finish", big_bits(k.n), kappa, wx, wy, 0, square, kk, &lay); if (rc) return rc;
  if (!x_enc || (!square && !y_enc) || !d_enc || !e || !s || !out || ew < 1) return fail(ctx, SC_ERR_ARG, "sc_initiator_dot_finish: bad argument");
  rc = ratio_coef(ctx, "sc_initiator_dot_finish", coef); if (rc) return rc;
  rc = exp_rows(ctx, "sc_initiator_dot_finish", ew, lay.ebits); if (rc) return rc;
  if (count == 0) return SC_OK;
  const int w2 = 2 * k.nw;
  const size_t col = (size_t)count * w2;
  uint32_t *mi, *pp, *inv, *tmp;
  rc = tmp_words(ctx, TMP_SEL_A, col, &mi); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_D, 2 * col, &pp); if (rc) return rc;
  rc = tmp_words(ctx, TMP_SEL_E, col, &inv); if (rc) return rc;
  rc = sc_paillier_encrypt_raw(ctx, k.mod_n2, k.cst_n, s, k.nw, mi, count); if (rc) return rc;        // 1 + S N
  // T: the exponents' planes follow the bases' (e: the k planes of x, then the k planes of y)
  const uint32_t* T = mi;
  rc = k.pairs ? dot_t_side(ctx, k, kk, lay.ebits, x_enc, e, ew, pp, &T, count) : SC_ERR_UNSUPPORTED;
  if (rc == SC_OK && !square) rc = dot_t_side(ctx, k, kk, lay.ebits, y_enc, e + (size_t)kk * count * ew, ew, pp, &T, count);
  if (rc == SC_ERR_UNSUPPORTED) {
    rc = tmp_words(ctx, TMP_SEL_B, col, &tmp); if (rc) return rc;
    rc = pow_product_plain(ctx, k, kk, lay.ebits, x_enc, e, ew, tmp, mi, mi, count);
    if (rc == SC_OK && !square) rc = pow_product_plain(ctx, k, kk, lay.ebits, y_enc, e + (size_t)kk * count * ew, ew, tmp, mi, mi, count);
    T = mi;
  }
  if (rc) return rc;
  return finish_ratio(ctx, k, coef, d_enc, T, base, out, count, inv);
}

// ---- secure one-hot encoding -------------------------------------------------------------------------------------------
// Blind, decrypt, rotate: P carries the fields d_q = i_q + r_q, the key holder returns the k fresh encryptions [[ [t == d_q mod k] ]] of
// every index, and since d_q mod k = (i_q + r_q) mod k the initiator reads row (t + r_q mod k) mod k as row t -- no arithmetic modulo N^2
// after the key holder's answer.  Index q lives in message q div g at position q mod g, so the planes of one position are NOT contiguous
// in index_enc [m][count][2 nw] once a row takes more than one message: they are gathered position by position (TMP_SEL_D) before the
// shared packer runs.  Same temporaries as the selection's.
int sc_initiator_onehot_pack(sc_ctx* ctx, int paillier_key_id, int kappa, int ib, int kk, int m, const uint32_t* index_enc, const uint32_t* r,
                             int rw, const uint32_t* rho_p, uint32_t* p_out, int32_t* rot_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: bad key");
  const PaillierKey k = *kp;
  OnehotLayout lay;
  int rc = onehot_layout(ctx, "sc_initiator_onehot_pack", big_bits(k.n), kappa, ib, kk, m, &lay); if (rc) return rc;
  if (!index_enc) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: index_enc: missing array");
  if (!r) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: r: missing array");
  rc = onehot_mask_words(ctx, "sc_initiator_onehot_pack", lay, rw); if (rc) return rc;
  if (!rho_p) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: rho_p is required: every P must carry a fresh rho^N");
  if (!p_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: p_out: missing array");
  if (!rot_out) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_pack: rot_out: missing array");
  rc = onehot_rows(ctx, "sc_initiator_onehot_pack", kk, m, count); if (rc) return rc;
  if (count == 0) return SC_OK;
  const int M = lay.M, g = lay.g;
  const size_t col = (size_t)count * 2 * k.nw;         // one plane
  const uint64_t items = (uint64_t)M * count;          // the messages
  uint32_t *R, *gat = nullptr;
  rc = tmp_words(ctx, TMP_SEL_A, items * k.nw, &R); if (rc) return rc;
  if (launch_onehot_prep(ctx->stream, r, rw, lay, k.nw, count, R, rot_out)) return fail(ctx, SC_ERR_HIP, "sc_initiator_onehot_pack: launch failed");
  if (M > 1) { rc = tmp_words(ctx, TMP_SEL_D, (uint64_t)m * col, &gat); if (rc) return rc; }
  const std::vector<PackField> fld = onehot_fields(M > 1 ? gat : index_enc, m, g, M, lay.f, count, col);
  // the gather: the planes of one position sit g planes apart in index_enc and become consecutive rows of their field
  for (size_t pos = 0; gat && pos < fld.size(); pos++)
    for (size_t mm = 0; mm * count < fld[pos].held; mm++)
      HIPCHK(ctx, hipMemcpyAsync(gat + (fld[pos].rows - gat) + mm * col, index_enc + (mm * g + pos) * col, col * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return pack_messages(ctx, k, paillier_key_id, fld, R, rho_p, p_out, items);
}

int sc_keyholder_onehot(sc_ctx* ctx, int paillier_key_id, int kappa, int ib, int kk, int m, const uint32_t* p_enc, const uint32_t* rho_e,
                        uint32_t* e_out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !kp->secret) return fail(ctx, SC_ERR_ARG, "sc_keyholder_onehot: needs the secret key");
  const PaillierKey k = *kp;
  OnehotLayout lay;
  int rc = onehot_layout(ctx, "sc_keyholder_onehot", big_bits(k.n), kappa, ib, kk, m, &lay); if (rc) return rc;
  if (!p_enc) return fail(ctx, SC_ERR_ARG, "sc_keyholder_onehot: p_enc: missing array");
  if (!rho_e) return fail(ctx, SC_ERR_ARG, "sc_keyholder_onehot: rho_e: missing array");
  if (!e_out) return fail(ctx, SC_ERR_ARG, "sc_keyholder_onehot: e_out: missing array");
  rc = onehot_rows(ctx, "sc_keyholder_onehot", kk, m, count); if (rc) return rc;
  if (count == 0) return SC_OK;
  return keyholder_round(ctx, "sc_keyholder_onehot", k, paillier_key_id, p_enc, rho_e, e_out, (uint64_t)lay.M * count, (uint64_t)m * kk * count,
                         [&](const uint32_t* pl, uint32_t* prod, uint32_t* bad) { return launch_onehot_split(ctx->stream, pl, k.nw, lay, count, prod, bad); },
                         "onehot: a decrypted P exceeds the end of its message in the announced layout (kappa, ib or m differ between the players)");
}

int sc_initiator_onehot_finish(sc_ctx* ctx, int paillier_key_id, int kappa, int ib, int kk, int m, const uint32_t* e_enc, const int32_t* rot,
                               uint32_t* out, uint64_t count) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_finish: bad key");
  OnehotLayout lay;
  int rc = onehot_layout(ctx, "sc_initiator_onehot_finish", big_bits(kp->n), kappa, ib, kk, m, &lay); if (rc) return rc;
  if (!e_enc) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_finish: e_enc: missing array");
  if (!rot) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_finish: rot: missing array");
  if (!out) return fail(ctx, SC_ERR_ARG, "sc_initiator_onehot_finish: out: missing array");
  rc = onehot_rows(ctx, "sc_initiator_onehot_finish", kk, m, count); if (rc) return rc;
  return onehot_rotate(ctx, "sc_initiator_onehot_finish", 2 * kp->nw, kk, m, e_enc, rot, out, count);
}

// ---- secure division by public divisors ------------------------------------------------------------------------------
// one pinned, device-visible word per context for k_divmod_words' zero-divisor verdict (the selection's verdict word's twin)
static int div_verdict_word(sc_ctx* ctx, uint32_t** out) {
  auto* ks = keys_of(ctx);
  if (!ks->div_verdict) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc((void**)&ks->div_verdict, sizeof(uint32_t), hipHostMallocMapped));
    *(volatile uint32_t*)ks->div_verdict = 0;
  }
  *out = ks->div_verdict;
  return SC_OK;
}
static bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

int sc_plain_divmod(sc_ctx* ctx, const uint32_t* x, int nw, const uint64_t* d, uint64_t count, uint32_t* q, uint64_t* rem) {
  if (!ctx) return SC_ERR_ARG;
  if (!x || !d || !q || !rem) return fail(ctx, SC_ERR_ARG, "sc_plain_divmod: null pointer");
  if (nw < 1) return fail(ctx, SC_ERR_ARG, "sc_plain_divmod: nw = %d: expected at least one word per row", nw);
  if (count == 0) return SC_OK;
  const size_t rows = (size_t)count * nw * 4, words = (size_t)count * 8;
  if (q != x && bytes_overlap(q, rows, x, rows))
    return fail(ctx, SC_ERR_ARG, "sc_plain_divmod: q partly overlaps x (q is x itself, in place, or an array apart from it)");
  if (bytes_overlap(rem, words, x, rows) || bytes_overlap(rem, words, q, rows) || bytes_overlap(d, words, q, rows) || bytes_overlap(d, words, rem, words))
    return fail(ctx, SC_ERR_ARG, "sc_plain_divmod: rem overlaps x, q or d, or d overlaps q");
  uint32_t* bad;
  int rc = div_verdict_word(ctx, &bad); if (rc) return rc;
  if (launch_divmod_words(ctx->stream, x, nw, d, count, q, rem, bad)) return fail(ctx, SC_ERR_HIP, "sc_plain_divmod: launch failed");
  return SC_OK;
}

int sc_div_fits(int nbits_n, int kappa, int x_bits, int is_signed) {
  if (kappa < 1 || kappa > 62 || x_bits < 1) return 0;
  // signed: the dividend is x + c d with c = ceil(2^x_bits / d), below 2^(x_bits + 2) where d <= 2^x_bits and below 2 d < 2^65 elsewhere
  const long long width = is_signed ? std::max<long long>((long long)x_bits + 2, 65) : x_bits;
  return width + kappa + 2 < (long long)nbits_n - 1 ? 1 : 0;
}

int sc_initiator_div_blind(sc_ctx* ctx, int paillier_key_id, int kappa, int x_bits, int is_signed, const uint32_t* x_enc, const uint32_t* r,
                           const uint32_t* rho, int flags, const uint64_t* d, uint32_t* z_out, uint32_t* rq, uint64_t* rm, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !x_enc || !r || !rho || !d || !z_out || !rq || !rm) return fail(ctx, SC_ERR_ARG, "sc_initiator_div_blind: bad argument");
  const PaillierKey k = *kp;
  if (!sc_div_fits(big_bits(k.n), kappa, x_bits, is_signed))
    return fail(ctx, SC_ERR_ARG, "sc_initiator_div_blind: x_bits = %d (%s), kappa = %d: the blinded dividend does not fit below a %d-bit N", x_bits,
                is_signed ? "signed" : "unsigned", kappa, big_bits(k.n));
  const int w2 = 2 * k.nw;
  const Prog* p;                                                          // the packing program of the four families: [[x + r]]
  int rc = cached_prog(ctx, "selpk:" + std::to_string(k.mod_n2) + ":" + std::to_string(k.cst_n), k.mod_n2, [&](Builder& bd) {
    const int cn = bd.use_const(k.cst_n);
    bd.loadw(1, 0, 0, k.nw); bd.mul_const(cn); bd.add1();                 // [[r]] = 1 + r N
    bd.mul_const(0); bd.mul_extw(0);                                      // [[x + r]]
    bd.storew(2);
  }, &p); if (rc) return rc;
  VmExt ex[3] = {mk_ext(x_enc, w2, w2), mk_ext(r, k.nw, k.nw), mk_ext(z_out, w2, w2)};
  rc = run_vm(ctx, k.mod_n2, *p, ex, 3, count); if (rc) return rc;
  if (flags & SC_STEP_RANDOMIZERS_READY) rc = sc_modmul(ctx, k.mod_n2, z_out, w2, rho, w2, z_out, count);
  else rc = sc_paillier_randomize(ctx, paillier_key_id, z_out, rho, z_out, count);
  if (rc) return rc;
  return sc_plain_divmod(ctx, r, k.nw, d, count, rq, rm);
}

int sc_keyholder_div_open(sc_ctx* ctx, int paillier_key_id, const uint32_t* z_enc, const uint64_t* d, uint32_t* zq, uint64_t* zm, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !z_enc || !d || !zq || !zm) return fail(ctx, SC_ERR_ARG, "sc_keyholder_div_open: bad argument");
  const int nw = kp->nw;
  int rc = sc_paillier_decrypt(ctx, paillier_key_id, z_enc, zq, count); if (rc) return rc;      // z, divided where it stands
  return sc_plain_divmod(ctx, zq, nw, d, count, zq, zm);
}

int sc_clock_probe(sc_ctx* ctx, int paillier_key_id, const uint32_t* rho, uint64_t count, double* out_ghz, double* out_ms) {
  const PaillierKey* kp = paillier_key(ctx, paillier_key_id);
  if (!kp || !rho || count == 0 || !out_ghz) return fail(ctx, SC_ERR_ARG, "sc_clock_probe: bad argument");
  const PaillierKey k = *kp;
  if ((k.secret && k.crt) || !k.pairs || sc_mod_supports_sq(ctx, k.mod_n) != 1)
    return fail(ctx, SC_ERR_ARG, "sc_clock_probe: needs a public Paillier key with pair arithmetic (the dominant launch)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t max_waves = (size_t)ctx->num_cu * 16;
  DevBuf<uint64_t> d_st; DevBuf<uint32_t> d_out;
  HIPCHK(ctx, hipMalloc((void**)&d_st.p, max_waves * 4 * sizeof(uint64_t)));
  if (hipMalloc((void**)&d_out.p, (size_t)count * 2 * k.nw * 4) != hipSuccess) return fail(ctx, SC_ERR_HIP, "sc_clock_probe: out of memory");
  LaunchTimer timer(ctx);
  (void)hipMemsetAsync(d_st.p, 0, max_waves * 4 * sizeof(uint64_t), ctx->stream);
  PolicyOverride keep(ctx);                                      // the probe's launches stay out of the MAC counter
  ctx->stamps = d_st.p; ctx->stamp_grid = 0;
  float ms = 0;
  const int rc = timer.time([&] { return sc_paillier_randomize(ctx, paillier_key_id, nullptr, rho, d_out.p, count); }, &ms);
  ctx->stamps = nullptr;
  if (rc) return rc;
  const uint32_t grid = ctx->stamp_grid;
  if (grid == 0) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_clock_probe: this batch did not take the (4,18) modulus-multiple pair launch");
  std::vector<uint64_t> st((size_t)grid * 4);
  HIPCHK(ctx, hipMemcpyAsync(st.data(), d_st.p, st.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rate_khz = 0;                                              // rate of s_memrealtime
  if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || rate_khz <= 0) rate_khz = 100000;
  double sum = 0; uint64_t used = 0;
  for (uint32_t w = 0; w < grid; w++) {
    const uint64_t dc = st[4 * w + 2] - st[4 * w], dr = st[4 * w + 3] - st[4 * w + 1];
    if (dr > 0 && st[4 * w + 3] != 0) { sum += (double)dc / (double)dr; used++; }
  }
  if (!used) return fail(ctx, SC_ERR_HIP, "sc_clock_probe: no wave recorded its clocks");
  *out_ghz = sum / (double)used * (double)rate_khz * 1e3 / 1e9;
  if (out_ms) *out_ms = ms;
  return SC_OK;
}

}  // extern "C"

int sc_host::div_verdict_check(sc_ctx* ctx) {
  auto* ks = (sc_scheme_keys*)ctx->scheme_keys;
  if (!ks || !ks->div_verdict || !*(volatile uint32_t*)ks->div_verdict) return SC_OK;
  *(volatile uint32_t*)ks->div_verdict = 0;
  return fail(ctx, SC_ERR_ARG, "sc_plain_divmod: a divisor is zero (the row's quotient and remainder were written as zero)");
}

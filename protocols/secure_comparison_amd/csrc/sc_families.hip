// Secure selection, multiplication, inner product and one-hot encoding: each family's layout rule on the
// host and the plaintext-word halves of its two players (k_*_prep / k_*_split, the one-hot's k_onehot_rotate); the compare-exchange
// finish of a sort (§8c).  The scheme-level entries of the four families (sc_schemes.hip) check the same layouts before they launch
// anything: the layout rules and refusals they share are declared, with their comments, in sc_host.h.  Host code only.
#include "sc_host.h"

using namespace sc;
using namespace sc_host;

// The one field-packing rule of the selection and the multiplication: a low field of s bits, then nf fields of
// fbits_j = widths_j + kappa + fbits_extra bits; every s + fbits_j and the end of the last field stay below bits(N) - 1.  Every refusal
// names its column.
static int pack_fields(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int s, int nf, const int* widths, int max_width, int fbits_extra,
                       const char* product_label, int* off, int* fbits, int* end) {
  if (!widths || nf < 1 || nf > SEL_MAX_FIELDS)
    return fail(ctx, SC_ERR_ARG, "%s: %d columns: expected 1 .. %d with their widths", who, nf, SEL_MAX_FIELDS);
  int o = s;
  for (int j = 0; j < nf; j++) {
    if (widths[j] < 1 || widths[j] > max_width) return fail(ctx, SC_ERR_ARG, "%s: column %d: width %d: expected 1 .. %d", who, j, widths[j], max_width);
    fbits[j] = widths[j] + kappa + fbits_extra; off[j] = o;
    if (s + fbits[j] >= nbits_n - 1)
      return fail(ctx, SC_ERR_ARG, "%s: column %d: the product %s (%d bits) does not fit below a %d-bit N", who, j, product_label, s + fbits[j], nbits_n);
    o += fbits[j];
    if (o >= nbits_n - 1)
      return fail(ctx, SC_ERR_ARG, "%s: column %d: the packed fields (%d bits) do not fit below a %d-bit N (kappa = %d)", who, j, o, nbits_n, kappa);
  }
  *end = o;
  return SC_OK;
}

// ---- secure selection: the plaintext-word halves of the two players (k_select_prep / k_select_split) -------------------------------
int sc_host::select_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int nfields, const int* widths, SelLayout* lay) {
  if (kappa < 1 || kappa > 62) return fail(ctx, SC_ERR_ARG, "%s: kappa = %d: expected 1 <= kappa <= 62", who, kappa);
  lay->s = kappa + 1; lay->nf = nfields;
  int rc = pack_fields(ctx, who, nbits_n, kappa, lay->s, nfields, widths, 4096, 2, "a * b", lay->off, lay->fbits, &lay->end); if (rc) return rc;
  std::copy(widths, widths + nfields, lay->width);
  return SC_OK;
}

extern "C" int sc_select_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int nfields, const int* widths_hptr, const uint32_t* r_a,
                   int aw, const uint32_t* r_b, int bw, int ew, uint32_t* R, uint32_t* e, uint32_t* rab, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!ctx || !n_hptr || nw <= 0 || !r_a || !r_b || !R || !e || !rab || aw < 1 || aw > 2 || bw < 1 || ew < 1)
    return fail(ctx, SC_ERR_ARG, "sc_select_prep: bad argument");
  SelLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = select_layout(ctx, "sc_select_prep", big_bits(n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  if (bw > nw) return fail(ctx, SC_ERR_ARG, "sc_select_prep: r_b rows of %d words are wider than N (%d words)", bw, nw);
  for (int j = 0; j < nfields; j++)
    if (32 * ew < lay.fbits[j]) return fail(ctx, SC_ERR_ARG, "sc_select_prep: exponent rows of %d words are too narrow", ew);
  if (launch_select_prep(ctx->stream, r_a, aw, r_b, bw, lay, nw, ew, count, R, e, rab)) return fail(ctx, SC_ERR_HIP, "sc_select_prep: launch failed");
  return SC_OK;
}

extern "C" int sc_select_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int nfields, const int* widths_hptr, const uint32_t* p,
                    uint32_t* prod, uint32_t* bad, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!ctx || !n_hptr || nw <= 0 || !p || !prod || !bad) return fail(ctx, SC_ERR_ARG, "sc_select_split: bad argument");
  SelLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = select_layout(ctx, "sc_select_split", big_bits(n), kappa, nfields, widths_hptr, &lay); if (rc) return rc;
  if (launch_select_split(ctx->stream, p, nw, lay, count, prod, bad)) return fail(ctx, SC_ERR_HIP, "sc_select_split: launch failed");
  return SC_OK;
}

// ---- secure multiplication: the plaintext-word halves of the two players (k_mul_prep / k_mul_split) ---------------
int sc_host::mul_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int wx, int nfields, const int* wy, int is_signed, MulLayout* lay) {
  if (kappa < 1 || kappa > 62) return fail(ctx, SC_ERR_ARG, "%s: kappa = %d: expected 1 <= kappa <= 62", who, kappa);
  if (wx < 1 || wx > MUL_MAX_WIDTH) return fail(ctx, SC_ERR_ARG, "%s: wx = %d: expected 1 .. %d", who, wx, MUL_MAX_WIDTH);
  lay->s = wx + kappa + 1; lay->nf = nfields; lay->wx = wx; lay->is_signed = is_signed ? 1 : 0;
  int rc = pack_fields(ctx, who, nbits_n, kappa, lay->s, nfields, wy, MUL_MAX_WIDTH, 1, "A * B", lay->off, lay->fbits, &lay->end); if (rc) return rc;
  std::copy(wy, wy + nfields, lay->wy);
  return SC_OK;
}
int sc_host::mul_ebits(const MulLayout& lay) { int b = lay.s; for (int j = 0; j < lay.nf; j++) b = std::max(b, lay.fbits[j]); return b; }
int sc_host::exp_rows(sc_ctx* ctx, const char* who, int ew, int bits) {
  return 32 * ew < bits ? fail(ctx, SC_ERR_ARG, "%s: exponent rows of %d words are too narrow for %d bits", who, ew, bits) : SC_OK;
}
int sc_host::ratio_coef(sc_ctx* ctx, const char* who, int coef) {
  return coef != 1 && coef != -1 && coef != -2 ? fail(ctx, SC_ERR_ARG, "%s: coef = %d: expected +1, -1 or -2", who, coef) : SC_OK;
}
int sc_host::row_words(sc_ctx* ctx, const char* who, int ebits, int aw, int bw, bool has_b, int bw_max, int ew) {
  if (aw < 1 || aw > MUL_FIELD_WORDS || (has_b && (bw < 1 || bw > bw_max)) || ew < 1)
    return fail(ctx, SC_ERR_ARG, "%s: rows of %d (r_a), %d (r_b), %d (e) words: expected 1 .. %d for the draws", who, aw, bw, ew, MUL_FIELD_WORDS);
  return exp_rows(ctx, who, ew, ebits);
}

extern "C" int sc_mul_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int nfields, const int* wy_hptr, int is_signed,
                const uint32_t* r_a, int aw, const uint32_t* r_b, int bw, int ew, uint32_t* R, uint32_t* e, uint32_t* rab, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!ctx || !n_hptr || nw <= 0 || !r_a || !r_b || !R || !e || !rab) return fail(ctx, SC_ERR_ARG, "sc_mul_prep: bad argument");
  MulLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = mul_layout(ctx, "sc_mul_prep", big_bits(n), kappa, wx, nfields, wy_hptr, is_signed, &lay); if (rc) return rc;
  rc = row_words(ctx, "sc_mul_prep", mul_ebits(lay), aw, bw, true, std::min(nw, MUL_FIELD_WORDS), ew); if (rc) return rc;
  if (launch_mul_prep(ctx->stream, r_a, aw, r_b, bw, lay, nw, ew, count, R, e, rab)) return fail(ctx, SC_ERR_HIP, "sc_mul_prep: launch failed");
  return SC_OK;
}

extern "C" int sc_mul_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int nfields, const int* wy_hptr, const uint32_t* p,
                 uint32_t* prod, uint32_t* bad, uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!ctx || !n_hptr || nw <= 0 || !p || !prod || !bad) return fail(ctx, SC_ERR_ARG, "sc_mul_split: bad argument");
  MulLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = mul_layout(ctx, "sc_mul_split", big_bits(n), kappa, wx, nfields, wy_hptr, 0, &lay); if (rc) return rc;
  if (launch_mul_split(ctx->stream, p, nw, lay, count, prod, bad)) return fail(ctx, SC_ERR_HIP, "sc_mul_split: launch failed");
  return SC_OK;
}

// ---- secure inner product: the plaintext-word halves of the two players (k_dot_prep / k_dot_split) -----------------
int sc_host::dot_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int wx, int wy, int is_signed, int square, int k, DotLayout* lay) {
  if (kappa < 1 || kappa > 62) return fail(ctx, SC_ERR_ARG, "%s: kappa = %d: expected 1 <= kappa <= 62", who, kappa);
  if (wx < 1 || wx > MUL_MAX_WIDTH) return fail(ctx, SC_ERR_ARG, "%s: wx = %d: expected 1 .. %d", who, wx, MUL_MAX_WIDTH);
  if (!square && (wy < 1 || wy > MUL_MAX_WIDTH)) return fail(ctx, SC_ERR_ARG, "%s: wy = %d: expected 1 .. %d", who, wy, MUL_MAX_WIDTH);
  if (k < 1 || k > DOT_MAX_K) return fail(ctx, SC_ERR_ARG, "%s: k = %d: expected 1 .. %d pairs per row", who, k, DOT_MAX_K);
  lay->wx = wx; lay->wy = square ? 0 : wy; lay->is_signed = is_signed ? 1 : 0; lay->square = square ? 1 : 0; lay->k = k;
  lay->sa = wx + kappa + 1; lay->sb = square ? 0 : wy + kappa + 1; lay->pb = lay->sa + lay->sb;
  lay->ebits = square ? lay->sa + 1 : std::max(lay->sa, lay->sb);
  lay->g = nbits_n >= 2 ? (nbits_n - 2) / lay->pb : 0;
  if (lay->g < 1) return fail(ctx, SC_ERR_ARG, "%s: pb = %d: one pair does not fit below a %d-bit N (kappa = %d)", who, lay->pb, nbits_n, kappa);
  const int prod = square ? 2 * lay->sa : lay->pb;
  int lg = 0;
  while ((1 << lg) < k) lg++;
  if (prod + lg >= nbits_n - 1)
    return fail(ctx, SC_ERR_ARG, "%s: the sum of k = %d products (%d + %d bits) does not fit below a %d-bit N", who, k, prod, lg, nbits_n);
  lay->M = (k + lay->g - 1) / lay->g;
  return SC_OK;
}

extern "C" int sc_dot_layout(int nbits_n, int kappa, int wx, int wy, int is_signed, int square, int k, int* out) {
  DotLayout lay;
  if (!out) return SC_ERR_ARG;
  int rc = dot_layout(nullptr, "sc_dot_layout", nbits_n, kappa, wx, wy, is_signed, square, k, &lay); if (rc) return rc;
  out[0] = lay.sa; out[1] = lay.sb; out[2] = lay.pb; out[3] = lay.g; out[4] = lay.M; out[5] = lay.ebits;
  return SC_OK;
}

extern "C" int sc_dot_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int wy, int is_signed, int square, int k, const uint32_t* r_a,
                int aw, const uint32_t* r_b, int bw, int ew, uint32_t* e, uint32_t* R, uint32_t* S, uint64_t count) {
  if (!ctx || !n_hptr || nw <= 0) return fail(ctx, SC_ERR_ARG, "sc_dot_prep: bad argument");
  DotLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = dot_layout(ctx, "sc_dot_prep", big_bits(n), kappa, wx, wy, is_signed, square, k, &lay); if (rc) return rc;
  if (!r_a || (!square && !r_b) || !e || !R || !S) return fail(ctx, SC_ERR_ARG, "sc_dot_prep: bad argument");
  rc = row_words(ctx, "sc_dot_prep", lay.ebits, aw, bw, !square, MUL_FIELD_WORDS, ew); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (launch_dot_prep(ctx->stream, r_a, aw, r_b, bw, lay, nw, ew, count, e, R, S)) return fail(ctx, SC_ERR_HIP, "sc_dot_prep: launch failed");
  return SC_OK;
}

extern "C" int sc_dot_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int wy, int square, int k, const uint32_t* p, uint32_t* D,
                 uint32_t* bad, uint64_t count) {
  if (!ctx || !n_hptr || nw <= 0) return fail(ctx, SC_ERR_ARG, "sc_dot_split: bad argument");
  DotLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = dot_layout(ctx, "sc_dot_split", big_bits(n), kappa, wx, wy, 0, square, k, &lay); if (rc) return rc;
  if (!p || !D || !bad) return fail(ctx, SC_ERR_ARG, "sc_dot_split: bad argument");
  if (count == 0) return SC_OK;
  if (launch_dot_split(ctx->stream, p, nw, lay, count, D, bad)) return fail(ctx, SC_ERR_HIP, "sc_dot_split: launch failed");
  return SC_OK;
}

// ---- secure one-hot encoding: the plaintext-word kernels of the two players (k_onehot_prep / _split / _rotate) ---------
int sc_host::onehot_layout(sc_ctx* ctx, const char* who, int nbits_n, int kappa, int ib, int k, int m, OnehotLayout* lay) {
  if (kappa < 1 || kappa > 62) return fail(ctx, SC_ERR_ARG, "%s: kappa = %d: expected 1 <= kappa <= 62", who, kappa);
  if (ib < 1 || ib > 32) return fail(ctx, SC_ERR_ARG, "%s: ib = %d: expected an index width of 1 .. 32 bits", who, ib);
  if (k < 1 || k > ONEHOT_MAX_K) return fail(ctx, SC_ERR_ARG, "%s: k = %d: expected a table length of 1 .. %d", who, k, ONEHOT_MAX_K);
  if (m < 1 || m > ONEHOT_MAX_M) return fail(ctx, SC_ERR_ARG, "%s: m = %d: expected 1 .. %d indices per row", who, m, ONEHOT_MAX_M);
  lay->kappa = kappa; lay->ib = ib; lay->k = k; lay->m = m;
  lay->f = ib + kappa + 1; lay->rw = (ib + kappa + 31) / 32;
  if (lay->f >= nbits_n - 1)
    return fail(ctx, SC_ERR_ARG, "%s: f = %d: one field does not fit below a %d-bit N (kappa = %d)", who, lay->f, nbits_n, kappa);
  lay->g = std::max(1, (nbits_n - 2) / lay->f);
  lay->M = (m + lay->g - 1) / lay->g;
  return SC_OK;
}
int sc_host::onehot_rows(sc_ctx* ctx, const char* who, int k, int m, uint64_t count) {
  if (count > (uint64_t)0x7fffffff / ((uint64_t)k * m))
    return fail(ctx, SC_ERR_ARG, "%s: m k count = %d * %d * %llu rows: expected fewer than 2^31", who, m, k, (unsigned long long)count);
  return SC_OK;
}
int sc_host::onehot_mask_words(sc_ctx* ctx, const char* who, const OnehotLayout& lay, int rw) {
  if (rw < lay.rw) return fail(ctx, SC_ERR_ARG, "%s: draw rows of %d words are too narrow for %d bits", who, rw, lay.ib + lay.kappa);
  if (rw > ONEHOT_FIELD_WORDS) return fail(ctx, SC_ERR_ARG, "%s: draw rows of %d words: expected at most %d", who, rw, ONEHOT_FIELD_WORDS);
  return SC_OK;
}

extern "C" int sc_onehot_layout(int nbits_n, int kappa, int ib, int k, int m, int* out) {
  OnehotLayout lay;
  if (!out) return SC_ERR_ARG;
  int rc = onehot_layout(nullptr, "sc_onehot_layout", nbits_n, kappa, ib, k, m, &lay); if (rc) return rc;
  out[0] = lay.f; out[1] = lay.g; out[2] = lay.M; out[3] = lay.rw;
  return SC_OK;
}

extern "C" int sc_onehot_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int ib, int k, int m, const uint32_t* r, int rw, uint32_t* R,
                   int32_t* rot, uint64_t count) {
  if (!ctx || !n_hptr || nw <= 0) return fail(ctx, SC_ERR_ARG, "sc_onehot_prep: bad argument");
  OnehotLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = onehot_layout(ctx, "sc_onehot_prep", big_bits(n), kappa, ib, k, m, &lay); if (rc) return rc;
  if (!r || !R || !rot) return fail(ctx, SC_ERR_ARG, "sc_onehot_prep: bad argument");
  rc = onehot_mask_words(ctx, "sc_onehot_prep", lay, rw); if (rc) return rc;
  rc = onehot_rows(ctx, "sc_onehot_prep", k, m, count); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (launch_onehot_prep(ctx->stream, r, rw, lay, nw, count, R, rot)) return fail(ctx, SC_ERR_HIP, "sc_onehot_prep: launch failed");
  return SC_OK;
}

extern "C" int sc_onehot_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int ib, int k, int m, const uint32_t* p, uint32_t* prod,
                    uint32_t* bad, uint64_t count) {
  if (!ctx || !n_hptr || nw <= 0) return fail(ctx, SC_ERR_ARG, "sc_onehot_split: bad argument");
  OnehotLayout lay;
  Big n(n_hptr, n_hptr + nw);
  int rc = onehot_layout(ctx, "sc_onehot_split", big_bits(n), kappa, ib, k, m, &lay); if (rc) return rc;
  if (!p || !prod || !bad) return fail(ctx, SC_ERR_ARG, "sc_onehot_split: bad argument");
  rc = onehot_rows(ctx, "sc_onehot_split", k, m, count); if (rc) return rc;
  if (count == 0) return SC_OK;
  if (launch_onehot_split(ctx->stream, p, nw, lay, count, prod, bad)) return fail(ctx, SC_ERR_HIP, "sc_onehot_split: launch failed");
  return SC_OK;
}

int sc_host::onehot_rotate(sc_ctx* ctx, const char* who, int words, int k, int m, const uint32_t* e, const int32_t* rot, uint32_t* out, uint64_t count) {
  const uint64_t total = (uint64_t)m * k * count * words;
  if (out < e + total && e < out + total) return fail(ctx, SC_ERR_ARG, "%s: out overlaps e: the rotation is not done in place", who);
  if (count == 0) return SC_OK;
  if (launch_onehot_rotate(ctx->stream, e, rot, k, m, words, count, out)) return fail(ctx, SC_ERR_HIP, "%s: launch failed", who);
  return SC_OK;
}

extern "C" int sc_onehot_rotate(sc_ctx* ctx, int words, int k, int m, const uint32_t* e, const int32_t* rot, uint32_t* out, uint64_t count) {
  if (!ctx || words < 1) return fail(ctx, SC_ERR_ARG, "sc_onehot_rotate: bad argument");
  if (k < 1 || k > ONEHOT_MAX_K) return fail(ctx, SC_ERR_ARG, "sc_onehot_rotate: k = %d: expected a table length of 1 .. %d", k, ONEHOT_MAX_K);
  if (m < 1 || m > ONEHOT_MAX_M) return fail(ctx, SC_ERR_ARG, "sc_onehot_rotate: m = %d: expected 1 .. %d indices per row", m, ONEHOT_MAX_M);
  if (!e || !rot || !out) return fail(ctx, SC_ERR_ARG, "sc_onehot_rotate: bad argument");
  int rc = onehot_rows(ctx, "sc_onehot_rotate", k, m, count); if (rc) return rc;
  return onehot_rotate(ctx, "sc_onehot_rotate", words, k, m, e, rot, out, count);
}

// ---- compare-exchange finish of a secure sort: both outputs of every column from one shared inversion ----------
// The nf columns run as flat items (nf * count of them), so the program does not depend on nf and an index row entry is read at the
// item's flat number.  Per item, with V = U^-1 R^3 (one product, shared by both outputs): hi = F ab ab V / R^3 = F ab^2 U^-1 and
// lo = G T T V / R^3 = G T^2 U^-1 -- seven Montgomery products on operands loaded once.
extern "C" int sc_select_finish_cx(sc_ctx* ctx, int mod, int nfields, const uint32_t* t, const uint32_t* ab, const uint32_t* u_inv, const uint32_t* f,
                        const uint32_t* g, const uint64_t* lo_index, const uint64_t* hi_index, uint32_t* out, uint64_t out_rows,
                        uint64_t count) {
  if (ctx && count == 0) return SC_OK;
  if (!valid_mod(ctx, mod) || nfields < 1 || nfields > SEL_MAX_FIELDS || !t || !ab || !u_inv || !f || !g || !out ||
      (!lo_index) != (!hi_index))
    return fail(ctx, SC_ERR_ARG, "sc_select_finish_cx: bad argument");
  const uint64_t items = (uint64_t)nfields * count;
  const bool indexed = lo_index != nullptr;
  if (!indexed && out_rows < 2 * items)
    return fail(ctx, SC_ERR_ARG, "sc_select_finish_cx: out holds %llu rows, the contiguous [2][nf][count] form needs %llu",
                (unsigned long long)out_rows, (unsigned long long)(2 * items));
  const Mod& m = ctx->mods[mod];
  int cid;
  {
    Big one(m.nwords, 0); one[0] = 1;
    int rc = sc_const_create_cached(ctx, mod, big_shl_mod(one, m.n, 3 * m.W * m.S), &cid); if (rc) return rc;   // R^3 mod n
  }
  const Prog* p;
  int rc = cached_prog(ctx, "cxfin:" + std::to_string(mod) + ":" + std::to_string(indexed ? 1 : 0), mod, [&](Builder& bd) {
    bd.loadw(2); bd.mul_const(bd.use_const(cid)); bd.stt(0);        // V = U^-1 R^3
    bd.loadw(3); bd.mul_extw(1); bd.mul_extw(1); bd.mul_tbl(0);     // hi = F ab^2 U^-1
    if (indexed) bd.storew_at(5, 7); else bd.storew(5, 1);
    bd.loadw(4); bd.mul_extw(0); bd.mul_extw(0); bd.mul_tbl(0);     // lo = G T^2 U^-1
    if (indexed) bd.storew_at(5, 6); else bd.storew(5, 0);
  }, &p); if (rc) return rc;
  const uint32_t nw = m.nwords;
  VmExt ex[8] = {mk_ext(t, nw, nw), mk_ext(ab, nw, nw), mk_ext(u_inv, nw, nw), mk_ext(f, nw, nw), mk_ext(g, nw, nw),
                 mk_ext(out, nw, nw, out_rows), mk_ext(lo_index, 0, 0), mk_ext(hi_index, 0, 0)};   // rows >= out_rows are not written
  return run_vm(ctx, mod, *p, ex, 8, items);
}

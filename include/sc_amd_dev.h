/*
 * sc_amd_dev.h -- the rest of libsc_amd.so's C ABI: the primitives the scheme-level entry points of sc_amd.h are composed of, the
 * kernel-policy switches and the measurement probes.  A maintainer binding the reference's scheme packages needs none of this
 * (sc_amd.h is complete for that); it is the toolbox of this repository's generic ciphertext operator algebra (schemes.py),
 * tests, tools/ and bench.py.  Same conventions as sc_amd.h; handles (`mod`, `exp`, `cst`, `fbt`) are small integers valid for
 * the context that created them.
 */
#ifndef SC_AMD_DEV_H
#define SC_AMD_DEV_H

#include "sc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- kernel policies (defaults are right for production; tests and A/B runs force them) ------------------------------------ */
/* Small-batch policy.  A modulus in an L = 18 configuration can be worked on by twice the lanes with 9 limbs each (same limb
 * arrays in memory): twice the waves, 1.8x shorter dependent chains, lower multiply-add density.  mode 0: never; 1 (default):
 * when the L = 18 launch would leave at least half of the SIMDs without a wave; 2: whenever such a kernel exists (tests). */
int sc_ctx_set_latency_mode(sc_ctx* ctx, int mode);
/* Large-batch policy for moduli of at most 1028 bits (the primes p, q of 2048-bit keys: key-holder CRT, DGK zero test).  The
 * shared-exponent entry points sc_modexp_shared / _isone / _isone_any can run such a modulus in the one-lane configuration -- one
 * number per lane, 37 limbs of 28 bits, operands of a squaring in registers, modulus in scalar registers: 1.25x the rate per
 * number, but 64 numbers per wave (exponents of more than 64 bits only).  mode 0: never; 1 (default): whichever form a model of
 * both forms' rounds of resident waves says is faster for this batch size, with the per-round times MEASURED on this device
 * (sc_ctx_policy); 2: whenever the modulus fits (tests).  Results are the same canonical residues in every mode. */
int sc_ctx_set_onelane_mode(sc_ctx* ctx, int mode);
/* Chunk length of sc_modprod_axis' tree.  0 (default): automatic -- the shortest chains of at least 4 and at most 32 members that still
 * fill the chip's resident group slots at each level; 2 .. 32: that length at every level (tests reach deep trees at small K this
 * way).  Results are the same canonical residues whatever the setting. */
int sc_ctx_set_reduce_chunk(sc_ctx* ctx, int c);
/* Tell the context that `contexts` library contexts (this one included) work on its GPU at the same time -- the concurrent
 * shards of one batch, each on its own stream.  Batch-size policies then count rounds of 1/contexts of the chip (a launch that
 * under-fills the whole chip is not alone on it).  Default 1. */
int sc_ctx_set_chip_share(sc_ctx* ctx, int contexts);
/* Fork / join inside one call.  The p- and q-side of the key holder's CRT (sc_paillier_decrypt, sc_paillier_randomize with a secret
 * key) are independent; when a launch of the batch leaves room for a second one beside it (small batches) the q-side is queued on
 * a second stream of the context, with its own scratch arena and temporaries, and joined before the recombination.  mode 1
 * (default): automatic -- small batches as described (off when the latency mode is 0, forced on by latency mode 2: tests), and
 * large ones when the context has the chip to itself (chip share 1: launches of 1.5 rounds pack when they overlap); 0: never;
 * 2: always. */
int sc_ctx_set_fork_mode(sc_ctx* ctx, int mode);
/* Long pair launches on a shared chip.  The waves of a launch of few rounds retire together, so nothing another context queues
 * behind it gets a wave slot before a round ends: Alice's rho^N of a shard of 32768 is 2048 waves for 54 ms, and the other shard's
 * sub-millisecond launches were seen waiting 26 .. 33 ms each behind it.  A context that shares its GPU (sc_ctx_set_chip_share > 1)
 * therefore cuts such a launch (sc_modexp_shared_sq) into segments -- the same micro-program cut at window boundaries, the pair
 * parked in the item's table slot in between; same residues.  The decision uses MEASURED quantities only: the time a resident wave
 * holds its slot = the program's pair squarings and products times the per-op times of the kernel instance, measured on the device
 * once per process (a lone wave of the caller's operands, ~2 ms); the launch is cut when it would occupy more than half of the
 * chip's wave slots (by the runtime's occupancy answer) for at most `max_rounds` rounds, into round(hold / hold_ms) segments (at
 * most 16).  hold_ms: how long a wave may hold its slot, default 5 ms (environment SC_PAIR_HOLD_MS at context creation; 0 or
 * SC_PAIR_SEGMENTS=1: never cut); max_rounds default 2.5 (longer launches retire their waves a round apart already). */
int sc_ctx_set_pair_policy(sc_ctx* ctx, double hold_ms, double max_rounds);
/* Counters of the context since its creation: out[0] = pair launches that ran in segments, out[1] = segments queued for them,
 * out[2] = op-time calibrations this context performed (the others are zero).  For tests and tools. */
int sc_ctx_stats(sc_ctx* ctx, uint64_t* out, int n);
/* Launches per compiled interpreter instance since the context was created (counted on the host, next to each launch; the
 * calibration launches of the automatic policies count like any other).  Up to `cap` (key, count) entries in ascending key order go
 * to keys_out / counts_out (either may be NULL with cap 0); *n_out = the number of instances launched so far, which may exceed
 * `cap`.  The key names the template instance:
 *   bits 0..7 L, bits 8..15 G, bits 16..23 W (limb bits), bit 24 NEG1, bit 25 STAMP, bit 26 DIG, bit 27 kind (0 k_vm, 1 k_pvm),
 *   bit 28 k_prod_axis (sc_modprod_axis, and the totals of sc_modscan_axis; bits 24..27 zero);
 *   bit 29 k_scan_axis (sc_modscan_axis; bits 24..28 zero);
 *   bit 30 k_lin_axis (sc_modlin_axis; bits 24..29 zero), with bit 24 its lifting launch k_lin_lift (bits 25..29 zero);
 * STAMP and DIG are always 0 for k_vm.  For tests and tools: which instance a call landed on is host policy no result shows. */
int sc_ctx_launch_counts(sc_ctx* ctx, uint32_t* keys_out, uint64_t* counts_out, int cap, int* n_out);
/* The constants behind the automatic policies, measured once per device and process when the first secret key is created (about
 * 80 ms: full, half and one-and-a-half rounds of x^e mod p, 1024 bits, on the two-lane and on the one-lane kernel) instead of fitted
 * on one box: out[0..5] =
 * one-lane full round, one-lane half round, two-lane full round, two-lane half round, two-lane single half round (all in ms), and
 * the number of SIMDs the rounds were counted on.  Forces the calibration if it has not happened yet. */
int sc_ctx_policy(sc_ctx* ctx, double* out6);

/* ---- per-key setup (replaces what the scheme constructors precompute; [ext] Paillier/DGK __init__) ---- */
/* Register an odd modulus (Paillier N, N^2, p^2, q^2; DGK n, p).  nwords = words of every residue array. */
int sc_mod_create(sc_ctx* ctx, const uint32_t* n_hptr, int nwords, int* out_mod);
int sc_mod_words(sc_ctx* ctx, int mod);
/* Register an exponent shared by a whole batch (Paillier N or lambda, DGK v_p, 2^i, 3, ...). */
int sc_exp_create(sc_ctx* ctx, const uint32_t* e_hptr, int ewords, int* out_exp);
/* Register a constant residue (kept in Montgomery form on the device): g, g^-1, mu, N (mod N^2) ... */
int sc_const_create(sc_ctx* ctx, int mod, const uint32_t* v_hptr, int nwords, int* out_const);
/* Build the fixed-base table base^(d * 2^(window*j)) for exponents below 2^exp_bits, window 1 .. 24
 * (DGK h and g: the randomizers h^r of SC/initiator.py:153-154 and SC/keyholder.py:106-108). */
int sc_fbt_create(sc_ctx* ctx, int mod, const uint32_t* base_hptr, int exp_bits, int window, int* out_fbt);
/* Use a table another context of the same device built for the same modulus (a window-20 table for h is 6 GB, a window-24 one 82 GB: concurrent
 * shard contexts of one GPU read one copy).  The rows are read-only and reference-counted: they are freed when the last
 * context holding the table is destroyed.  `mod` must be `ctx`'s registration of the modulus the table was built for.  Call it
 * while `src_ctx` is idle (its table list is read without a lock); the imported table itself is safe to use from `ctx`'s thread
 * while `src_ctx` works. */
int sc_fbt_import(sc_ctx* ctx, int mod, sc_ctx* src_ctx, int src_fbt, int* out_fbt);
/* Device bytes of a table's rows (reported by bench.py next to the throughput that depends on them). */
int sc_fbt_bytes(sc_ctx* ctx, int fbt, uint64_t* out_bytes);

/* ---- batched residue arithmetic (the ciphertext operator algebra) ---------------- */
/* out[i] = a[i] * b[i] mod n.  Stride 0 broadcasts a single residue.  ct + ct (SC/initiator.py:254,
 * 476-483, 563), ct * randomizer (every .randomize()). */
int sc_modmul(sc_ctx* ctx, int mod, const uint32_t* a_dptr, int a_stride_words, const uint32_t* b_dptr,
              int b_stride_words, uint32_t* out_dptr, uint64_t count);
/* out[i] = a[i] * c mod n for a registered constant c (ct + int with int in {0,1}: SC/initiator.py:320,
 * 476, 484, 531). */
int sc_modmul_const(sc_ctx* ctx, int mod, const uint32_t* a_dptr, int cst, uint32_t* out_dptr, uint64_t count);
/* out[i] = a[i] * (flags[i] ? c1 : c0) mod n for registered constants (-1 = the residue 1), one byte flag per item: the
 * unrandomized DGK encryption of a bit folded into its randomizer, g^bit * h^r (SC/keyholder.py:213, 231 with :106-108) --
 * no array of g^bit values is ever materialised. */
int sc_modmul_const_sel(sc_ctx* ctx, int mod, const uint32_t* a_dptr, int cst0, int cst1, const uint8_t* flags_dptr,
                        uint32_t* out_dptr, uint64_t count);
/* out[i] = x[i]^e mod n [* mul_into[i]], e shared: Paillier rho^N mod N^2 (SC/initiator.py:109,
 * SC/keyholder.py:126-128), c^lambda (SC/keyholder.py:195), w^(2^i) (SC/initiator.py:406), w_sum^3 (:480).
 * x may be wider than the modulus (x_words > nwords): it is reduced first (DGK zero test works mod p). */
int sc_modexp_shared(sc_ctx* ctx, int mod, int exp, const uint32_t* x_dptr, int x_words,
                     const uint32_t* mul_into_dptr /* nullable */, uint32_t* out_dptr, uint64_t count);
/* out[i] = x[i]^e mod m^2 [* mul_into[i]] for a modulus that is a perfect square m^2 (Paillier N^2, and p^2 / q^2 in the key
 * holder's CRT), computed with Montgomery products modulo m only: elements are held as pairs (x0, x1), X = (x0 + x1 m)/R, and
 * the recorded Montgomery quotient of x0 y0 carries the overflow into the m-part -- 3.5 S^2 multiply-adds per squaring
 * instead of 6 S^2 (S = limbs of m), identical residues.  mod_m2 must be registered for m^2 with 2 * words(mod_m) words;
 * x: [count][x_words], x_words <= 4 * words(mod_m) (wider operands are reduced mod m^2 implicitly); out / mul_into:
 * [count][2 * words(mod_m)].  Available when sc_mod_supports_sq(mod_m) returns 1 (moduli up to 2080 bits), else
 * SC_ERR_UNSUPPORTED -- use sc_modexp_shared on mod_m2 then.  Same reference call sites as sc_modexp_shared. */
int sc_modexp_shared_sq(sc_ctx* ctx, int mod_m, int mod_m2, int exp, const uint32_t* x_dptr, int x_words,
                        const uint32_t* mul_into_dptr /* nullable */, uint32_t* out_dptr, uint64_t count);
int sc_mod_supports_sq(sc_ctx* ctx, int mod);
/* out[i] = prod_j x_j[i]^(e_j[i]) [* mul_into[i]] mod m^2, j < nbases (1 .. 3), with exponents PER ROW: the pair arithmetic of
 * sc_modexp_shared_sq driven by an interleaved fixed-window schedule whose products pick their table entry from the item's own
 * exponent bits (the batched twin of ct * k, and the exponentiations of a secure selection).  x: [nbases][count][x_words],
 * x_words <= 4 * words(mod_m); e: [nbases][count][ewords], bits at or above ebits ignored (ebits = 0: out = 1 [* mul_into]);
 * out / mul_into: [count][2 * words(mod_m)].  mod_m2 must be registered for m^2.  SC_ERR_UNSUPPORTED where
 * sc_mod_supports_sq(mod_m) is 0 or the modulus's pair configuration has no per-row instance (Paillier N of 1024, 2048 and
 * 3072 bits have one): compose sc_modexp_var on mod_m2 with sc_modmul then. */
int sc_modexp_var_sq(sc_ctx* ctx, int mod_m, int mod_m2, int nbases, const uint32_t* x_dptr, int x_words, const uint32_t* e_dptr,
                     int ewords, int ebits, const uint32_t* mul_into_dptr /* nullable */, uint32_t* out_dptr, uint64_t count);
/* flags[i] = (x[i]^e mod n == 1): DGK.is_zero, SC/keyholder.py:249 (e = v_p, n = p). */
int sc_modexp_shared_isone(sc_ctx* ctx, int mod, int exp, const uint32_t* x_dptr, int x_words,
                           uint8_t* flags_dptr, uint64_t count);
/* any_flags[b] = OR over the planes i of (x[i * inner + b]^e mod n == 1), b < inner, count = planes * inner items (bit-major):
 * the whole of KeyHolder.step_4j -- delta_B = any(is_zero(c_i)) (SC/keyholder.py:246-253) -- in the zero-test launch itself
 * (uint64 per comparison, 0 or 1; the array is cleared first). */
int sc_modexp_shared_isone_any(sc_ctx* ctx, int mod, int exp, const uint32_t* x_dptr, int x_words, uint64_t inner,
                               uint64_t* any_flags_dptr, uint64_t count);
/* out[i] = base^e[i] mod n [* mul_into[i]] with the fixed-base table: DGK randomize / encrypt
 * g^m h^r (SC/keyholder.py:106-108, 213, 231; SC/initiator.py:153-154). e: [count][ewords]. */
int sc_fixedbase_pow(sc_ctx* ctx, int fbt, const uint32_t* e_dptr, int ewords,
                     const uint32_t* mul_into_dptr /* nullable */, uint32_t* out_dptr, uint64_t count);
/* out[i] = x[i]^e[i] mod n [* base^e2[i]] with per-element exponents of at most ebits bits:
 * the blinding c_i^rho_i of SC/initiator.py:512 optionally fused with the randomizer h^r_i of :153-154. */
int sc_modexp_var(sc_ctx* ctx, int mod, const uint32_t* x_dptr, const uint32_t* e_dptr, int ewords, int ebits,
                  int fbt /* -1 = none */, const uint32_t* e2_dptr, int e2words, uint32_t* out_dptr,
                  uint64_t count);
/* The same with the result of item i stored at row dest_index[i] of out[count][nwords] (uint64 per item): the per-comparison
 * shuffle of the blinded c-vector (SC/initiator.py:212-226, :516) happens in the store of the blinding launch instead of a
 * separate gather pass over the 0.5 GB vector.  dest_index should be a permutation of 0 .. count-1; rows >= count are dropped
 * (never written out of bounds), rows named twice keep one of the values. */
int sc_modexp_var_scatter(sc_ctx* ctx, int mod, const uint32_t* x_dptr, const uint32_t* e_dptr, int ewords, int ebits,
                          int fbt /* -1 = none */, const uint32_t* e2_dptr, int e2words, const uint64_t* dest_index_dptr,
                          uint32_t* out_dptr, uint64_t count);
/* out[i] = x[i]^-1 mod n (Montgomery's simultaneous inversion + an on-device binary extended GCD):
 * ct * -1 / int - ct / ct - ct (SC/initiator.py:254, 320, 371, 466, 478, 531, 559).
 * Synchronous.  On SC_ERR_NOT_INVERTIBLE *bad_index (nullable) is the index of a non-invertible element (found by testing
 * the members of the failing chunk individually) and sc_last_error() names it; `out` is unspecified then.
 * `out` must not overlap `x` (SC_ERR_ARG): the operands are re-read on the error path.
 * Operands are canonical residues.  The inversion kernel reduces an operand below 4 n and refuses a larger one: SC_ERR_ARG
 * ("operand i is not reduced modulo n", *bad_index = i), never SC_ERR_NOT_INVERTIBLE. */
int sc_modinv(sc_ctx* ctx, int mod, const uint32_t* x_dptr, uint32_t* out_dptr, uint64_t count,
              int64_t* bad_index);
/* The product along one axis: x viewed as [outer][K][inner][nwords] canonical residues, out[o][i] = prod_{j < K} x[o][j][i] mod n,
 * [outer][inner][nwords] canonical.  A tree of launches of the dedicated kernel k_prod_axis on the context's stream, one per level:
 * a chain of at most 32 members per group of lanes and exactly one Montgomery product acc * x / R per member after the first -- no
 * operand is converted, no product reduced on its own, partials travel in limb form, lazily reduced.  Each product leaves a factor
 * 1 / R behind, K - 1 of them whatever the shape of the tree, and the last level's product with the constant R^K mod n (built on the
 * host once per modulus and K and copied on the context's stream from a pinned buffer) removes them: the shape of the tree does not
 * change the result.  Asynchronous, no host round trip.  K = 1 is a
 * canonical copy.  Operands must be canonical (below n): the kernel does not check them, and an unreduced operand gives an unspecified
 * residue (sc_modinv, whose kernel sees every operand anyway, reports one; this call would need a pass of its own).  A context keeps
 * the closing factors of the last 64 (modulus, K) pairs.  Checked before anything is launched or allocated (SC_ERR_ARG): null pointers, K >= 1,
 * outer * K * inner * nwords <= 2^40 words, `out` must not overlap `x`; an empty outer or inner is SC_OK.  The modulus runs in its own
 * configuration; one without an instance (one-lane (1,18), 28-bit limbs, modulus multiples) is SC_ERR_ARG and the message names the
 * configuration.  Launches are counted in sc_ctx_launch_counts under the key  L | G << 8 | 29 << 16 | 1 << 28. */
int sc_modprod_axis(sc_ctx* ctx, int mod, const uint32_t* x_dptr, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out_dptr);
/* The running product along one axis, inclusive: x viewed as [outer][K][inner][nwords] canonical residues,
 * out[o][j][i] = prod_{j' <= j} x[o][j'][i] mod n, canonical, in the shape of x.  Every position is an output, so nothing may drift:
 * the dedicated kernel k_scan_axis keeps the running prefix as the canonical residue it has just stored and pays two Montgomery
 * products per member (prefix * R^(e+2) / R, then * member / R, for a member that carries R^-e), with no conversion launch before and
 * no reduction launch after.  One launch, one chain per (o, i), when outer * inner chains fill the chip's resident group slots or K is
 * no longer than one chunk (sc_modprod_axis' chunk rule, sc_ctx_set_reduce_chunk included); otherwise reduce-then-scan: the totals of
 * the full chunks by one k_prod_axis level (limb form, drift R^-(chunk - 1), absorbed by the next level's constant), their inclusive
 * scan by the same plan, and one k_scan_axis launch in which chunk q starts from prefix q - 1.  All on the context's stream, no host
 * round trip; totals and prefixes live in one grow-only temporary; the level constants share sc_modprod_axis' table of R^e mod n.
 * Operands must be canonical, as for sc_modprod_axis, and the argument checks are that call's: null pointers, K >= 1,
 * outer * K * inner * nwords <= 2^40 words, `out` must not overlap `x`, an empty outer or inner is SC_OK, a modulus without an
 * instance is SC_ERR_ARG.  Launches are counted in sc_ctx_launch_counts under  L | G << 8 | 29 << 16 | 1 << 29  (the totals' under
 * bit 28). */
int sc_modscan_axis(sc_ctx* ctx, int mod, const uint32_t* x_dptr, uint64_t outer, uint64_t K, uint64_t inner, uint32_t* out_dptr);
/* Linear maps with public weights along one axis: x viewed as [outer][K][inner][nwords] canonical residues, w_host [J][K] unsigned
 * 64-bit weights on the host, out[o][j][i] = prod_{k < K} x[o][k][i]^w[j][k] mod n, [outer][J][inner][nwords] canonical.  Two launches
 * on the context's stream: k_lin_lift takes every member once to Montgomery form (one product with R^2; limb form, in a grow-only
 * temporary), then the dedicated kernel k_lin_axis runs one chain per output: the K bases of an output share one squaring chain (Straus),
 * from the Montgomery one, for every bit of the row's widest weight from the top one squaring -- none while the accumulator is still R
 * -- and one product per member whose weight has that bit, then one reduction pass and the canonical residue.  All groups of a wave
 * work on the same row j, so the weight bits are wave-uniform.  An all-zero row gives the residue 1, a row with a single weight 1 the
 * member itself.  The weights and the bit length of every row's widest one are copied to the device through a pinned buffer of the
 * context: w_host is free to reuse on return, and the call does not wait for the stream (only for the previous call's copy, should
 * it still be under way).  Operands must be canonical.  Checked before anything is launched or allocated (SC_ERR_ARG, the message names
 * the quantity): null pointers; outer, K, inner, J >= 1; K, J <= 1024; outer * K * inner * nwords and outer * J * inner * nwords <=
 * 2^40 words; `out` must not overlap `x`; a modulus without an instance (sc_modprod_axis' rule, the message names G=, L=, W=).
 * Launches are counted in sc_ctx_launch_counts under  L | G << 8 | 29 << 16 | 1 << 30, the lifting launch's with bit 24 as well. */
int sc_modlin_axis(sc_ctx* ctx, int mod, const uint32_t* x_dptr, uint64_t outer, uint64_t K, uint64_t inner, const uint64_t* w_host, uint64_t J,
                   uint32_t* out_dptr);

/* ---- Paillier pieces that are not plain residue products --------------------------------------- */
/* out[i] = 1 + m[i] * N mod N^2 (g = N+1 encryption without randomness: unsafe_encrypt(..) of
 * SC/initiator.py:256, 562; SC/keyholder.py:274-286).  mod_n2 = N^2, cst_n = sc_const_create(mod_n2, N).
 * m: [count][m_words], any m < 2^(32 m_words) (reduction mod N is implicit). */
int sc_paillier_encrypt_raw(sc_ctx* ctx, int mod_n2, int cst_n, const uint32_t* m_dptr, int m_words,
                            uint32_t* out_dptr, uint64_t count);
/* out[i] = 1 - m[i] * N mod N^2 = [[-m]] = [[m]]^-1: lets the Initiator form ([[r div 2^l]])^-1 of SC/initiator.py:559-563 without
 * a modular inversion. */
int sc_paillier_encrypt_raw_neg(sc_ctx* ctx, int mod_n2, int cst_n, const uint32_t* m_dptr, int m_words,
                                uint32_t* out_dptr, uint64_t count);
/* out[i] = ((x[i] - 1) / n) * k mod n for x[i] = 1 (mod n), x: [count][x_words]: the L function and the
 * mu multiplication of Paillier.decrypt (SC/keyholder.py:195).  mod = N (or p, q for CRT), cst_k = mu. */
int sc_paillier_l_mul(sc_ctx* ctx, int mod, int cst_k, const uint32_t* x_dptr, int x_words, uint32_t* out_dptr,
                      uint64_t count);

/* out[i] = the x in [0, m_p m_q) with x = a_p[i] (mod m_p), x = a_q[i] (mod m_q):  a_q + m_q ((a_p - a_q) m_q^-1 mod m_p).
 * Used by the key holder to recombine the CRT halves of decrypt (m_p = p, m_q = q; SC/keyholder.py:195) and of rho^N (m_p = p^2,
 * m_q = q^2; SC/keyholder.py:126-128); identical integers to the reference's single-modulus pow_mod.  Constants: cst_k = m_q^-1 mod m_p and cst_negk =
 * m_p - cst_k registered for mod_p, cst_mq = m_q registered for mod_full (= m_p m_q). */
int sc_crt_combine(sc_ctx* ctx, int mod_p, int mod_full, int cst_k, int cst_negk, int cst_mq, const uint32_t* a_p_dptr,
                   int a_p_words, const uint32_t* a_q_dptr, int a_q_words, uint32_t* out_dptr, uint64_t count);

/* ---- plaintext-side word arithmetic of the two parties (HBM-bound helpers) ------------------------ */
/* From r[count][nw] and the Paillier N: m1 = 2^l + r ([count][nw+1], SC/initiator.py:256), alpha = r mod 2^l
 * (:270), alpha_tilde = (r - N) mod 2^l (:373), rsmall = [r < (N-1)/2] (:289, :559), rshift = r >> l (:562).
 * 1 <= l <= 255.  alpha / alpha_tilde are flag rows of lw = ceil(l / 64) little-endian uint64 words per item ([count][lw], the
 * bits above l zero: one uint64 per item for l <= 64); rsmall is one uint64 per item.  l >= 32 nw is SC_ERR_ARG (m1 holds nw + 1
 * words); the same holds for sc_plain_bob. */
int sc_plain_alice(sc_ctx* ctx, const uint32_t* r_dptr, const uint32_t* n_hptr, int nw, int l, uint64_t count,
                   uint32_t* m1_dptr, uint64_t* alpha_dptr, uint64_t* alpha_tilde_dptr, uint64_t* rsmall_dptr,
                   uint32_t* rshift_dptr);
/* From z[count][nw]: beta = z mod 2^l (SC/keyholder.py:196), dbit = [z < (N-1)/2] (:213), zeta1 = z >> l,
 * zeta2 = (z + N) >> l if dbit else z >> l (:274-282).  1 <= l <= 255; beta is a flag row [count][ceil(l/64)] uint64, dbit one
 * uint64 per item. */
int sc_plain_bob(sc_ctx* ctx, const uint32_t* z_dptr, const uint32_t* n_hptr, int nw, int l, uint64_t count,
                 uint64_t* beta_dptr, uint64_t* dbit_dptr, uint32_t* zeta1_dptr, uint32_t* zeta2_dptr);

/* ---- secure division: the plaintext-word long division of both players ------------------------------------------- */
/* q [count][nw] = x div d and rem [count] = x mod d, row by row, for x [count][nw] (nw >= 1 words) and d [count] uint64 divisors, all
 * device arrays (k_divmod_words: Knuth's algorithm D, one thread per row).  q may be x itself -- the division then runs in place -- or
 * an array apart from x; a q that partly overlaps x, a rem that overlaps x, q or d, a d that overlaps q, a null pointer and nw < 1 are
 * SC_ERR_ARG before anything is launched.  A row whose divisor is ZERO is an error the call cannot see when it queues the launch: the
 * kernel writes that row's q and rem as zero, divides nothing and sets a flag word of the context, and the next sc_ctx_synchronize of
 * the context returns SC_ERR_ARG once (and clears the flag).  Never a device fault. */
int sc_plain_divmod(sc_ctx* ctx, const uint32_t* x_dptr, int nw, const uint64_t* d_dptr, uint64_t count, uint32_t* q_dptr,
                    uint64_t* rem_dptr);

/* ---- secure selection ("Secure selection"): the plaintext-word halves of the two players -------------- */
/* Layout of the packed plaintext of P = [[delta]] prod_j [[d_j]]^(2^off_j) (1 + R N) rho^N, low bits first: a = delta + r_a in
 * [0, s), s = kappa + 1, then field j = d_j + r_b_j (d_j < 2^(widths[j] + 1)) of widths[j] + kappa + 2 bits; nfields <= 4,
 * 1 <= kappa <= 62.  Both calls return SC_ERR_ARG when the fields, or one product a * b_j, would not fit below N (n_hptr, nw words).
 * sc_select_prep (initiator): from r_a [count][aw] (aw <= 2, r_a < 2^kappa) and r_b [nfields][count][bw]: R = r_a + sum_j
 * 2^off_j r_b_j [count][nw], e_j = r_b_j + 2^widths[j] [nfields][count][ew], rab_j = r_a r_b_j [nfields][count][nw]. */
int sc_select_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int nfields, const int* widths_hptr,
                   const uint32_t* r_a_dptr, int aw, const uint32_t* r_b_dptr, int bw, int ew, uint32_t* R_dptr, uint32_t* e_dptr,
                   uint32_t* rab_dptr, uint64_t count);
/* sc_select_split (key holder): from the decrypted P [count][nw]: prod_j = a * b_j [nfields][count][nw].  *bad_dptr (one uint32,
 * not cleared here) is set to 1 when a row has a bit at or above the end of the last field: the initiator packed a WIDER layout
 * than the one given here.  A narrower one cannot be detected from P; the two players' layouts must be compared as well
 * (selection.py announces it in the message that carries P). */
int sc_select_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int nfields, const int* widths_hptr,
                    const uint32_t* p_dptr, uint32_t* prod_dptr, uint32_t* bad_dptr, uint64_t count);
/* ---- secure multiplication: the plaintext-word halves of the two players ------------------------- */
/* Layout of the packed plaintext of P = [[x]] prod_j [[y_j]]^(2^off_j) (1 + R N) rho^N, low bits first: A = x + e_y in [0, s),
 * s = wx + kappa + 1, then field j = B_j = y_j + e_x_j of wy[j] + kappa + 1 bits; nfields <= 4, 1 <= kappa <= 62, 1 <= wx, wy[j] <= 255.
 * Both calls return SC_ERR_ARG when the fields, or one product A * B_j, would not fit below N (n_hptr, nw words).  Every field may
 * span several words: the products are multi-word by multi-word.
 * sc_mul_prep (initiator): from r_a [count][aw] (< 2^(wx + kappa)) and r_b [nfields][count][bw] (column j < 2^(wy[j] + kappa)),
 * aw, bw <= 10: e [nfields + 1][count][ew] with e[j] = e_x_j = r_b_j + oy_j and e[nfields] = e_y = r_a + ox (ox = 2^(wx - 1),
 * oy_j = 2^(wy[j] - 1) when is_signed, else 0), R = e_y + sum_j 2^off_j e_x_j [count][nw], rab_j = e_x_j e_y [nfields][count][nw].
 * 32 ew >= max(s, max_j fbits_j). */
int sc_mul_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int nfields, const int* wy_hptr, int is_signed,
                const uint32_t* r_a_dptr, int aw, const uint32_t* r_b_dptr, int bw, int ew, uint32_t* R_dptr, uint32_t* e_dptr,
                uint32_t* rab_dptr, uint64_t count);
/* sc_mul_split (key holder): from the decrypted P [count][nw]: prod_j = A * B_j [nfields][count][nw].  *bad_dptr as sc_select_split's:
 * set to 1 (never cleared here) when a row has a bit at or above the end of the last field. */
int sc_mul_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int nfields, const int* wy_hptr,
                 const uint32_t* p_dptr, uint32_t* prod_dptr, uint32_t* bad_dptr, uint64_t count);
/* ---- secure inner product: the plaintext-word halves of the two players ----------------------------- */
/* A row has k pairs (A_j, B_j), A_j = x_j + a_j of sa = wx + kappa + 1 bits and B_j = y_j + b_j of sb = wy + kappa + 1 bits, pb = sa + sb
 * bits per pair, g = the largest integer with g pb < bits(N) - 1 pairs per message and M = ceil(k / g) messages per row; pair j lives in
 * message j mod M at position t = j div M, A in bits [t pb, t pb + sa), B above it.  square != 0: every pair is the one field A_j
 * (sb = 0, pb = sa; wy, r_b and y are not read).  Layout (sc_dot_layout's rule): 1 <= kappa <= 62, 1 <= wx, wy <= 255, 1 <= k <= 1024,
 * g >= 1 and pb' + ceil(log2 k) < bits(N) - 1 with pb' = sa + sb (2 sa for a square); SC_ERR_ARG otherwise, against N (n_hptr, nw words).
 * sc_dot_prep (initiator): from r_a [k][count][aw] (< 2^(wx + kappa)) and r_b [k][count][bw] (< 2^(wy + kappa)), aw, bw <= 10, every
 * field with a mask of its own: with a_j = r_a_j + ox, b_j = r_b_j + oy (ox = 2^(wx - 1), oy = 2^(wy - 1) when is_signed, else 0),
 * e [2k][count][ew]: planes 0 .. k-1 = b_j (the exponents of x_j), planes k .. 2k-1 = a_j (the exponents of y_j); R [M][count][nw] the
 * packed masks of every message; S [count][nw] = sum_j a_j b_j.  Square: e [k][count][ew] = 2 a_j, S = sum_j a_j^2.  32 ew >= ebits. */
int sc_dot_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int wy, int is_signed, int square, int k,
                const uint32_t* r_a_dptr, int aw, const uint32_t* r_b_dptr /* nullable when square */, int bw, int ew, uint32_t* e_dptr,
                uint32_t* R_dptr, uint32_t* S_dptr, uint64_t count);
/* sc_dot_split (key holder): from the decrypted P [M][count][nw]: D [count][nw] = sum_j A_j B_j (square: sum_j A_j^2).  *bad_dptr (one
 * uint32, never cleared here) is set to 1 when a message has a bit at or above its OWN end n_m pb, n_m = the pairs it holds. */
int sc_dot_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int wx, int wy, int square, int k, const uint32_t* p_dptr,
                 uint32_t* D_dptr, uint32_t* bad_dptr, uint64_t count);
/* ---- secure one-hot encoding: the plaintext-word kernels of the two players ------------------------------------------ */
/* Layout as sc_onehot_layout's (include/sc_amd.h), against N (n_hptr, nw words): field q of a row, d_q = i_q + r_q of f = ib + kappa + 1
 * bits, lives in message q div g at bits [(q mod g) f, (q mod g + 1) f); message mm holds n_mm = min(g, m - mm g) fields.
 * sc_onehot_prep (initiator): from r [m][count][rw] (< 2^(ib + kappa), rw <= 3, 32 rw >= ib + kappa): R [M][count][nw], the masks of
 * every message at their bit offsets, and rot [m][count] int32 = r mod k over all the words of r. */
int sc_onehot_prep(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int ib, int k, int m, const uint32_t* r_dptr, int rw,
                   uint32_t* R_dptr, int32_t* rot_dptr, uint64_t count);
/* sc_onehot_split (key holder): from the decrypted P [M][count][nw]: prod [m][k][count][nw] with prod[q][t][b] = [t == d_q mod k] (the
 * remainder over all the words of the field).  *bad_dptr (one uint32, never cleared here) is set to 1 when a message has a bit at or
 * above its OWN end n_mm f. */
int sc_onehot_split(sc_ctx* ctx, const uint32_t* n_hptr, int nw, int kappa, int ib, int k, int m, const uint32_t* p_dptr,
                    uint32_t* prod_dptr, uint32_t* bad_dptr, uint64_t count);
/* sc_onehot_rotate (initiator): out[q][t][b] = e[q][(t + rot[q][b]) mod k][b] for rows of `words` words, e and out [m][k][count][words],
 * rot [m][count] int32.  The kernel reduces rot modulo k as an UNSIGNED 32-bit number, so no value of it reads outside e: for
 * 0 <= rot < 2^31 that is rot mod k; a negative rot turns by (2^32 + rot) mod k, which is the mathematical residue only where k divides
 * 2^32.  The library's own callers pass 0 .. k - 1.  out must not overlap e (SC_ERR_ARG). */
int sc_onehot_rotate(sc_ctx* ctx, int words, int k, int m, const uint32_t* e_dptr, const int32_t* rot_dptr, uint32_t* out_dptr,
                     uint64_t count);
/* sc_select_finish_cx (initiator, the compare-exchange of a secure sort): from a selection with sigma = delta,
 * base F and d = G - F + 2^w, both outputs hi = F ab^2 u_inv and lo = G t^2 u_inv modulo mod (N^2), where u_inv = (t ab)^-1.
 * t, ab, u_inv, f, g: [nfields][count][words(mod)], nfields 1 .. 4.  lo_index / hi_index (both or neither): uint64 [nfields][count],
 * the row of out [out_rows][words(mod)] that the lo / hi output of each column and item goes to; rows >= out_rows are not written.
 * Both null: out is [2][nfields][count][words(mod)] = (lo, hi), out_rows >= 2 nfields count. */
int sc_select_finish_cx(sc_ctx* ctx, int mod, int nfields, const uint32_t* t_dptr, const uint32_t* ab_dptr, const uint32_t* u_inv_dptr,
                        const uint32_t* f_dptr, const uint32_t* g_dptr, const uint64_t* lo_index_dptr /* nullable */,
                        const uint64_t* hi_index_dptr /* nullable */, uint32_t* out_dptr, uint64_t out_rows, uint64_t count);

/* ---- fused Initiator steps 4c-4h (SC/initiator.py:272-485) --------------------------------------- */
/* Inputs, all bit-major: beta[l][count][nw], beta_inv[l][count][nw], d[count][nw], d_inv[count][nw]
 * (DGK ciphertexts mod n and their inverses), alpha / alpha_tilde flag rows [count][ceil(l/64)] uint64 (1 <= l <= 255),
 * rsmall / delta_a uint64 per comparison,
 * cst_g / cst_ginv = registered g and g^-1.  Output c[l+1][count][nw] in the order c_-1, c_0 .. c_{l-1}
 * (SC/initiator.py:484), not blinded. */
int sc_dgk_step4(sc_ctx* ctx, int mod, int cst_g, int cst_ginv, int l, const uint32_t* beta_dptr,
                 const uint32_t* beta_inv_dptr, const uint32_t* d_dptr, const uint32_t* d_inv_dptr,
                 const uint64_t* alpha_dptr, const uint64_t* alpha_tilde_dptr, const uint64_t* rsmall_dptr,
                 const uint64_t* delta_a_dptr, uint32_t* c_out_dptr, uint64_t count);

/* ---- measurement -------------------------------------------------------------------------------- */
/* Runs an on-device v_mad_u64_u32 issue-rate probe; returns lane-MACs per second (the VALU-integer peak
 * used as the roofline denominator).  Synchronous. */
int sc_peak_probe(sc_ctx* ctx, double* out_mac_per_s);
/* Number of Montgomery limb-products (v_mad_u64_u32 lane operations) issued by library calls since the
 * last reset -- counted on the host from the micro-programs, used for the roofline numerator. */
int sc_mac_counter(sc_ctx* ctx, int reset, double* out_macs);
/* Measurement aid (bench / profiles only, no reference counterpart): per item, write `entries` rows of the per-slot scratch
 * table and read rows back `reads` times with the kernels' own limb-form access pattern, then store the last row read
 * (= x) to out[count][nwords].  Known HBM bytes per item: entries * S * 4 written, reads * S * 4 read (S = *out_row_limbs),
 * plus one operand in and out -- the calibration point for the FETCH_SIZE / WRITE_SIZE counters of this access pattern. */
int sc_table_traffic_probe(sc_ctx* ctx, int mod, const uint32_t* x, uint32_t* out, uint64_t count, int entries, int reads,
                           int* out_row_limbs);
/* In-kernel clock of the dominant launch (diagnostic, never a timed kernel): runs rho^N mod N^2 for `count` items of `paillier_key`
 * (a public key: the pair launch k_pvm<4,18,neg1>) on a twin of the kernel whose waves stamp s_memtime (shader clock) and
 * s_memrealtime (constant-rate clock) at entry and exit.  *out_ghz = mean over waves of d(memtime) / d(realtime) x the
 * constant clock's rate -- the engine clock the kernel actually held; *out_ms = the launch's duration by HIP events.  bench.py
 * calls it before the warm-up and after the timed loop (roofline.clock_ghz_before / _after).  Synchronous. */
int sc_clock_probe(sc_ctx* ctx, int paillier_key, const uint32_t* rho_dptr, uint64_t count, double* out_ghz, double* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* SC_AMD_DEV_H */
